#!/usr/bin/env python3
"""Covariance on the BAL-49 shape (developer tool; the record profiles/covariance_time.txt).

usage: covariance_time.py OUT.txt [cameras points observations]

bal.generate(49, 7776, 31843), cameras 0 and 1 constant (N = 23 751 columns), the covariance of all camera-camera pairs (k = 423):
the median of five computes, the five phases from HIP events ("phase_seconds_0..4" of sk_covariance_stat), and what two of them are
measured against —
  assembly       the bytes it must move: the values read once per pair term (num_residuals x (size_i + size_j) doubles) and each tile
                 of H written once, against the HBM copy rate of profiles/r01_mfma_f64_peak_microbench.txt.  The memset of the dense
                 matrix and the scaling pass (read + write of the lower triangle) belong to the same phase and are stated next to it;
  factorisation  n^3 / 3 flops (n = N padded to 128; the border adds n^2 x its rows) at the fp64 matrix peak of the datasheet, 78.6
                 TFLOP/s (the package sustains about 50 under fp64-MFMA load, same file).
No target is set: stated, then measured.  Without a device the tool fails; the record then says that no run happened."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402

HBM_COPY_BYTES_PER_S = 4.99e12   # profiles/r01_mfma_f64_peak_microbench.txt: HBM copy, read + write
FP64_MATRIX_FLOPS = 78.6e12      # datasheet; mfma_f64_16x16x4 on 256 CUs sustains 49.0 in the same file


def main(argv):
    path = argv[1]
    shape = tuple(int(v) for v in argv[2:5]) if len(argv) >= 5 else (49, 7776, 31843)
    if sk.device_count() < 1:
        raise SystemExit("covariance_time needs a HIP device")
    prob = bal.generate(*shape)
    C, P = prob.num_cameras, prob.num_points
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    loss = sk.PredefinedLossFunctions.trivialLoss()
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    for i in (0, 1):
        problem.setParameterBlockConstant(params.slice(9 * i))
    cams = [params.slice(9 * i) for i in range(2, C)]
    cov = sk.Covariance()
    runs = []
    for run in range(6):   # the first one is the warm-up: code objects, the first launches
        t = time.perf_counter()
        ok = cov.compute(cams, problem)
        wall = time.perf_counter() - t
        if not ok:
            raise SystemExit("compute failed: " + cov.lastError())
        if run:
            runs.append([wall] + [cov.stat("phase_seconds_%d" % i) for i in range(5)])
    med = [statistics.median(r[i] for r in runs) for i in range(6)]
    N, k, pairs = int(cov.stat("columns")), int(cov.stat("selected_columns")), int(cov.stat("normal_matrix_pairs"))
    n = (N + 127) // 128 * 128
    npad = n + (k + 127) // 128 * 128
    # the assembly's bytes from the problem's shape: an observation is the terms (camera, camera), (point, point) and (camera, point)
    moving = prob.camera_index >= 2
    terms = int(prob.num_observations + 2 * moving.sum())
    read = 8 * 2 * int((9 + 9) * moving.sum() + (3 + 3) * prob.num_observations + (9 + 3) * moving.sum())
    cam_pt = len({(int(c), int(p)) for c, p in zip(prob.camera_index[moving], prob.point_index[moving])})
    written = 8 * (81 * (C - 2) + 9 * P + 27 * cam_pt)
    flops = n ** 3 / 3.0 + float(n) * n * (npad - n)
    d = np.sqrt(np.diag(cov.getCovarianceBlock(cams[0], cams[0])))
    lines = ["covariance: bal.generate%s, cameras 0 and 1 constant: N = %d columns, k = %d selected, %d normal-matrix pairs (%d terms), dense matrix %d^2 doubles = %.2f GB"
             % (shape, N, k, pairs, terms, npad, 8.0 * npad * npad / 1e9),
             "  five computes after a warm-up; medians.  wall %.1f ms (host clock, plan and uploads included); reciprocal pivot ratio %.3e" % (1e3 * med[0], cov.stat("reciprocal_pivot_ratio")),
             "  device phases (ms): evaluation %.3f, assembly and scaling %.3f, factorisation %.3f, extraction %.3f, downloads %.3f" % tuple(1e3 * v for v in med[1:]),
             "  every run (ms): " + "; ".join(" ".join("%.2f" % (1e3 * v) for v in r) for r in runs),
             "  assembly, stated: %.2f MB of values read (once per pair term) + %.2f MB of H tiles written (once each) = %.2f MB: %.4f ms at the HBM copy rate."
             % (read / 1e6, written / 1e6, (read + written) / 1e6, 1e3 * (read + written) / HBM_COPY_BYTES_PER_S),
             "    the same phase also zeroes the dense matrix (%.2f GB written) and scales the lower triangle of H (%.2f GB read + written): %.3f ms at that rate."
             % (8.0 * npad * npad / 1e9, 8.0 * N * N / 1e9, 1e3 * (8.0 * npad * npad + 8.0 * N * N) / HBM_COPY_BYTES_PER_S),
             "    measured: %.3f ms for the phase (allocation of the matrix, its memset, both assembly launches, both scaling launches)" % (1e3 * med[2]),
             "  factorisation, stated: n^3 / 3 + n^2 (border rows) = %.3e flops: %.2f ms at the fp64 matrix peak of %.1f TFLOP/s; measured %.2f ms = %.1f TFLOP/s (%.0f %% of it)"
             % (flops, 1e3 * flops / FP64_MATRIX_FLOPS, FP64_MATRIX_FLOPS / 1e12, 1e3 * med[3], flops / max(med[3], 1e-12) / 1e12, 100 * flops / FP64_MATRIX_FLOPS / max(med[3], 1e-12)),
             "  standard deviations of camera 2: " + " ".join("%.3e" % v for v in d)]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv)
