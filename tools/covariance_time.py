#!/usr/bin/env python3
"""Covariance on the BAL-49 shape (developer tool; the record profiles/covariance_time.txt).

usage: covariance_time.py OUT.txt [cameras points observations]
       covariance_time.py --schur OUT.txt      (the record profiles/covariance_schur_time.txt; see schur_main below)

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


def _bal_problem(prob):
    C = prob.num_cameras
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    loss = sk.PredefinedLossFunctions.trivialLoss()
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    for i in (0, 1):
        problem.setParameterBlockConstant(params.slice(9 * i))
    return problem, params, loss


def _timed(cov, request, problem, runs=5):
    out = []
    for run in range(runs + 1):   # the first one is the warm-up
        t = time.perf_counter()
        ok = cov.compute(request, problem)
        wall = time.perf_counter() - t
        if not ok:
            raise SystemExit("compute failed: " + cov.lastError())
        if run:
            out.append([wall] + [cov.stat("phase_seconds_%d" % i) for i in range(5)])
    return [statistics.median(r[i] for r in out) for i in range(6)], out


def schur_main(path):
    """Covariance with the Schur elimination (sk_covariance_options_set_schur_elimination) on two shapes:
      BAL-49        bal.generate(49, 7776, 31843), cameras 0 and 1 constant, all camera-camera pairs (k = 423), beside the dense route's
                    figures, which are READ FROM profiles/covariance_time.txt (not measured again, not taken from the code under test);
      Ladybug-1723  bal.generate_named("ladybug-1723-156502"), cameras 0 and 1 constant (N = 485 013): all pairs among cameras 100..146 and
                    the diagonal blocks of the three widest tracks; the Schur update is stated as the bytes it must read (two tiles of at
                    most 27 doubles per term) against the HBM copy rate, the factorisation as n^3 / 3 + n^2 (border rows) flops; the host
                    plan is timed through sk_covariance_elimination_plan (the same plan without requests)."""
    if sk.device_count() < 1:
        raise SystemExit("covariance_time needs a HIP device")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dense = [ln.strip() for ln in open(os.path.join(here, "profiles", "covariance_time.txt")) if "device phases (ms)" in ln or "five computes" in ln]
    o = sk.Covariance.Options()
    o.schurElimination(True)
    lines = []
    # BAL-49
    prob = bal.generate(49, 7776, 31843)
    problem, params, keep = _bal_problem(prob)
    cams = [params.slice(9 * i) for i in range(2, prob.num_cameras)]
    cov = sk.Covariance(o)
    med, runs = _timed(cov, cams, problem)
    lines += ["BAL-49: bal.generate(49, 7776, 31843), cameras 0 and 1 constant, all camera-camera pairs: N = %d columns, %d eliminated blocks, %d reduced columns, k = %d selected, %d Schur terms"
              % (cov.stat("columns"), cov.stat("eliminated_blocks"), cov.stat("reduced_columns"), cov.stat("selected_columns"), cov.stat("schur_terms")),
              "  Schur route, five computes after a warm-up; medians.  wall %.1f ms (host clock, plan and uploads included); reciprocal pivot ratio %.3e" % (1e3 * med[0], cov.stat("reciprocal_pivot_ratio")),
              "  Schur route, device phases (ms): evaluation %.3f, assembly to Schur update %.3f, factorisation %.3f, extraction %.3f, downloads %.3f" % tuple(1e3 * v for v in med[1:]),
              "  every run (ms): " + "; ".join(" ".join("%.2f" % (1e3 * v) for v in r) for r in runs),
              "  dense route, from profiles/covariance_time.txt:"] + ["    " + ln for ln in dense]
    d = np.sqrt(np.diag(cov.getCovarianceBlock(cams[0], cams[0])))
    lines.append("  standard deviations of camera 2: " + " ".join("%.3e" % v for v in d))
    del cov, problem, params
    # Ladybug-1723
    t = time.perf_counter()
    prob = bal.generate_named("ladybug-1723-156502")
    gen = time.perf_counter() - t
    C, P = prob.num_cameras, prob.num_points
    problem, params, keep = _bal_problem(prob)
    t = time.perf_counter()
    plan = sk.Covariance.eliminationPlan(problem)
    plan_s = time.perf_counter() - t
    track = np.bincount(prob.point_index, minlength=P)
    widest = [int(q) for q in np.argsort(-track, kind="stable")[:3]]
    cam = lambda i: params.slice(9 * i)             # noqa: E731
    pt = lambda q: params.slice(9 * C + 3 * q)      # noqa: E731
    window = list(range(100, 147))
    request = [(cam(a), cam(b)) for i, a in enumerate(window) for b in window[i:]] + [(pt(q), pt(q)) for q in widest]
    cov = sk.Covariance(o)
    med, runs = _timed(cov, request, problem, runs=3)
    nF, k, terms = int(cov.stat("reduced_columns")), int(cov.stat("selected_columns")), int(cov.stat("schur_terms"))
    n = (nF + 127) // 128 * 128
    npad = n + (k + 127) // 128 * 128
    flops = n ** 3 / 3.0 + float(n) * n * (npad - n) + float(n) * (npad - n) ** 2   # the border's own trailing update is not small here
    bytes_update = 8.0 * 2 * 27 * terms
    lines += ["",
              "Ladybug-1723: bal.generate_named('ladybug-1723-156502') (%.1f s to generate), cameras 0 and 1 constant: N = %d columns, %d eliminated blocks (of %d points), %d reduced columns"
              % (gen, cov.stat("columns"), cov.stat("eliminated_blocks"), P, nF),
              "  requests: all pairs among cameras 100..146 (%d pairs) and the diagonal blocks of the three widest tracks (points %s, seen by %s cameras): k = %d selected columns"
              % (len(request) - 3, widest, [int(track[q]) for q in widest], k),
              "  three computes after a warm-up; medians.  wall %.1f ms (host clock); host plan alone (sk_covariance_elimination_plan) %.1f ms; reciprocal pivot ratio %.3e"
              % (1e3 * med[0], 1e3 * plan_s, cov.stat("reciprocal_pivot_ratio")),
              "  device phases (ms): evaluation %.3f, assembly to Schur update %.3f, factorisation %.3f, extraction %.3f, downloads %.3f" % tuple(1e3 * v for v in med[1:]),
              "  every run (ms): " + "; ".join(" ".join("%.2f" % (1e3 * v) for v in r) for r in runs),
              "  Schur update, stated: %d terms x two tiles of at most 27 doubles = at most %.1f MB read: %.3f ms at the HBM copy rate (the phase also zeroes %.2f GB of dense matrix and %.2f GB of tiles)"
              % (terms, bytes_update / 1e6, 1e3 * bytes_update / HBM_COPY_BYTES_PER_S, 8.0 * npad * npad / 1e9, 8.0 * 256 * (2 * plan["num_eliminated"] + prob.num_observations) / 1e9),
              "  factorisation, stated: n^3 / 3 + n^2 b + n b^2 (n = %d, b = %d border rows) = %.3e flops: %.2f ms at the 51 TFLOP/s this SYRK sustains; measured %.2f ms = %.1f TFLOP/s"
              % (n, npad - n, flops, 1e3 * flops / 51e12, 1e3 * med[3], flops / max(med[3], 1e-12) / 1e12)]
    d = np.sqrt(np.diag(cov.getCovarianceBlock(cam(100), cam(100))))
    lines.append("  standard deviations of camera 100: " + " ".join("%.3e" % v for v in d))
    d = np.sqrt(np.diag(cov.getCovarianceBlock(pt(widest[0]), pt(widest[0]))))
    lines.append("  standard deviations of point %d: " % widest[0] + " ".join("%.3e" % v for v in d))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--schur":
        schur_main(sys.argv[2])
    else:
        main(sys.argv)
