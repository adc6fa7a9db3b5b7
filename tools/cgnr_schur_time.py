#!/usr/bin/env python3
"""CGNR with and without the Schur elimination on a synthetic bundle-adjustment problem (developer tool; the record
profiles/cgnr_schur_time.txt).

usage: cgnr_schur_time.py OUT.txt [cameras] [points] [observations] [repeats]

A skeres_amd.bal.generate problem (default 600 cameras, 60 000 points, 300 000 observations; cameras 0 and 1 constant) is solved
by CGNR to its own convergence in one build, one process: the option off (the code path without this feature) and on, alternating,
`repeats` times each after one warm-up solve of each.  Per run: LM iterations, total CG iterations, device ms per CG iteration
(the CG loop's phase between HIP events over its iterations), wall time of the stepping loop (a host clock; every step ends in a
synchronise), and the rate that charges the CG loop's whole time to the 16 bytes per stored entry that the two products read, as
tools/cgnr_time.py states it (with the elimination the projection reads E's entries again: the figure stays per stored entry).

Without a device the tool fails; no record is written then."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402


def solve(prob, schur, max_iterations=50):
    C = prob.num_cameras
    params = sk.RichDoubleArray.fromArray(prob.parameters.copy())
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    loss = sk.PredefinedLossFunctions.trivialLoss()
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    for i in (0, 1):
        problem.setParameterBlockConstant(params.slice(9 * i))
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.CGNR)
    o.setMaxNumIterations(max_iterations)
    o.setSchurElimination(schur)
    t = time.perf_counter()
    solver = sk.StepSolver(o, problem)
    setup = time.perf_counter() - t
    summary = sk.Solver.Summary()
    t = time.perf_counter()
    while not solver.step():
        pass
    wall = time.perf_counter() - t
    solver.finish(summary)
    out = dict(setup=setup, wall=wall, iterations=len(summary.iterations()) - 1, initial=summary.initialCost(), final=summary.finalCost(),
               message=summary.message(), phases=[summary.phaseSeconds(k) for k in range(5)])
    for nm in ("cg_iterations", "cg_batches", "jacobian_nonzeros", "linear_solves", "eliminated_blocks", "reduced_columns", "schur_diagonal_pairs"):
        out[nm] = solver.stat(nm)
    return out


def main(argv):
    path = argv[1]
    C, P, N = (int(argv[k]) if len(argv) > k else d for k, d in ((2, 600), (3, 60000), (4, 300000)))
    repeats = int(argv[5]) if len(argv) > 5 else 3
    if sk.device_count() < 1:
        raise SystemExit("cgnr_schur_time needs a HIP device")
    prob = bal.generate(C, P, N, seed=7)
    lines = ["CGNR with and without the Schur elimination (tools/cgnr_schur_time.py; one MI355X, JACOBI, eta 0.1, the default tolerances).",
             "bal.generate(%d, %d, %d, seed=7), cameras 0 and 1 constant; one process, the two settings alternating, %d runs each after a warm-up of each."
             % (C, P, N, repeats),
             "Wall: host clock around the stepping loop.  ms per CG iteration: the CG loop's device phase (HIP events) over its iterations.",
             "GB/s: 16 bytes per stored entry per CG iteration over the CG loop's time (the whole loop charged to the products' reads).", ""]
    for schur in (False, True):
        solve(prob, schur, 3)
    runs = {False: [], True: []}
    for rep in range(repeats):
        for schur in (False, True):
            r = solve(prob, schur)
            runs[schur].append(r)
            nnz, cg = r["jacobian_nonzeros"], max(r["cg_iterations"], 1)
            r["ms_per_cg"] = 1e3 * r["phases"][2] / cg
            r["gbs"] = 16.0 * nnz * cg / max(r["phases"][2], 1e-12) / 1e9
            lines += ["elimination %s, run %d: %d LM iterations, %d CG iterations in %d batches; cost %.6e -> %.9e (%s)"
                      % ("on " if schur else "off", rep, r["iterations"], r["cg_iterations"], r["cg_batches"], r["initial"], r["final"], r["message"]),
                      "  set-up %.1f ms; wall %.1f ms; device phases (ms): evaluation %.3f, block sums + factors%s %.3f, CG loop %.3f, %smodel + candidate %.3f, cost %.3f"
                      % ((1e3 * r["setup"], 1e3 * r["wall"], 1e3 * r["phases"][0], " + diagonal of S + s" if schur else "", 1e3 * r["phases"][1], 1e3 * r["phases"][2],
                          "back-substitution + " if schur else "", 1e3 * r["phases"][3], 1e3 * r["phases"][4])),
                      "  %.4f ms per CG iteration; %d stored entries; %.1f GB/s%s"
                      % (r["ms_per_cg"], nnz, r["gbs"], "; %d blocks eliminated, %d reduced columns, %d (F, e) pairs"
                         % (r["eliminated_blocks"], r["reduced_columns"], r["schur_diagonal_pairs"]) if schur else "")]
    med = {s: {f: statistics.median(r[f] for r in runs[s]) for f in ("wall", "ms_per_cg", "gbs")} for s in runs}
    lines += ["", "medians            LM iterations   CG iterations   ms per CG iteration   wall ms to the final cost   GB/s"]
    for schur in (False, True):
        r = runs[schur][0]
        lines.append("elimination %s   %13d   %13d   %19.4f   %25.1f   %6.1f" % ("on " if schur else "off", r["iterations"], r["cg_iterations"], med[schur]["ms_per_cg"],
                                                                                 1e3 * med[schur]["wall"], med[schur]["gbs"]))
    ratio = med[True]["ms_per_cg"] / med[False]["ms_per_cg"]
    lines.append("ms per CG iteration with the elimination / without: %.2f%s" % (ratio, " (more than twice: see DESIGN.md section 8)" if ratio > 2 else ""))
    lines.append("wall with the elimination / without: %.2f; final costs %.9e / %.9e" % (med[True]["wall"] / med[False]["wall"], runs[True][0]["final"], runs[False][0]["final"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv)
