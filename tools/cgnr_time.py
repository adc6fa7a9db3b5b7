#!/usr/bin/env python3
"""CGNR on a synthetic sparse problem (developer tool; the record profiles/cgnr_time.txt).  Device functors only.

usage: cgnr_time.py OUT.txt [blocks] [residual blocks on the shared block]

  1. a chain of `blocks` (default 100 000) blocks of size 2 with one shared block (skeres_amd/examples/chain_smoothing.py): ms per LM
     iteration, ms per CG iteration, and the rate the CG loop sustains against the 16 bytes per stored entry that its two products
     must read (the values array once each; the loop's whole time is charged to them, so this is a lower bound of the products'
     own rate), for the batch size in force (SK_CGNR_BATCH);
  2. the same chain at n = 3000, small enough for DENSE_NORMAL_CHOLESKY: wall time of both solvers to their final cost.

Without a device the tool fails; the record then says that no run happened."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd.examples import chain_smoothing as cs  # noqa: E402


def solve(num_blocks, hub_blocks, solver_type, max_iterations=50):
    x0, c, offsets = cs.chain_problem(num_blocks, hub_blocks)
    problem, params = cs.build(x0, c, offsets)
    o = sk.Solver.Options()
    o.setLinearSolverType(solver_type)
    o.setMaxNumIterations(max_iterations)
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
               message=summary.message(), phases=[summary.phaseSeconds(k) for k in range(5)], n=len(x0), residual_blocks=len(c))
    if solver_type == sk.LinearSolverType.CGNR:
        for nm in ("cg_iterations", "cg_batches", "jacobian_nonzeros", "linear_solves"):
            out[nm] = solver.stat(nm)
    return out


def main(argv):
    path = argv[1]
    num_blocks = int(argv[2]) if len(argv) > 2 else 100000
    hub_blocks = int(argv[3]) if len(argv) > 3 else 2000
    if sk.device_count() < 1:
        raise SystemExit("cgnr_time needs a HIP device")
    lines = []
    solve(2000, 100, sk.LinearSolverType.CGNR, 3)   # warm-up: code objects, the first launches
    for run in range(2):
        r = solve(num_blocks, hub_blocks, sk.LinearSolverType.CGNR)
        nnz, cg = r["jacobian_nonzeros"], r["cg_iterations"]
        lines += ["chain: %d blocks of size 2 (n = %d), %d residual blocks, %d on the shared block, %d stored entries; run %d"
                  % (num_blocks, r["n"], r["residual_blocks"], hub_blocks, nnz, run),
                  "  %d LM iterations, %d linear solves, %d CG iterations in %d batches (batch size %s)"
                  % (r["iterations"], r["linear_solves"], cg, r["cg_batches"], os.environ.get("SK_CGNR_BATCH", "8, the default")),
                  "  cost %.6e -> %.6e (%s)" % (r["initial"], r["final"], r["message"]),
                  "  set-up %.1f ms; %.3f ms per LM iteration (wall, %.1f ms in all)" % (1e3 * r["setup"], 1e3 * r["wall"] / max(r["iterations"], 1), 1e3 * r["wall"]),
                  "  device phases (ms): evaluation %.3f, block sums + preconditioner %.3f, CG loop %.3f, model + candidate %.3f, cost %.3f"
                  % tuple(1e3 * p for p in r["phases"]),
                  "  %.4f ms per CG iteration; 16 bytes x %d entries per iteration over the CG loop's time: %.1f GB/s"
                  % (1e3 * r["phases"][2] / max(cg, 1), nnz, 16.0 * nnz * cg / max(r["phases"][2], 1e-12) / 1e9)]
    small = 1500
    a = solve(small, 100, sk.LinearSolverType.CGNR)
    b = solve(small, 100, sk.LinearSolverType.DENSE_NORMAL_CHOLESKY)
    lines += ["chain at n = %d (%d residual blocks), both solvers to their own convergence:" % (a["n"], a["residual_blocks"]),
              "  CGNR                   %3d iterations, %8.1f ms wall, final cost %.9e (%s)" % (a["iterations"], 1e3 * a["wall"], a["final"], a["message"]),
              "  DENSE_NORMAL_CHOLESKY  %3d iterations, %8.1f ms wall, final cost %.9e (%s)" % (b["iterations"], 1e3 * b["wall"], b["final"], b["message"])]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv)
