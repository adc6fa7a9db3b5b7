#!/usr/bin/env python3
"""Parameter bounds against plain LEVENBERG_MARQUARDT on the Ladybug-1723 shape (developer tool; the records profiles/bounds_*.txt).
usage: bounds_vs_lm.py [runs] [iterations]
Three ways from the benchmark's own start: without bounds; with bounds on every coordinate that never bind; with an upper bound on
every third focal length 1 % below its start, which binds.  Per way: ms per iteration around sk_solver_step (kernel timing off),
then, in runs of their own under kernel timing, the three kernels bounds add on the DENSE_SCHUR path and the bytes they move."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402

NAME, SEED = "ladybug-1723-156502", 1723
# doubles a lane reads and writes per coordinate of the [cameras | points] vector
KERNELS = (("bal_bounded_candidate", 6, "x, step, scale, lo, hi read; x_new written"),
           ("bal_directional_derivative", 3, "gs, step, scale read"),
           ("bounded_grad_max_xnorm", 5, "gs, scale, x, lo, hi read"))


def build(prob, way):
    C, P = prob.num_cameras, prob.num_points
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, sk.PredefinedLossFunctions.trivialLoss(), params, offs)
    x0 = prob.parameters
    if way == "inactive":
        for off, size in [(9 * i, 9) for i in range(C)] + [(9 * C + 3 * q, 3) for q in range(P)]:
            blk = params.slice(off)
            for k in range(size):
                w = 1e7 * (1.0 + abs(x0[off + k]))
                problem.setParameterLowerBound(blk, k, x0[off + k] - w)
                problem.setParameterUpperBound(blk, k, x0[off + k] + w)
    elif way == "active":
        for i in range(2, C, 3):
            problem.setParameterUpperBound(params.slice(9 * i), 6, 0.99 * x0[9 * i + 6])
    return problem, params


def options(iterations):
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
    o.setMaxNumIterations(iterations)
    o.setFunctionTolerance(0.0)
    o.setParameterTolerance(0.0)
    return o


def one_run(prob, way, iterations, timing):
    problem, params = build(prob, way)
    solver = sk.StepSolver(options(iterations), problem)
    solver.step()  # (the first launches of a process carry its one-off costs)
    if timing:
        solver.setKernelTiming(1)
    walls, done = [], False
    while not done:
        t0 = time.perf_counter()
        done = solver.step()
        walls.append(time.perf_counter() - t0)
    kernels = {}
    if timing:
        for name, _, _ in KERNELS:
            s, c = solver.kernelSeconds(name)
            kernels[name] = (s, c)
    stats = {nm: solver.stat(nm) for nm in ("bounded_coordinates", "active_bounds", "line_search_evaluations", "graph_replay")}
    summary = sk.Solver.Summary()
    solver.finish(summary)
    its = summary.iterations()
    return dict(walls=walls[:len(its) - 2], its=its, kernels=kernels, stats=stats, message=summary.message())


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    prob = bal.generate_named(NAME, seed=SEED, perturb=(1e-2, 1e-1, 1e-1))
    n = prob.num_parameters
    print("Parameter bounds against plain LEVENBERG_MARQUARDT on one MI355X, same build, same problem: Ladybug-1723 shape (%d cameras, %d points," % (prob.num_cameras, prob.num_points))
    print("%d observations; %d coordinates, %.2f MB per vector), the benchmark's own start, %d iterations, %d runs of each way." % (prob.num_observations, n, 8e-6 * n, iterations, runs))
    print("Wall times around sk_solver_step from the second iteration on, kernel timing off.")
    for way in ("none", "inactive", "active"):
        for r in range(runs):
            out = one_run(prob, way, iterations, False)
            its = out["its"]
            print("bounds %-8s run %d: %d iterations, %.3f ms per iteration (min %.3f, max %.3f); cost %.6e -> %.6e; alpha %s; evaluations %s; stats %s" % (
                way, r, len(out["walls"]), 1e3 * np.mean(out["walls"]), 1e3 * min(out["walls"]), 1e3 * max(out["walls"]), its[0]["cost"], its[-1]["cost"],
                sorted(set(round(e["step_size"], 6) for e in its[1:])), sorted(set(int(e["line_search_evaluations"]) for e in its[1:])),
                {k: int(v) for k, v in out["stats"].items()}), flush=True)
    print()
    print("Under kernel timing (sk_solver_set_kernel_timing(1): an event pair around every named launch, which serialises the launches):")
    lines = []
    for way in ("inactive", "active"):
        for r in range(runs):
            out = one_run(prob, way, iterations, True)
            parts = []
            for name, doubles, what in KERNELS:
                s, c = out["kernels"][name]
                each = s / max(c, 1)
                parts.append("%s %d launches %.1f us each (%.2f MB: %s; %.0f GB/s)" % (name, c, 1e6 * each, 8e-6 * doubles * n, what, 8e-9 * doubles * n / each if each > 0 else 0.0))
                if r == 0:
                    lines.append("bounds %-8s %-28s %3d launches  %6.1f us each  %5.2f MB moved (%s)  %5.0f GB/s" % (way, name, c, 1e6 * each, 8e-6 * doubles * n, what, 8e-9 * doubles * n / each if each > 0 else 0.0))
            print("bounds %-8s run %d: %s" % (way, r, "; ".join(parts)), flush=True)
    print()
    print("KERNELS")
    for line in lines:
        print(line)


if __name__ == "__main__":
    main()
