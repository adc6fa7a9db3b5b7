#!/usr/bin/env python3
"""DOGLEG against LEVENBERG_MARQUARDT on the Ladybug-1723 shape (developer tool; the records profiles/dogleg_*.txt).
usage: dogleg_vs_lm.py compare [runs] [max iterations]   per-iteration wall and phase times of both strategies from a hard start
       dogleg_vs_lm.py products [runs] [iterations]      bal_dogleg_products_kernel and its neighbours under kernel timing"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402

NAME, SEED = "ladybug-1723-156502", 1723
HARD_START = (0.03, 0.3, 0.5)
PLANE_BYTES = 208  # F (18), E (6) and r (2) doubles per observation


def build(prob, const_cams=()):
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * prob.num_cameras + 3 * prob.point_index.astype(np.int64)], axis=1)
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, sk.PredefinedLossFunctions.trivialLoss(), params, offs)
    for i in const_cams:
        problem.setParameterBlockConstant(params.slice(9 * i))
    return problem, params


def options(dogleg, max_iterations):
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
    o.setMaxNumIterations(max_iterations)
    if dogleg:
        o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    return o


def one_run(prob, dogleg, max_iterations):
    """Steps one solver to its end: per iteration the wall time around the step, the phase seconds it added and the two counters."""
    problem, params = build(prob, const_cams=(0, 1))
    solver = sk.StepSolver(options(dogleg, max_iterations), problem)
    rows, done = [], False
    phases = [solver.stat("phase_seconds_%d" % i) for i in range(5)]
    t_loop = time.perf_counter()
    while not done:
        t0 = time.perf_counter()
        done = solver.step()
        wall = time.perf_counter() - t0
        now = [solver.stat("phase_seconds_%d" % i) for i in range(5)]
        rows.append(dict(wall=wall, phases=[b - a for a, b in zip(phases, now)], linear_solves=int(solver.stat("linear_solves")),
                         reused=int(solver.stat("dogleg_reused_steps"))))
        phases = now
    loop = time.perf_counter() - t_loop
    summary = sk.Solver.Summary()
    solver.finish(summary)
    its = summary.iterations()
    rows = rows[:len(its) - 1]  # (a step that only found the solve ended adds no iteration)
    for row, it in zip(rows, its[1:]):
        row.update(it)
    return dict(rows=rows, loop=loop, initial=its[0]["cost"], final=its[-1]["cost"], message=summary.message())


def ms(values):
    return "[" + ", ".join("%.3f" % (1e3 * v) for v in values) + "]"


def span(values):
    return "%.3f-%.3f ms" % (1e3 * min(values), 1e3 * max(values)) if values else "none"


def compare(runs, max_iterations):
    prob = bal.generate_named(NAME, seed=SEED, perturb=HARD_START)
    out = {True: [], False: []}
    for _ in range(runs):
        for dogleg in (True, False):
            out[dogleg].append(one_run(prob, dogleg, max_iterations))
    label = {True: "DOGLEG", False: "LM"}
    print("DOGLEG against LEVENBERG_MARQUARDT on one MI355X, same build, same problem; wall times around sk_solver_step, phases from the solver's events.")
    print("%d runs of each strategy: the stepping loops took %s ms (DOGLEG) and %s ms (LM)." % (
        runs, " / ".join("%.1f" % (1e3 * r["loop"]) for r in out[True]), " / ".join("%.1f" % (1e3 * r["loop"]) for r in out[False])))
    print("Ladybug-1723 shape, start perturbed by %s; cameras 0 and 1 constant; default tolerances, at most %d iterations" % (HARD_START, max_iterations))
    print()
    target = max(out[True][0]["final"], out[False][0]["final"])
    for dogleg in (True, False):
        r = out[dogleg][0]
        elapsed = 0.0
        for k, row in enumerate(r["rows"], 1):
            elapsed += row["wall"]
            if row["cost"] <= target:
                print("%s reaches cost <= %.6e (the larger of the two final costs) at iteration %d, after %.1f ms of stepping (cost there %.6e)" % (
                    label[dogleg], target, k, 1e3 * elapsed, row["cost"]))
                break
    for dogleg in (True, False):
        for n, r in enumerate(out[dogleg]):
            rows = r["rows"]
            rejected = [row for row in rows if not row["step_is_successful"]]
            prev = [0] + [row["reused"] for row in rows[:-1]]
            for row, p in zip(rows, prev):
                row["re"] = row["reused"] > p
            reinterpolated = [row for row in rows if row["re"]]
            print("%s run %d: %d iterations, %.1f ms in the stepping loop, cost %.6e -> %.6e (%s)" % (
                label[dogleg], n, len(rows), 1e3 * r["loop"], r["initial"], r["final"], r["message"]))
            if n == 0:
                for k, row in enumerate(rows, 1):
                    print("  it %2d %s wall %7.3f ms  phases(jac, assembly, cholesky, backsub, cost) %s  linear_solves %d reused %d  cost %.6e rho %.3g radius %.3g" % (
                        k, "accepted" if row["step_is_successful"] else "REJECTED", 1e3 * row["wall"], " ".join("%6.3f" % (1e3 * p) for p in row["phases"]),
                        row["linear_solves"], row["reused"], row["cost"], row["relative_decrease"], row["trust_region_radius"]))
            rej_re = [row["wall"] for row in rejected if row["re"]]
            rej_solved = [row["wall"] for row in rejected if not row["re"]]
            acc_re = [row["wall"] for row in reinterpolated if row["step_is_successful"]]
            print("  %s run %d: %d rejected after a factorisation of their own, %s; %d rejected re-interpolated, %s; %d accepted re-interpolated (with the Jacobian evaluation that follows), %s" % (
                label[dogleg], n, len(rej_solved), span(rej_solved), len(rej_re), span(rej_re), len(acc_re), span(acc_re)))
            print("  %s run %d: rejected iterations wall ms %s" % (label[dogleg], n, ms(row["wall"] for row in rejected)))
            print("  %s run %d: re-interpolated iterations wall ms %s" % (label[dogleg], n, ms(row["wall"] for row in reinterpolated)))


def products(runs, iterations):
    prob = bal.generate_named(NAME, seed=SEED, perturb=(1e-2, 1e-1, 1e-1))
    print("bal_dogleg_products_kernel and its neighbours on one MI355X (sk_solver_set_kernel_timing(1): an event pair around every named launch,")
    print("which serialises the launches), DOGLEG from the benchmark's own start, %d iterations, %d runs." % (iterations, runs))
    print("Ladybug-1723 shape: %d cameras, %d points, %d observations; %.1f MB of planes per launch at %d B per observation" % (
        prob.num_cameras, prob.num_points, prob.num_observations, 1e-6 * PLANE_BYTES * prob.num_observations, PLANE_BYTES))
    for n in range(runs):
        problem, params = build(prob)
        solver = sk.StepSolver(options(True, iterations), problem)
        solver.step()  # (the first launches of a process carry its one-off costs)
        solver.setKernelTiming(1)
        while not solver.step():
            pass
        seconds, launches = solver.kernelSeconds("bal_dogleg_products")
        each = seconds / launches
        others = []
        for name in ("dogleg_vector_norms", "bal_dogleg_combine", "bal_eval_cost"):
            s, c = solver.kernelSeconds(name)
            others.append("%s %.1f us" % (name, 1e6 * s / c))
        print("run %d: bal_dogleg_products %d launches, %.1f us each, %.0f GB/s at %d B/observation; %s" % (
            n, launches, 1e6 * each, 1e-9 * PLANE_BYTES * prob.num_observations / each, PLANE_BYTES, "; ".join(others)), flush=True)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "compare"
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if mode == "products":
        products(runs, int(sys.argv[3]) if len(sys.argv) > 3 else 6)
    else:
        compare(runs, int(sys.argv[3]) if len(sys.argv) > 3 else 50)


if __name__ == "__main__":
    main()
