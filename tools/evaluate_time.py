#!/usr/bin/env python3
"""Developer tool: time of Problem.evaluate on the Ladybug-1723-shaped problem of bench.py — a record, not a gate.

One call each for cost only, cost + gradient and everything (cost, residuals, gradient, Jacobian): wall time of the call and the
device time of each of its phases from HIP events (sk_evaluate_options_set_launch_timing), after one warm-up call, median of five.
The solver's own phase_seconds_0 (its Jacobian evaluation of iteration 0) is printed beside it for scale.

    python tools/evaluate_time.py [output file]        (profiles/evaluate_time.txt is such a record)"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402

PHASES = ("uploads", "evaluation", "finish", "gradient", "cost", "downloads")
prob = bal.generate_named("ladybug-1723-156502", seed=1723, perturb=(1e-2, 1e-1, 1e-1))
params = sk.RichDoubleArray.fromArray(prob.parameters)
problem = sk.Problem()
offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * prob.num_cameras + 3 * prob.point_index.astype(np.int64)], axis=1)
problem.addResidualBlocks(1, prob.observations, None, params, offs)
options = sk.Problem.EvaluateOptions()
options.setLaunchTiming(True)
num_rows, num_cols, nnz = problem._evaluate_sizes(options)
lines = ["Problem.evaluate, %s: %d rows, %d columns, %d stored entries" % ("ladybug-1723-156502", num_rows, num_cols, nnz),
         "median of 5 calls after one warm-up; milliseconds; the phases are device time between HIP events on the call's stream",
         "%-28s %9s  %s" % ("outputs", "wall", "  ".join("%10s" % p for p in PHASES))]
for label, want in (("cost", (True, False, False, False)), ("cost + gradient", (True, False, True, False)), ("everything", (True, True, True, True))):
    wall, phases = [], []
    for k in range(6):
        t0 = time.perf_counter()
        problem.evaluate(options, *want)
        t1 = time.perf_counter()
        if k:
            wall.append(t1 - t0)
            phases.append(options.launchSeconds())
    med = [statistics.median(p[i] for p in phases) for i in range(len(PHASES))]
    lines.append("%-28s %9.3f  %s" % (label, 1e3 * statistics.median(wall), "  ".join("%10.3f" % (1e3 * m) for m in med)))
o = sk.Solver.Options()
o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
solver = sk.StepSolver(o, problem)
lines.append("for scale: the solver's phase_seconds_0 (Jacobian evaluation, iteration 0): %.3f ms" % (1e3 * solver.stat("phase_seconds_0")))
del solver
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
