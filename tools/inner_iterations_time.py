#!/usr/bin/env python3
"""CGNR with and without inner iterations, with and without the Schur elimination, on the problem and settings of
tools/cgnr_schur_time.py (developer tool; the record profiles/inner_iterations_time.txt).

usage: inner_iterations_time.py OUT.txt [cameras] [points] [observations] [repeats]

A skeres_amd.bal.generate problem (default 600 cameras, 60 000 points, 300 000 observations; cameras 0 and 1 constant) is solved
by CGNR to its own convergence in one build, one process: the four settings alternating, `repeats` times each after one warm-up
solve of each.  Per run: LM iterations, total CG iterations, inner rounds, ms per round (the wall time spent refining over the
rounds: every batch of rounds ends in a synchronise), wall time of the stepping loop, the final cost and the termination message.
Beside the ms per round stands the yardstick from profiles/cgnr_schur_time.txt: a round is one evaluation with the Jacobian and
one without, which the parent's evaluation and cost phases give per LM iteration.

Without a device the tool fails; no record is written then."""
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402


def solve(prob, schur, inner, max_iterations=50):
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
    o.setUseInnerIterations(inner)
    solver = sk.StepSolver(o, problem)
    summary = sk.Solver.Summary()
    t = time.perf_counter()
    while not solver.step():
        pass
    wall = time.perf_counter() - t
    solver.finish(summary)
    out = dict(wall=wall, iterations=len(summary.iterations()) - 1, initial=summary.initialCost(), final=summary.finalCost(), message=summary.message(),
               phases=[summary.phaseSeconds(k) for k in range(5)])
    for nm in ("cg_iterations", "inner_iteration_steps", "inner_iteration_rounds", "inner_iterations_enabled", "inner_iteration_seconds"):
        out[nm] = solver.stat(nm)
    return out


def parent_yardstick():
    """{elimination: ms of the evaluation and cost phases per LM iteration} from run 0 of each setting in profiles/cgnr_schur_time.txt."""
    out = {}
    try:
        text = open(os.path.join(ROOT, "profiles", "cgnr_schur_time.txt")).read()
    except OSError:
        return out
    for m in re.finditer(r"elimination (on|off)\s*, run 0: (\d+) LM iterations.*?\n.*?evaluation ([0-9.]+),.*?cost ([0-9.]+)\n", text):
        out[m.group(1) == "on"] = (float(m.group(3)) + float(m.group(4))) / int(m.group(2))
    return out


def main(argv):
    path = argv[1]
    C, P, N = (int(argv[k]) if len(argv) > k else d for k, d in ((2, 600), (3, 60000), (4, 300000)))
    repeats = int(argv[5]) if len(argv) > 5 else 3
    if sk.device_count() < 1:
        raise SystemExit("inner_iterations_time needs a HIP device")
    prob = bal.generate(C, P, N, seed=7)
    yard = parent_yardstick()
    settings = [(schur, inner) for schur in (False, True) for inner in (False, True)]
    name = lambda s: "elimination %s, inner iterations %s" % ("on " if s[0] else "off", "on " if s[1] else "off")
    lines = ["CGNR with and without inner iterations (tools/inner_iterations_time.py; one MI355X, JACOBI, eta 0.1, the default tolerances).",
             "bal.generate(%d, %d, %d, seed=7), cameras 0 and 1 constant; one process, the four settings alternating, %d runs each after a warm-up of each."
             % (C, P, N, repeats),
             "Wall: host clock around the stepping loop.  ms per round: the wall time spent refining over the rounds.",
             "Yardstick for a round (one evaluation with the Jacobian and one without): the parent's evaluation + cost phases per LM iteration,",
             "from profiles/cgnr_schur_time.txt: %s." % ", ".join("elimination %s %.3f ms" % ("on" if s else "off", v) for s, v in sorted(yard.items())), ""]
    for s in settings:
        solve(prob, s[0], s[1], 3)
    runs = {s: [] for s in settings}
    for rep in range(repeats):
        for s in settings:
            r = solve(prob, *s)
            runs[s].append(r)
            r["ms_per_round"] = 1e3 * r["inner_iteration_seconds"] / max(r["inner_iteration_rounds"], 1)
            lines += ["%s, run %d: %d LM iterations, %d CG iterations, %d inner rounds over %d refined steps (%s at the end); cost %.6e -> %.9e (%s)"
                      % (name(s), rep, r["iterations"], r["cg_iterations"], r["inner_iteration_rounds"], r["inner_iteration_steps"],
                         "enabled" if r["inner_iterations_enabled"] else "off", r["initial"], r["final"], r["message"]),
                      "  wall %.1f ms; refining %.1f ms, %.3f ms per round%s; device phases (ms): evaluation %.3f, CG loop %.3f"
                      % (1e3 * r["wall"], 1e3 * r["inner_iteration_seconds"], r["ms_per_round"],
                         " (yardstick %.3f)" % yard[s[0]] if s[1] and s[0] in yard else "", 1e3 * r["phases"][0], 1e3 * r["phases"][2])]
    lines += ["", "medians                                   LM iterations   CG iterations   inner rounds   ms per round   wall ms to the final cost   final cost"]
    med = {}
    for s in settings:
        r = runs[s][0]
        med[s] = {f: statistics.median(q[f] for q in runs[s]) for f in ("wall", "ms_per_round")}
        lines.append("%s   %13d   %13d   %12d   %12.3f   %25.1f   %.9e" % (name(s), r["iterations"], r["cg_iterations"], r["inner_iteration_rounds"],
                                                                            med[s]["ms_per_round"], 1e3 * med[s]["wall"], r["final"]))
    for schur in (False, True):
        on, off = (schur, True), (schur, False)
        lines.append("elimination %s: wall with inner iterations / without %.2f; ms per round / yardstick %s"
                     % ("on " if schur else "off", med[on]["wall"] / med[off]["wall"], "%.2f" % (med[on]["ms_per_round"] / yard[schur]) if schur in yard else "n/a"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv)
