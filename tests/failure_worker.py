"""Subprocess of tests/test_gpu_failure.py's case i: the device runs of one case (argv[1]), pickled to argv[2].  A process of its own
because a time-out of the resident chain or of the resident back-substitution clears a process-wide switch (g_bs_resident), which
must not leak into other tests — and would hide what these cases are there to show.

    run     the case stepped to its end (failure_cases.device_run): log, x after every step, the plan's stats, linear_solves
    twin    a second solver on a fresh copy of the problem, started with initial_trust_region_radius = the radius of the first valid
            solve of `run` (exact: the initial radius over a power of two) and as many iterations as `run` had left from there
    zero    per evaluation (Problem.evaluate at x0 and at the final x of `run`) and per named zero column: is every entry of the
            CRS Jacobian's column exactly 0 (and is there an entry at all)
    retained_points   the points the forced retained plan keeps (Problem.retainedPlan), where the case forces one"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skeres_amd as sk  # noqa: E402
import failure_cases as fc  # noqa: E402

STATS = ("graph_replay", "cholesky_columns_resident", "retained_points", "dissected", "border_cameras")


def crs_columns(prob, problem, params, columns):
    """The CRS Jacobian's column of each coordinate in `columns` (indices in x): parameter blocks stand in the problem's own order,
    that of their first mention (camera, then point, of each residual block in turn); checked against Problem.parameterBlockIndex."""
    nc = 9 * prob.num_cameras
    offs = np.stack([9 * prob.camera_index.astype(np.int64), nc + 3 * prob.point_index.astype(np.int64)], axis=1).ravel()
    blocks, first = np.unique(offs, return_index=True)
    blocks = blocks[np.argsort(first, kind="stable")]
    sizes = np.where(blocks < nc, 9, 3)
    start = dict(zip(blocks.tolist(), (np.cumsum(sizes) - sizes).tolist()))
    index = dict(zip(blocks.tolist(), range(len(blocks))))
    out = []
    for j in columns:
        b = j - (j % 9 if j < nc else (j - nc) % 3)
        assert problem.parameterBlockIndex(params.slice(int(b))) == index[b], (j, b)
        out.append(start[b] + j - b)
    return out


def zero_columns(problem, cols):
    m = problem.evaluate(cost=False, residuals=False, gradient=False)["jacobian"]
    return [(int(np.count_nonzero(m.cols == j)), bool(not np.any(m.values[m.cols == j]))) for j in cols]


def main():
    name, path = sys.argv[1], sys.argv[2]
    c = fc.CASES[name]
    prob, comp = fc._prob(c), fc.component(name)
    built = fc.device_problem(name)
    problem, params, n, _ = built
    cols = crs_columns(prob, problem, params, comp["zero_columns"])
    out = dict(zero=[zero_columns(problem, cols)])
    if isinstance(c.get("knobs", {}).get("setRetainedPoints"), tuple):
        mode, npts = c["knobs"]["setRetainedPoints"]
        plan = problem.retainedPlan(mode, npts)
        out["retained_points"] = sorted(set(prob.point_index[plan["retained_of_block"] == 1].tolist()))
    run = fc.device_run(name, STATS + ("linear_solves",), built=built, end_stats=("linear_solves", "cholesky_columns_resident", "graph_replay"))
    out["zero"].append(zero_columns(problem, cols))   # (the parameter memory holds the final x)
    out["run"] = run
    first_valid = next(k for k, e in enumerate(run["log"]) if k and e["step_is_valid"])
    radius = run["log"][first_valid - 1]["trust_region_radius"]
    left = c["options"]["max_num_iterations"] - (first_valid - 1)
    out["twin"] = fc.device_run(name, ("linear_solves",), override=dict(initial_trust_region_radius=radius, max_num_iterations=left),
                                end_stats=("linear_solves",))
    out["first_valid"] = first_valid
    for r in (out["run"], out["twin"]):
        r.pop("report")
    with open(path, "wb") as f:
        pickle.dump(out, f)
    print("FAILURE_WORKER_OK", name, flush=True)


if __name__ == "__main__":
    main()
