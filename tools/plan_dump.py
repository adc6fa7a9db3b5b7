#!/usr/bin/env python3
"""The host plans of DENSE_SCHUR on a fixed list of generated problems, one JSON file per problem: what a change that must not
move a plan is compared on, byte for byte (no device needed).

    python tools/plan_dump.py OUT_DIR

Per problem: borderPlan for auto / on / off, retainedPlan for (auto), (on, 9), (auto, 0, border off), (off), segmentPlan for 2, 3, 4
and 8 segments, forced and not.  Integer arrays as SHA-256, doubles as float.hex()."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import skeres_amd as sk  # noqa: E402
from skeres_amd import bal  # noqa: E402

REVISITS = [(200, 900, 40, 150), (450, 1300, 40, 150), (700, 1600, 40, 150)]  # (tests/test_retained_plan_cpu.py)
PROBLEMS = [
    ("small-16", lambda: bal.generate(16, 600, 2600, seed=11)),
    ("band-400", lambda: bal.generate(400, 30000, 140000, seed=77)),
    ("ladybug", lambda: bal.generate_named("ladybug-1723-156502", seed=1723)),
    ("ladybug-revisits", lambda: bal.generate_named("ladybug-1723-156502", seed=1723, revisits=REVISITS)),
    ("ladybug-long-range", lambda: bal.generate_named("ladybug-1723-156502", seed=1723, long_range_fraction=0.005)),
]


def plain(v):
    if isinstance(v, np.ndarray):
        return "sha256:" + hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    if isinstance(v, float):
        return float(v).hex()
    if isinstance(v, dict):
        return {k: plain(x) for k, x in sorted(v.items())}
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    return v


def to_sk(prob):
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    loss = sk.PredefinedLossFunctions.trivialLoss()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * prob.num_cameras + 3 * prob.point_index.astype(np.int64)], axis=1)
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    return problem, params, loss


def plans(problem):
    out = {}
    for mode in ("auto", "on", "off"):
        out["borderPlan %s" % mode] = plain(problem.borderPlan(mode))
    for args in (("auto",), ("on", 9), ("auto", 0, "off"), ("off",)):
        out["retainedPlan %s" % (args,)] = plain(problem.retainedPlan(*args))
    for n in (2, 3, 4, 8):
        for forced in (True, False):
            out["segmentPlan %d %s" % (n, "forced" if forced else "free")] = plain(problem.segmentPlan(n, forced))
    return out


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    for name, make in PROBLEMS:
        problem, params, loss = to_sk(make())
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(plans(problem), f, indent=1, sort_keys=True)
            f.write("\n")
        print("plan_dump: %s" % name, flush=True)


if __name__ == "__main__":
    main()
