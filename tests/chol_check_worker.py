"""Subprocess of tests/test_gpu_chol_check.py::test_resident_pairs_plan_backward_error: the automatic plan with RESIDENT PAIRS
(SK_CHAIN_PAIR_MAX_TRAILING=56 in the environment, read once per process, as in tests/pair_plan_worker.py) on one banded_hard
shape (argv[1]), held to the bounds of tests/chol_check.py.  Prints the measured ratios as one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skeres_amd as sk  # noqa: E402
import chol_check as cc  # noqa: E402


def main():
    assert os.environ.get("SK_CHAIN_PAIR_MAX_TRAILING") == "56"
    case = cc.Case(("plan", sys.argv[1]))
    low = np.tril(case.A)
    xs, L = [], None
    for k, (_, b) in enumerate(case.rhs):
        if k == 0:
            x, L = sk.api.cholesky_solve(low, b, want_L=True, last=case.last, group=0, automatic_plan=True)
        else:
            x = sk.api.cholesky_solve(low, b, last=case.last, group=0, automatic_plan=True)
        xs.append(x)
    m = case.measure(L, xs)
    cc.record(case, "device", "automatic-pairs", m)
    print("CHOL_CHECK " + json.dumps(m))


if __name__ == "__main__":
    main()
