"""Subprocess of tests/test_gpu_chol_check.py::test_a_failed_factorisation_and_the_solve_after_it: one plan (argv[1]) on one case of
tests/chol_check.py (argv[2], argv[3]), in a process of its own because a time-out of the resident chain switches it off for the rest of the process (and the
pairs plan reads SK_CHAIN_PAIR_MAX_TRAILING once per process).

    the good matrix is solved; the matrix with one negative eigenvalue met in a middle block (chol_check.indefinite_in_block) must
    raise "not positive definite"; the good matrix again gives the same bits; the matrix with a NaN below the diagonal of that block
    must raise the same; the good matrix again gives the same bits.

A pivot that is not positive, or NaN, is a status and not a stop: every workgroup that waits on the failed block column is released
by its counters.  A waiter left to its time-out would raise "the resident panel chain timed out" instead (and take a second): the
message tells the two apart.  Prints the wall time of every call as one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skeres_amd as sk  # noqa: E402
import chol_check as cc  # noqa: E402

AUTOMATIC = {"group": 0, "automatic_plan": True}
DISSECTED_HEAD_BLOCK = {"band": 17, "two-wide-parts": 29}                 # as test_dissected_solve_backward_error
SEGMENT_STARTS = {"band": (9, 19, 30), "two-wide-parts": (4, 30, 58)}     # as test_segmented_solve_backward_error


def _reach(low, begin):
    return int(np.max(np.nonzero(np.any(low[:, :begin] != 0, axis=1))[0]))


def solver(plan, case):
    """solve(A, b) of the plan on the case's envelope, and the 128-block the defects go into."""
    low = np.tril(case.A)
    nblk = (case.n + 127) // 128
    if plan in ("automatic", "pairs"):
        if case.border_begin is not None:
            return (lambda A, b: sk.api.cholesky_solve_bordered(np.tril(A), b, case.border_begin, **AUTOMATIC)), nblk // 2
        return (lambda A, b: sk.api.cholesky_solve(np.tril(A), b, last=case.last, **AUTOMATIC)), nblk // 2
    if plan == "dissected":
        head = 128 * DISSECTED_HEAD_BLOCK[case.cid[1]] - 37
        tail_begin = max(head, _reach(low, head) + 1)
        return (lambda A, b: sk.api.cholesky_solve_dissected(np.tril(A), b, head, tail_begin, **AUTOMATIC)), DISSECTED_HEAD_BLOCK[case.cid[1]] // 2
    cuts, prev_end = [], 0
    for k, blk in enumerate(SEGMENT_STARTS[case.cid[1]]):
        begin = max(prev_end + 50, 128 * blk - 37 - 11 * k)
        end = max(begin, _reach(low, begin) + 1)
        cuts.append((begin, end))
        prev_end = end
    return (lambda A, b: sk.api.cholesky_solve_segments(np.tril(A), b, cuts, **AUTOMATIC)), (SEGMENT_STARTS[case.cid[1]][0] + SEGMENT_STARTS[case.cid[1]][1]) // 2


def main():
    plan, kind, shape = sys.argv[1], sys.argv[2], sys.argv[3]
    assert (os.environ.get("SK_CHAIN_PAIR_MAX_TRAILING") == "56") == (plan == "pairs")
    case = cc.Case((kind, shape))
    solve, block = solver(plan, case)
    b = case.rhs[0][1]
    indefinite = cc.indefinite_in_block(case.A, np.linalg.cholesky(case.A), block)
    assert np.all(np.diag(indefinite) == 1.0) and np.array_equal(indefinite != 0, case.A != 0)
    with_nan = case.A.copy()
    i = 128 * block + 70
    assert with_nan[i, i - 3] != 0
    with_nan[i, i - 3] = with_nan[i - 3, i] = np.nan
    seconds, messages = [], []

    def timed(A):
        t0 = time.perf_counter()
        try:
            return solve(A, b)
        finally:
            seconds.append(time.perf_counter() - t0)

    timed(case.A)   # (the first call of a process pays for the context and the chain's trial run)
    x = timed(case.A)
    assert cc.solve_row_ratio(case.A, x, b, case.m) <= 1.0
    for bad in (indefinite, with_nan):
        try:
            timed(bad)
            messages.append(None)
        except sk.SkeresError as e:
            messages.append(str(e))
        again = timed(case.A)
        assert np.array_equal(again.view(np.uint64), x.view(np.uint64)), "the solve after a failed factorisation differs"
    print("CHOL_FAILURE " + json.dumps({"plan": plan, "shape": shape, "block": block, "messages": messages, "seconds": seconds}))


if __name__ == "__main__":
    main()
