"""The device's Cholesky plans against the backward-error bounds of tests/chol_check.py, on systems whose 128 x 128 diagonal
blocks are ill-conditioned: factor_ratio <= 1 wherever an entry point returns its factor, solve_row_ratio <= 1 everywhere, for b
random and for b = A s with s = +-1.  Both are formed in extended precision from the matrix alone: no other double-precision
factor or solution is compared with.  The same matrices pass through LAPACK and the explicit-inverse emulation in
tests/test_chol_check_cpu.py, which also establishes the kappa_b each shape carries (chol_check.KAPPA_B).

With CHOL_CHECK_LOG set, every measured plan appends one JSON line there (profiles/chol_backward_error.txt)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import skeres_amd as sk
import chol_check as cc

pytestmark = pytest.mark.gpu

EXPLICIT_1 = {"group": 1, "automatic_plan": False}
EXPLICIT_2 = {"group": 2, "automatic_plan": False}
EXPLICIT_4 = {"group": 4, "automatic_plan": False}
AUTOMATIC = {"group": 0, "automatic_plan": True}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


@functools.lru_cache(maxsize=1)
def _case(cid):
    return cc.Case(cid)


def _plan_name(kw):
    return "automatic" if kw["automatic_plan"] else "group-%d" % kw["group"]


def _check(case, kw, solve, want_L=True, label=None):
    """solve(b, want_L) -> x or (x, L).  Measures, records, asserts."""
    xs, L = [], None
    for k, (_, b) in enumerate(case.rhs):
        got = solve(b, want_L and k == 0)
        if want_L and k == 0:
            got, L = got
        xs.append(got)
    m = case.measure(L, xs)
    cc.record(case, "device", label or _plan_name(kw), m)
    print(case.name, label or _plan_name(kw), m)
    if want_L:
        assert m["factor_ratio"] <= 1.0, (case.name, kw, m)
    assert max(m["solve_row_ratio"]) <= 1.0, (case.name, kw, m)


@pytest.mark.parametrize("cid", cc.DENSE_CASES, ids=cc.case_id)
def test_dense_factorisation_backward_error(cid):
    """graded (kappa 1e4, 1e8, 1e12) and hard_blocks at one block, one block plus a row, two blocks plus a row and six blocks
    with a partial last one; explicit groups of 1, 2 and 4 and the automatic plan."""
    case = _case(cid)
    for kw in (EXPLICIT_1, EXPLICIT_2, EXPLICIT_4, AUTOMATIC):
        _check(case, kw, lambda b, want: sk.api.cholesky_solve(case.A, b, want_L=want, **kw))


@pytest.mark.parametrize("kw", [EXPLICIT_1, EXPLICIT_2, AUTOMATIC], ids=_plan_name)
@pytest.mark.parametrize("cid", cc.PLAN_CASES, ids=cc.case_id)
def test_factorisation_plans_backward_error(cid, kw):
    """banded_hard on the envelopes of test_gpu_parity._PLAN_SHAPES (every regime of cholesky_plan and every hand-over), cut 70
    rows off the block grid: explicit groups of one and two, and the automatic plan with the resident chain (with resident pairs:
    test_resident_pairs_plan_backward_error)."""
    case = _case(cid)
    low = np.tril(case.A)
    _check(case, kw, lambda b, want: sk.api.cholesky_solve(low, b, want_L=want, last=case.last, **kw))


@pytest.mark.parametrize("cid", cc.PLAN_CASES, ids=cc.case_id)
def test_resident_pairs_plan_backward_error(cid):
    """The same four shapes under the automatic plan with resident PAIRS of block columns (one K = 256 SYRK per pair under the
    potrf server): the knob SK_CHAIN_PAIR_MAX_TRAILING is read once per process, so tests/chol_check_worker.py runs it."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chol_check_worker.py")
    out = subprocess.run([sys.executable, worker, cid[1]], env=dict(os.environ, SK_CHAIN_PAIR_MAX_TRAILING="56"), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CHOL_CHECK ")][-1][len("CHOL_CHECK "):])
    print(cc.case_id(cid), "automatic-pairs", m)
    assert m["factor_ratio"] <= 1.0, m
    assert max(m["solve_row_ratio"]) <= 1.0, m


@pytest.mark.parametrize("kw", [EXPLICIT_2, AUTOMATIC], ids=_plan_name)
@pytest.mark.parametrize("cid", cc.BORDERED_CASES, ids=cc.case_id)
def test_bordered_factorisation_backward_error(cid, kw):
    """bordered_hard: a border narrower than a block, a border reached by the very first block column, three revisits."""
    case = _case(cid)
    low = np.tril(case.A)
    _check(case, kw, lambda b, want: sk.api.cholesky_solve_bordered(low, b, case.border_begin, want_L=want, **kw))


def _reach(low, begin):
    """The last row coupled with anything before `begin`."""
    return int(np.max(np.nonzero(np.any(low[:, :begin] != 0, axis=1))[0]))


@pytest.mark.parametrize("shape,head_block", [("band", 17), ("two-wide-parts", 29)])
def test_dissected_solve_backward_error(shape, head_block):
    """Two-way dissection with the cuts of test_dissected_factorisation_vs_numpy: no factor comes back, the solve metric applies
    as it stands (it does not depend on the elimination order)."""
    case = _case(("plan", shape))
    low = np.tril(case.A)
    head = 128 * head_block - 37
    first_tail = max(head, _reach(low, head) + 1)
    for tail_begin in sorted({first_tail, min(case.n, first_tail + 200), case.n}):
        for kw in (AUTOMATIC, EXPLICIT_2):
            _check(case, kw, lambda b, want: sk.api.cholesky_solve_dissected(low, b, head, tail_begin, **kw), want_L=False,
                   label="dissected-%d-%d-%s" % (head, tail_begin, _plan_name(kw)))


@pytest.mark.parametrize("shape,starts", [("band", (9, 19, 30)), ("two-wide-parts", (4, 30, 58))])
def test_segmented_solve_backward_error(shape, starts):
    """Multi-way dissection with the cuts of test_multiway_dissected_factorisation_vs_numpy."""
    case = _case(("plan", shape))
    low = np.tril(case.A)
    cuts, prev_end = [], 0
    for k, blk in enumerate(starts):
        begin = max(prev_end + 50, 128 * blk - 37 - 11 * k)
        end = max(begin, _reach(low, begin) + 1)
        cuts.append((begin, end))
        prev_end = end
    assert prev_end < case.n - 50
    for kw in (AUTOMATIC, EXPLICIT_2):
        _check(case, kw, lambda b, want: sk.api.cholesky_solve_segments(low, b, cuts, **kw), want_L=False,
               label="segments-%d-%s" % (len(cuts) + 1, _plan_name(kw)))


@pytest.mark.parametrize("starts", [(700, 1500, 2600), (400, 900, 1400, 1900, 2400, 2900, 3400)], ids=["three-separators", "seven-separators"])
def test_segmented_scalar_band_backward_error(starts):
    """The scalar band of 40 with separators of 40 rows, three and seven of them."""
    case = _case(cc.SCALAR_BAND_CASE)
    low = np.tril(case.A)
    cuts = [(a, a + 40) for a in starts]
    for kw in (AUTOMATIC, EXPLICIT_2):
        _check(case, kw, lambda b, want: sk.api.cholesky_solve_segments(low, b, cuts, **kw), want_L=False,
               label="segments-%d-%s" % (len(cuts) + 1, _plan_name(kw)))


def _solve_case(case, A, b, kw):
    if case.border_begin is not None:
        return sk.api.cholesky_solve_bordered(np.tril(A), b, case.border_begin, **kw)
    return sk.api.cholesky_solve(A, b, **kw)


@pytest.mark.parametrize("cid,block", cc.NPD_CASES, ids=lambda v: cc.case_id(v) if isinstance(v, tuple) else str(v))
def test_a_matrix_that_is_not_positive_definite_is_reported(cid, block):
    """A - (mu + 1e-6) v v^T restored to a unit diagonal (chol_check.indefinite_in_block): one eigenvalue of -1e-6 that the
    factorisation meets in the first block, a middle block, the last partial block, the border of a bordered system.  Every
    diagonal entry is 1, so nothing shows before the factorisation.  Explicit groups only; the untouched matrix factors."""
    case = _case(cid)
    bad = cc.indefinite_in_block(case.A, np.linalg.cholesky(case.A), block)
    assert np.all(np.diag(bad) == 1.0)
    b = case.rhs[0][1]
    for kw in (EXPLICIT_1, EXPLICIT_2):
        x = _solve_case(case, case.A, b, kw)
        assert cc.solve_row_ratio(case.A, x, b, case.m) <= 1.0
        with pytest.raises(sk.SkeresError):
            _solve_case(case, bad, b, kw)


def test_a_nan_below_the_diagonal_is_reported():
    cid, (i, j) = cc.NAN_CASE
    case = _case(cid)
    bad = case.A.copy()
    bad[i, j] = bad[j, i] = np.nan
    b = case.rhs[0][1]
    for kw in (EXPLICIT_1, EXPLICIT_2):
        x = sk.api.cholesky_solve(case.A, b, **kw)
        assert cc.solve_row_ratio(case.A, x, b, case.m) <= 1.0
        with pytest.raises(sk.SkeresError):
            sk.api.cholesky_solve(bad, b, **kw)


FAILURE_COMBINATIONS = ([("automatic",) + cid for cid in cc.PLAN_CASES + cc.BORDERED_CASES] + [("pairs",) + cid for cid in cc.PLAN_CASES]
                        + [(plan, "plan", shape) for plan in ("dissected", "segments") for shape in ("band", "two-wide-parts")])


@pytest.mark.parametrize("plan,kind,shape", FAILURE_COMBINATIONS, ids=lambda v: str(v))
def test_a_failed_factorisation_and_the_solve_after_it(plan, kind, shape):
    """The automatic plan (resident panel chain, resident back-substitution), resident pairs, the two-way and the multi-way dissection
    on the shapes their backward-error tests use: the good matrix, then a matrix with one negative eigenvalue in a middle block, then
    the good matrix again; then one with a NaN below the diagonal, then the good matrix again (tests/chol_failure_worker.py, a
    process per combination).  Both bad matrices must be reported as not positive definite — not as a time-out of the chain, which is
    what a waiter that the failed block column did not release would end in — and the good matrix must give the same bits each time."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chol_failure_worker.py")
    env = dict(os.environ, SK_CHAIN_PAIR_MAX_TRAILING="56") if plan == "pairs" else {k: v for k, v in os.environ.items() if k != "SK_CHAIN_PAIR_MAX_TRAILING"}
    out = subprocess.run([sys.executable, worker, plan, kind, shape], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CHOL_FAILURE ")][-1][len("CHOL_FAILURE "):])
    print(got)
    assert "timed out" not in out.stderr, out.stderr[-2000:]
    for message in got["messages"]:
        assert message is not None and "not positive definite" in message and "timed out" not in message, got
