"""tests/chol_check.py on the CPU: its extended-precision product is right, every matrix tests/test_gpu_chol_check.py uses is
factored by LAPACK with cond(A) <= 1e13 (and carries the largest kappa_b that allows it), LAPACK and the explicit-inverse
emulation stay below both bounds on every one of them (calibration), planted defects of the emulation land above 100 by the
factor metric and by the solve metric, the sampled form on the largest shape included (teeth), and the inputs that are not
positive definite are rejected by LAPACK while their neighbours are accepted.

With CHOL_CHECK_LOG set, every measured case appends one JSON line there (profiles/chol_backward_error.txt)."""
import functools

import numpy as np
import pytest

import chol_check as cc

LD = np.longdouble


def test_long_double_is_extended():
    assert np.finfo(LD).nmant >= 63


def test_exact_product_against_a_plain_long_double_product():
    """_exact_nt against products and sums in long double: entries over twelve decades, cancellation to 1e-13 of the terms."""
    rng = np.random.default_rng(1)
    X = rng.normal(size=(70, 1500)) * 10.0 ** rng.uniform(-12, -0.5, (70, 1500))
    Y = rng.normal(size=(50, 1500)) * 10.0 ** rng.uniform(-12, -0.5, (50, 1500))
    Y[:, 750:] = -Y[:, :750] * (1 + 1e-13 * rng.normal(size=(50, 750)))
    X[:, 750:] = X[:, :750]
    ref = X.astype(LD) @ Y.astype(LD).T
    mag = np.abs(X).astype(LD) @ np.abs(Y).astype(LD).T
    got, left = cc._exact_nt(X, Y)
    assert np.max(np.abs(got - ref) / mag) <= 1500 * 2.0 ** -63
    assert np.all(left <= 1e-28)
    # a row that is tiny throughout keeps its relative accuracy: the scaling is per row and chunk
    got, left = cc._exact_nt(X * 2.0 ** -200, Y)
    assert np.max(np.abs(got - ref * LD(2.0) ** -200) / (mag * LD(2.0) ** -200)) <= 1500 * 2.0 ** -63
    assert np.all(left <= 1e-28 * 2.0 ** -200)
    for S in cc._slices(X)[:-1]:
        assert np.all(S == np.rint(S * 2.0 ** 100) / 2.0 ** 100)
    assert np.array_equal(functools.reduce(np.add, cc._slices(X)[::-1]), X)


def test_factor_ratio_of_an_exact_factor_and_of_one_wrong_entry():
    """Integer factor, exact product: ratio 0.  One entry of L moved by 1e-9: the dense and the sampled form both see it, where it is."""
    n = 300
    L0 = np.tril(((np.arange(n)[:, None] * 7 + np.arange(n)[None, :] * 3) % 5 - 2).astype(float)) / 64.0
    L0[np.arange(n), np.arange(n)] = 0.5
    A = L0 @ L0.T
    assert cc.factor_ratio(A, L0) == 0.0
    L1 = L0.copy()
    L1[170, 140] += 1e-9
    for sampled in (False, True):
        r, where = cc.factor_ratio(A, L1, sampled=sampled, where=True)
        assert r > 1e3 and where[0] // 128 == 1 and where[1] // 128 == 1, (sampled, r, where)
    L1 = L0.copy()
    L1[10, 200] = 1e-300                   # above the diagonal: not a factor
    assert cc.factor_ratio(A, L1) == float("inf")


def test_m_ij_counts_the_blocked_dot_product():
    fb = np.array([0, 0, 1, 1, 4])
    g, valid = cc._entry_bound(np.array([0, 300, 300, 400, 600]), np.array([0, 100, 290, 130, 520]), fb)
    assert list(valid) == [True, False, True, True, True]
    m = [128 + 129, None, 2 * 128 + 129, 128 + 129, 128 + 129]
    for k in (0, 2, 3, 4):
        assert g[k] == cc.gamma(m[k])
    assert cc.max_m(fb, 640) == 3 * 128 + 129
    assert cc.regime_rows([7] * 8 + [40 - i for i in range(30)] + [9] * 24) == [7, 8, 23, 24, 37, 38]
    assert cc.regime_rows([6] * 40) == []
    # a border row that reaches back to block 0 against a band row that starts at block 4: the columns of BOTH envelopes
    fb = np.array([0, 0, 1, 2, 3, 4, 0])
    g, valid = cc._entry_bound(np.array([800, 800]), np.array([700, 100]), fb)
    assert list(valid) == [True, True] and g[0] == cc.gamma(2 * 128 + 129) and g[1] == cc.gamma(128 + 129)
    assert cc.max_m(fb, 896) == 7 * 128 + 129


@functools.lru_cache(maxsize=1)
def _case(cid):
    return cc.Case(cid)


@functools.lru_cache(maxsize=1)
def _lapack(cid):
    return cc.Lapack(_case(cid).A)


ALL_CASES = cc.DENSE_CASES + cc.PLAN_CASES + cc.BORDERED_CASES + [cc.SCALAR_BAND_CASE]


def _next_kappa(kb):
    k = cc.KAPPAS.index(kb)
    return cc.KAPPAS[k + 1] if k + 1 < len(cc.KAPPAS) else None


@pytest.mark.parametrize("cid", ALL_CASES, ids=cc.case_id)
def test_lapack_and_the_emulation_stay_below_both_bounds(cid):
    """Calibration.  LAPACK factors the matrix, cond(A) <= 1e13, and for LAPACK and for blocked_explicit_inverse factor_ratio <= 1
    and solve_row_ratio <= 1 for b random and b = A s, s = +-1."""
    case = _case(cid)
    A = case.A
    assert np.array_equal(A, A.T) and np.all(np.diag(A) == 1.0)
    lap = _lapack(cid)
    assert cc.cond_estimate(A, lap.L) <= cc.COND_MAX
    emu = cc.blocked_explicit_inverse(A, case.envelope)
    for who, f in (("lapack", lap), ("emulation", emu)):
        got = case.measure(f.L, [f.solve(b) for _, b in case.rhs])
        cc.record(case, who, None, got)
        assert got["factor_ratio"] <= 1.0, (who, got)
        assert max(got["solve_row_ratio"]) <= 1.0, (who, got)


HARD_CASES = [c for c in ALL_CASES if c[0] != "graded"]


@pytest.mark.parametrize("cid", HARD_CASES, ids=cc.case_id)
def test_kappa_b_is_the_largest_the_shape_carries(cid):
    """chol_check.KAPPA_B holds, per shape, the largest of KAPPAS at which LAPACK factors the matrix with cond(A) <= 1e13 (that it
    does there: the calibration above): at the next one LAPACK fails or cond(A) > 1e13."""
    key = {"plan": "banded_hard", "bordered": "bordered_hard"}.get(cid[0], cid[0])
    harder = _next_kappa(cc.KAPPA_B[(key, cid[1])])
    if harder is None:
        return
    A = cc.case_matrix(cid, harder)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return
    assert cc.cond_estimate(A, L) > cc.COND_MAX


def _defects(case, lap):
    """The planted defects, placed from the envelope: c is the block column at the plan's first change of regime (the middle of a
    dense matrix), the single wrong entry sits in a diagonal block (which the sampled form reads whole) and leaves out the largest
    term of its dot product."""
    fb = case.envelope
    c = case.rows[1] if case.rows else len(fb) // 2
    assert fb[c + 1] <= c - 2 and fb[c] <= c - 2
    i, j = 128 * c + 77, 128 * c + 13
    k0, k1 = 128 * int(fb[c]), 128 * c
    k = k0 + int(np.argmax(np.abs(lap.L[i, k0:k1] * lap.L[j, k0:k1])))
    return [("skip_tile", c - 2, 128 * (c + 1) + 40, 128 * c + 70), ("skip_panel", c - 2, c), ("float32_L",), ("float32_inv", c - 1),
            ("drop_term", i, j, k), ("transpose_tile", c - 1, 128 * (c + 1))]


@pytest.mark.parametrize("cid", [("hard_blocks", 700, 1.0), cc.LARGEST_CASE + (1.0,)], ids=cc.case_id)
def test_planted_defects_are_flagged(cid):
    """Teeth: each defect of blocked_explicit_inverse gives factor_ratio > 100 and solve_row_ratio > 100 (both right-hand sides)
    on hard_blocks(700), dense, and factor_ratio > 100 in the sampled form on the largest shape of the GPU tests.  (Both with
    kappa_b = 1: at the kappa_b they carry, a skipped update leaves a diagonal block indefinite and there is no factor to measure.)

    Measured: factor_ratio 7e5 .. 3e13 (the float32 roundings 7e5 .. 3e6); solve_row_ratio on hard_blocks(700) 140 .. 1e9.  On the
    largest shape (n = 8250, m = 5377) the solve metric, loose by the envelope width, gives 6e4 .. 2e7 for the four structural
    defects, which is asserted, but only 4 .. 5 for L rounded to float32 and 9 .. 26 for one inverse block rounded to float32:
    above the bound, not a hundred times above it; those two are asserted to exceed 1 there."""
    case, lap = _case(cid), _lapack(cid)
    dense = case.n <= cc.DENSE_MAX
    for defect in _defects(case, lap):
        emu = cc.blocked_explicit_inverse(case.A, case.envelope, defect)
        got = case.measure(emu.L, [emu.solve(b) for _, b in case.rhs])
        print(case.name, defect, got)
        assert got["factor_ratio"] > 100.0, (defect, got)
        assert min(got["solve_row_ratio"]) > (100.0 if dense or not defect[0].startswith("float32") else 1.0), (defect, got)


@pytest.mark.parametrize("cid", [("hard_blocks", 700), ("plan", "band")], ids=cc.case_id)
def test_defects_that_keep_the_factor_are_flagged_at_the_carried_kappa_b(cid):
    """The three defects that leave every diagonal block positive definite there (the two float32 roundings, the term left out),
    planted in the ill-conditioned matrices the GPU file uses (kappa_b 1e4 and 1e3): factor_ratio > 100, dense and sampled.  The
    solve metric is asserted above 100 where the well-conditioned teeth above found it able to see the defect at this size (all
    three at n = 700, the single term at n = 5178) and above 1 for the float32 roundings at n = 5178."""
    case, lap = _case(cid), _lapack(cid)
    dense = case.n <= cc.DENSE_MAX
    for defect in _defects(case, lap):
        if defect[0] in ("skip_tile", "skip_panel", "transpose_tile"):
            continue
        emu = cc.blocked_explicit_inverse(case.A, case.envelope, defect)
        got = case.measure(emu.L, [emu.solve(b) for _, b in case.rhs])
        print(case.name, defect, got)
        assert got["factor_ratio"] > 100.0, (defect, got)
        assert min(got["solve_row_ratio"]) > (100.0 if dense or not defect[0].startswith("float32") else 1.0), (defect, got)


@pytest.mark.parametrize("cid,block", cc.NPD_CASES, ids=lambda v: cc.case_id(v) if isinstance(v, tuple) else str(v))
def test_indefinite_inputs_are_rejected_by_lapack_and_their_neighbours_accepted(cid, block):
    case, lap = _case(cid), _lapack(cid)
    bad = cc.indefinite_in_block(case.A, lap.L, block)
    assert np.all(np.diag(bad) == 1.0) and np.array_equal(bad, bad.T)
    diff = bad != case.A
    diff[128 * block:128 * (block + 1), :] = False
    diff[:, 128 * block:128 * (block + 1)] = False
    assert not diff.any()                                                         # only that block's rows and columns differ
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(bad)
    e = 128 * block
    if e:
        np.linalg.cholesky(bad[:e, :e])                                          # nothing is wrong before that block
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(bad[:e + 128, :e + 128])
    np.linalg.cholesky(cc.indefinite_in_block(case.A, lap.L, block, shift=0.5))   # the neighbour on this side of singular
