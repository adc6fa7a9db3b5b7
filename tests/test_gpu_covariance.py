"""Covariance on the device (sk_covariance_compute) on the cases of tests/covariance_cases.py.

    border route   steps 3 to 6 (scaling, the partial factorisation with the selected unit rows as its border, the pivot ratio, the
                   extraction) on a random SPD matrix given as such, through the testing library's entry;
    (i) inversion  the device's blocks against the long-double inverse of J^T J formed from the values that sk_problem_evaluate
                   returns at the same point: assembly, scaling, factorisation, extraction and lift, nothing of the evaluation.
                   Bound per case: max(16 D, 64 u), D the deviation of the float64 restatement from the long-double one on that
                   case (tests/covariance_reference.py), computed here, never taken from the device.  Why 16: the device sums H in
                   plan order and factors in 128-blocks with MFMA accumulation; both orders differ from numpy's column loop, and the
                   error constant of either grows like N u;
    (ii) end to end the same blocks against the independent reference (its own Jacobian): the bound of (i) plus kappa_2 of the
                   reference's scaled normal matrix times the Jacobian tolerance that tests/evaluate_reference.py holds
                   sk_problem_evaluate to (1e-11);
    structure      exact zeros for constant blocks, block(b, a) == block(a, b)^T and get_matrix == the assembled get_blocks bitwise,
                   two computes return the same bytes, apply_loss_function off == a problem built without the loss, the stats;
    rank           an unused coordinate and an unreferenced block fail the compute, and the object recovers;
    lifts          the quaternion's ambient block is 4 x 4 with q in its null space, held intrinsics give zero rows.

Gauge-free bundle adjustment is not asserted either way: floating-point pivots of an exactly singular matrix are not a contract.

SKERES_COVARIANCE_ERROR_FILE=<path>: case, D, the observed deviations and their ratios to the bounds are appended there
(profiles/covariance_error.txt is such a record)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import skeres_amd as sk
import covariance_reference as cv
import covariance_cases as vc
from evaluate_reference import TOL_JAC

pytestmark = pytest.mark.gpu
LD = np.longdouble
VARIANTS = [(name, True) for name in sorted(vc.CASES)] + [("bal-robust", False)]


@pytest.fixture(scope="module", autouse=True)
def _device(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _record(line):
    print(line, flush=True)
    path = os.environ.get("SKERES_COVARIANCE_ERROR_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _run(name, apply_loss=True):
    """One compute of the case on the device, and the Jacobian sk_problem_evaluate returns at the same point; shared."""
    c = vc.case(name)
    cov, ok, problem, params, h, keep = vc.compute(c, apply_loss=apply_loss)
    assert ok, cov.lastError()
    return dict(cov=cov, problem=problem, params=params, h=h, keep=keep, blocks=vc.device_blocks(c, cov, h),
                jacobian=vc.device_jacobian(c, problem, h, apply_loss))


# ---- the border route ------------------------------------------------------------------------------------------------------------
def test_border_route():
    """H = I + A A^T / 300 (300 rows, fixed seed), 140 selected columns (eight blocks of 16 and the last block of 12, scrambled): the
    selected block of the inverse from the partial factorisation's border against the long-double inverse, at max(16 D, 64 u)."""
    path = os.path.join(os.path.dirname(os.path.abspath(sk.__file__)), "libskeres_amd_testing.so")
    lib = C.CDLL(path)
    fn = lib.sk_testing_covariance_border_route
    fn.restype = C.c_int
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    fn.argtypes = [C.c_int, dp, C.c_int, ip, C.c_int, dp, dp]
    n, block = 300, 16
    A = np.random.default_rng(7).normal(0, 1, (n, n))
    H = np.eye(n) + A @ A.T / n
    H = 0.5 * (H + H.T)
    sel_blocks = np.array([18, 3, 0, 17, 5, 9, 11, 2, 14], dtype=np.int32)
    sel = np.concatenate([np.arange(b * block, min(n, (b + 1) * block)) for b in sel_blocks])
    k = len(sel)
    assert k == 140
    out, ratio = np.zeros((k, k)), C.c_double()
    rc = fn(n, H.ctypes.data_as(dp), block, sel_blocks.ctypes.data_as(ip), len(sel_blocks), out.ctypes.data_as(dp), C.byref(ratio))
    lib.sk_last_error.restype = C.c_char_p
    assert rc == 0, (rc, lib.sk_last_error())

    def inverse(T):
        Ht = H.astype(T)
        d = 1 / np.sqrt(np.diag(Ht))
        L = cv.cholesky(Ht * d[:, None] * d[None, :])
        E = np.zeros((n, k), dtype=T)
        E[sel, np.arange(k)] = 1
        X = cv.forward(L, E)
        return (X.T @ X) * d[sel][:, None] * d[sel][None, :], float(np.min(np.diag(L) ** 2) / np.max(np.diag(L) ** 2))
    ref, ref_ratio = inverse(LD)
    scale = float(np.max(np.diag(ref)))
    D = float(np.max(np.abs(inverse(np.float64)[0].astype(LD) - ref))) / scale
    dev = float(np.max(np.abs(out.astype(LD) - ref))) / scale
    tol = max(16 * D, 64 * cv.U)
    _record("border-route         D %.3e  device %.3e  bound %.3e  ratio %.3f   pivot ratio %.6e (reference %.6e)" % (D, dev, tol, dev / tol, ratio.value, ref_ratio))
    assert dev <= tol
    assert np.array_equal(out, out.T)
    assert 0.5 * ref_ratio <= ratio.value <= 2 * ref_ratio


# ---- (i) and (ii) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,apply_loss", VARIANTS)
def test_inversion_and_end_to_end(name, apply_loss):
    c = vc.case(name)
    run = _run(name, apply_loss)
    D, tol = vc.self_deviation(name, apply_loss), vc.tolerance(name, apply_loss)
    # (i): the long-double inverse of J^T J formed from the device's own values
    H = cv.normal_matrix_from_crs(run["jacobian"], c.blocks)
    own = cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, LD)
    dev_i = cv.deviation(run["blocks"], own, c.pairs)
    # (ii): the independent reference
    ref = vc.reference(name, True, apply_loss)
    jac_term = ref["kappa"] * TOL_JAC
    dev_ii = cv.deviation(run["blocks"], ref, c.pairs)
    _record("%-16s loss %d  D %.3e  (i) device %.3e  bound %.3e  ratio %.3f  |  (ii) device %.3e  bound %.3e + kappa_2 %.3e x %.0e = %.3e  ratio %.3f"
            % (name, apply_loss, D, dev_i, tol, dev_i / tol, dev_ii, tol, ref["kappa"], TOL_JAC, tol + jac_term, dev_ii / (tol + jac_term)))
    assert dev_i <= tol, (name, dev_i, tol)
    assert dev_ii <= tol + jac_term, (name, dev_ii, tol + jac_term)
    assert np.array_equal(run["params"].toArray(len(c.x)), c.x)   # the point is read, never written


def test_callback_equals_curve():
    a, b = _run("curve")["blocks"], _run("callback")["blocks"]
    ref = vc.reference("curve", True)
    assert cv.deviation(a, b, vc.case("curve").pairs) <= vc.tolerance("curve")
    assert cv.deviation(b, ref, vc.case("curve").pairs) <= vc.tolerance("curve") + ref["kappa"] * TOL_JAC


# ---- structure -------------------------------------------------------------------------------------------------------------------
def test_constant_blocks_are_exact_zeros():
    b = _run("bal-small")["blocks"]
    for key in ((0, 2), (0, 0)):
        assert b["tangent"][key].shape == (9, 9) and b["ambient"][key].shape == (9, 9)
        assert not np.any(b["tangent"][key]) and not np.any(b["ambient"][key])
    run, c = _run("bal-robust"), vc.case("bal-robust")
    pt5 = 16 + 5
    for a in c.all_of:
        key = (min(a, pt5), max(a, pt5))
        assert not np.any(run["blocks"]["tangent"][key]) and not np.any(run["blocks"]["ambient"][key])


@pytest.mark.parametrize("name", ["bal-small", "tape-quaternion", "chain"])
def test_both_orders_are_transposes_bitwise(name):
    run, c = _run(name), vc.case(name)
    cov, h = run["cov"], run["h"]
    for a, b in c.pairs:
        for get in (cov.getCovarianceBlock, cov.getCovarianceBlockInTangentSpace):
            assert get(h[a], h[b]).tobytes() == np.ascontiguousarray(get(h[b], h[a]).T).tobytes(), (a, b)
    for a in sorted({q for ab in c.pairs for q in ab}):
        if (a, a) in c.pairs:
            t = cov.getCovarianceBlockInTangentSpace(h[a], h[a])
            assert np.array_equal(t, t.T)


def test_get_matrix_equals_the_assembled_blocks_bitwise():
    run, c = _run("bal-robust"), vc.case("bal-robust")
    cov, h = run["cov"], run["h"]
    order = c.all_of[::-1][:7] + c.all_of[:5]              # a listed order of its own: points first, descending
    for tangent, get_m, get_b in ((True, cov.getCovarianceMatrixInTangentSpace, cov.getCovarianceBlockInTangentSpace),
                                  (False, cov.getCovarianceMatrix, cov.getCovarianceBlock)):
        M = get_m([h[b] for b in order])
        rows = [np.concatenate([get_b(h[a], h[b]) for b in order], axis=1) for a in order]
        assert M.tobytes() == np.ascontiguousarray(np.concatenate(rows, axis=0)).tobytes()
        assert M.shape[0] == sum((c.blocks[b].tangent if tangent else c.blocks[b].size) for b in order)
    full = cov.getCovarianceMatrix([h[b] for b in c.all_of])
    assert full.shape == (14 * 9 + 21 * 3, 14 * 9 + 21 * 3)
    for i in range(14):                                    # ambient rows and columns of the held intrinsics are zero
        assert not np.any(full[9 * i + 6:9 * i + 9]) and not np.any(full[:, 9 * i + 6:9 * i + 9])
    # a pair among the listed blocks that was not computed
    with pytest.raises(ValueError, match="was not computed"):
        cov.getCovarianceMatrix([h[2], h[16 + 40]])
    with pytest.raises(ValueError, match="was not computed"):
        cov.getCovarianceBlock(h[2], h[16 + 40])
    with pytest.raises(ValueError, match="not a parameter block"):
        cov.getCovarianceBlock(h[2], sk.RichDoubleArray.fromArray([0.0]))


def test_two_computes_return_the_same_bytes():
    for name in ("bal-duplicate", "chain"):
        c = vc.case(name)
        a = _run(name)["blocks"]
        cov, ok, problem, params, h, keep = vc.compute(c)
        assert ok
        b = vc.device_blocks(c, cov, h)
        again = cov.compute([(h[p], h[q]) for p, q in c.pairs], problem)   # and on the same object
        assert again
        d = vc.device_blocks(c, cov, h)
        for space in ("tangent", "ambient"):
            for key in c.pairs:
                assert a[space][key].tobytes() == b[space][key].tobytes() == d[space][key].tobytes(), (name, space, key)


def test_loss_off_equals_a_problem_without_the_loss_bitwise():
    c = vc.case("bal-robust")
    off = _run("bal-robust", False)["blocks"]
    cov, ok, problem, params, h, keep = vc.compute(c, with_loss=False)
    assert ok
    plain = vc.device_blocks(c, cov, h)
    on = _run("bal-robust", True)["blocks"]
    differ = False
    for space in ("tangent", "ambient"):
        for key in c.pairs:
            assert off[space][key].tobytes() == plain[space][key].tobytes(), (space, key)
            differ = differ or not np.array_equal(on[space][key], off[space][key])
    assert differ


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_stats(name):
    run, ref = _run(name), vc.reference(name)
    cov = run["cov"]
    assert cov.stat("columns") == ref["N"] and cov.stat("selected_columns") == ref["k"]
    assert cov.stat("normal_matrix_pairs") == ref["normal_matrix_pairs"]
    ratio = cov.stat("reciprocal_pivot_ratio")
    print(name, "reciprocal pivot ratio", ratio, "reference", ref["ratio"], [cov.stat("phase_seconds_%d" % i) for i in range(5)], flush=True)
    assert 0.5 * ref["ratio"] <= ratio <= 2 * ref["ratio"]
    assert all(cov.stat("phase_seconds_%d" % i) >= 0 for i in range(5)) and cov.stat("phase_seconds_2") > 0
    with pytest.raises(ValueError):
        cov.stat("no_such_stat")


# ---- rank deficiency -------------------------------------------------------------------------------------------------------------
def _first_coordinate_functor():
    class First(sk.TracedCostFunctor):
        """r = x_0 over a 2-block: x_1 is unused."""

        def __init__(self):
            super().__init__(1, 2)

        def apply(self, x):
            return [x[0] * 1.0]
    return First()


def test_rank_zero_column_and_recovery():
    f = _first_coordinate_functor()
    params = sk.RichDoubleArray.fromArray([0.5, -2.0])
    problem = sk.Problem()
    problem.addResidualBlocksTraced(f, np.zeros((1, 0)), None, params, np.array([[0]], dtype=np.int64))
    cov = sk.Covariance()
    assert cov.compute([params], problem) is False
    msg = cov.lastError()
    assert "rank deficient" in msg and "parameter block 0" in msg and "coordinate 1" in msg
    with pytest.raises(ValueError, match="no covariance has been computed"):
        cov.getCovarianceBlock(params, params)
    held = sk.PredefinedLocalParameterizations.subset(2, [1])
    problem.setParameterization(params, held)
    assert cov.compute([params], problem) is True
    assert np.array_equal(cov.getCovarianceBlockInTangentSpace(params, params), [[1.0]])
    assert np.array_equal(cov.getCovarianceBlock(params, params), [[1.0, 0.0], [0.0, 0.0]])
    assert cov.stat("columns") == 1


def test_unreferenced_block_is_rank_deficient():
    c = vc.case("curve")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    extra = sk.RichDoubleArray.fromArray([1.0, 2.0])
    problem.addParameterBlock(extra, 2)
    cov = sk.Covariance()
    assert cov.compute([(h[0], h[1])], problem) is False
    assert "rank deficient" in cov.lastError() and "parameter block 2" in cov.lastError() and "coordinate 0" in cov.lastError()
    problem.setParameterBlockConstant(extra)
    assert cov.compute([(h[0], h[1]), (extra, h[0])], problem) is True
    assert not np.any(cov.getCovarianceBlock(extra, h[0])) and cov.getCovarianceBlock(h[0], extra).shape == (1, 2)


def test_a_problem_of_constant_blocks_gives_zeros():
    c = vc.case("curve")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    for b in h:
        problem.setParameterBlockConstant(b)
    cov = sk.Covariance()
    assert cov.compute(h, problem) is True and cov.stat("columns") == 0 and cov.stat("selected_columns") == 0
    assert np.array_equal(cov.getCovarianceMatrix(h), np.zeros((2, 2))) and np.array_equal(cov.getCovarianceBlockInTangentSpace(h[1], h[0]), [[0.0]])


def test_a_failing_functor_is_an_error_not_rank_deficiency():
    import evaluate_cases as ec
    problem, _, params, keep = ec.bal_host(failing=True).build()
    cov = sk.Covariance()
    with pytest.raises(sk.SkeresError, match="status 5"):
        cov.compute([params.slice(0)], problem)


# ---- lifts -----------------------------------------------------------------------------------------------------------------------
def test_quaternion_and_subset_lifts():
    run, c = _run("tape-quaternion"), vc.case("tape-quaternion")
    ref = vc.reference("tape-quaternion", True)
    amb, tan = run["blocks"]["ambient"][(0, 0)], run["blocks"]["tangent"][(0, 0)]
    assert tan.shape == (3, 3) and amb.shape == (4, 4) and run["blocks"]["ambient"][(0, 1)].shape == (4, 3)
    q = c.x[:4]
    assert float(np.max(np.abs(amb @ q))) <= 64 * cv.U * float(np.linalg.norm(amb))
    assert np.linalg.matrix_rank(amb, tol=1e-9 * np.linalg.norm(amb)) == 3
    assert cv.deviation(run["blocks"], ref, c.pairs, spaces=("ambient",)) <= vc.tolerance("tape-quaternion") + ref["kappa"] * TOL_JAC
    run, c = _run("bal-robust"), vc.case("bal-robust")
    ref = vc.reference("bal-robust", True)
    amb = run["blocks"]["ambient"][(2, 3)]
    assert amb.shape == (9, 9) and not np.any(amb[6:]) and not np.any(amb[:, 6:])
    assert amb[:6, :6].tobytes() == np.ascontiguousarray(run["blocks"]["tangent"][(2, 3)]).tobytes()   # a subset lift is a scatter
    assert cv.deviation(run["blocks"], ref, c.pairs, spaces=("ambient",)) <= vc.tolerance("bal-robust") + ref["kappa"] * TOL_JAC
