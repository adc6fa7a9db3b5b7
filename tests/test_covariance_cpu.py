"""Covariance without a device: the validation of the options, every SK_ERR_INVALID_ARGUMENT that needs no compute, SK_ERR_NO_DEVICE,
the refusals that are decided from host data alone, the reference (tests/covariance_reference.py) against itself in float64 and in
long double on every case of tests/covariance_cases.py, what each case is there to exercise, and the comparison shown to reject
planted defects at the tolerance the device is held to."""
import ctypes as C

import numpy as np
import pytest

import skeres_amd as sk
import covariance_reference as cv
import covariance_cases as vc
import cgnr_cases as cc

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _status(fn):
    with pytest.raises(sk.SkeresError) as e:
        fn()
    return str(e.value)


# ---- options and arguments -------------------------------------------------------------------------------------------------------
def test_option_validation():
    o = sk.Covariance.Options()
    o.applyLossFunction(False)
    o.applyLossFunction(True)
    for good in (0.0, 1e-14, 0.5, 1.0 - 2.0 ** -53):
        o.minReciprocalConditionNumber(good)
    for bad in (-1e-300, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            o.minReciprocalConditionNumber(bad)
    o.setDevice(0)
    lib = sk.lib()
    assert lib.sk_covariance_options_set_apply_loss_function(None, 1) == 1
    assert lib.sk_covariance_options_set_min_reciprocal_condition_number(None, 0.5) == 1
    assert lib.sk_covariance_options_set_device(None, 0) == 1
    assert sk.Covariance(None)._h            # options may be NULL


def test_invalid_arguments_need_no_device():
    c = vc.case("curve")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    cov = sk.Covariance()
    stranger = sk.RichDoubleArray.fromArray([0.0])
    with pytest.raises(ValueError, match="no parameter block"):
        cov.compute([(h[0], stranger)], problem)
    with pytest.raises(ValueError, match="no parameter block"):
        cov.compute([stranger], problem)
    with pytest.raises(ValueError):
        cov.compute([], problem)                      # num_pairs <= 0
    lib = sk.lib()
    pp = (C.POINTER(C.c_double) * 1)(h[0].cast())
    assert lib.sk_covariance_compute(cov._h, problem._h, pp, pp, 0) == 1
    assert lib.sk_covariance_compute(cov._h, problem._h, pp, pp, -3) == 1
    assert lib.sk_covariance_compute_blocks(cov._h, problem._h, pp, 0) == 1
    assert lib.sk_covariance_compute(None, problem._h, pp, pp, 1) == 1
    assert lib.sk_covariance_compute(cov._h, None, pp, pp, 1) == 1
    # getters before a successful compute
    for get in (cov.getCovarianceBlock, cov.getCovarianceBlockInTangentSpace):
        with pytest.raises(ValueError, match="no covariance has been computed"):
            get(h[0], h[0])
    for get in (cov.getCovarianceMatrix, cov.getCovarianceMatrixInTangentSpace):
        with pytest.raises(ValueError, match="no covariance has been computed"):
            get([h[0], h[1]])
    with pytest.raises(ValueError):
        cov.stat("columns")


def test_without_a_device_compute_reports_no_device():
    if sk.device_count() > 0:
        pytest.skip("a device is present: the compute runs (tests/test_gpu_covariance.py)")
    c = vc.case("curve")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    pp = (C.POINTER(C.c_double) * 1)(h[0].cast())
    cov = sk.Covariance()
    assert sk.lib().sk_covariance_compute(cov._h, problem._h, pp, pp, 1) == 2 and b"no HIP device" in sk.lib().sk_last_error()
    with pytest.raises(ValueError, match="no covariance has been computed"):
        cov.getCovarianceBlock(h[0], h[0])


def test_refusals_from_host_data_alone():
    """SK_ERR_UNSUPPORTED before a device is asked for: with or without one, the status is 4."""
    cov = sk.Covariance()
    # N above the cap: 2049 blocks of 16 columns
    x = sk.RichDoubleArray.ofSize(16 * 2049)
    problem = sk.Problem()
    for i in range(2049):
        problem.addParameterBlock(x.slice(16 * i), 16)
    msg = _status(lambda: cov.compute([x.slice(0)], problem))
    assert "status 4" in msg and "32768" in msg and "32784" in msg and "reduced camera system is not built" in msg
    # a tangent size above 16
    y = sk.RichDoubleArray.ofSize(17)
    problem = sk.Problem()
    problem.addParameterBlock(y, 17)
    msg = _status(lambda: cov.compute([y], problem))
    assert "status 4" in msg and "17" in msg
    # dense rows
    from skeres_amd import dense_synth  # noqa: F401  (the functor's home)
    z = sk.RichDoubleArray.ofSize(4)
    problem = sk.Problem()
    problem.addDenseRows(10, np.array([[1.0, 0.0, 0.5], [1.0, 1.0, -0.5]]), None, z, 4)
    msg = _status(lambda: cov.compute([z], problem))
    assert "status 4" in msg and "dense" in msg


# ---- the reference itself --------------------------------------------------------------------------------------------------------
VARIANTS = [(name, True) for name in sorted(vc.CASES)] + [("bal-robust", False)]


@pytest.mark.parametrize("name,with_loss", VARIANTS)
def test_reference_in_double_and_long_double(name, with_loss):
    """On every case the float64 restatement stays within 1e-9 of the long-double one in the metric."""
    D = vc.self_deviation(name, with_loss)
    r = vc.reference(name, False, with_loss)
    print("%s loss %d: N %d k %d pairs %d kappa_2 %.3e pivot ratio %.3e float64 against long double %.3e"
          % (name, with_loss, r["N"], r["k"], r["normal_matrix_pairs"], r["kappa"], r["ratio"], D), flush=True)
    assert D <= 1e-9


def test_curve_against_the_closed_form():
    H, _ = vc.normal_matrix("curve", True)
    det = H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]
    closed = np.array([[H[1, 1], -H[0, 1]], [-H[1, 0], H[0, 0]]], dtype=LD) / det
    r = vc.reference("curve", True)
    got = np.block([[r["tangent"][(0, 0)], r["tangent"][(0, 1)]], [r["tangent"][(0, 1)].T, r["tangent"][(1, 1)]]])
    assert float(np.max(np.abs(got - closed)) / np.max(np.abs(closed))) <= 64 * cv.U * 40   # (kappa_2 = 38)
    assert np.array_equal(vc.reference("callback", True)["tangent"][(0, 1)], r["tangent"][(0, 1)])


def test_cases_exercise_what_they_are_there_for():
    small, robust = vc.reference("bal-small"), vc.reference("bal-robust")
    assert small["N"] == 156 and 128 < small["N"] <= 256 and small["k"] <= 128         # H: two 128-blocks; the border: a third
    assert robust["N"] == 1881 and robust["k"] == 144 > 128                            # two border block rows
    prob = cc.bal_problem("bal-robust")
    seen = np.bincount(prob.camera_index, minlength=prob.num_cameras)[2:]
    assert any(128 < n <= 192 for n in seen) and seen.max() > 192 and seen.min() > 64    # a camera's diagonal pair: two, three and four parts
    c = vc.case("bal-small")
    C6 = 6
    assert np.all(small["tangent"][(0, 2)] == 0) and small["tangent"][(0, 2)].shape == (9, 9) and np.all(small["ambient"][(0, 0)] == 0)
    assert (C6 + 7, C6 + 5) in c.pairs                                                  # a pair given in descending order
    # bal-duplicate: one more residual block, the same pairs of blocks
    assert vc.reference("bal-duplicate")["normal_matrix_pairs"] == small["normal_matrix_pairs"]
    assert vc.normal_matrix("bal-duplicate")[0].shape == (156, 156)
    # chain: the hub's diagonal pair has five full parts and a partial one; a reversed neighbour pair; a held block
    chain = vc.case("chain")
    hub = cc.CHAIN_HUB
    on_hub = sum(1 for blk in chain.model().blocks if hub in blk[2])
    assert 5 * 64 < on_hub < 6 * 64
    assert any(blk[2] == [6, 5] for blk in chain.model().blocks) and (6, 5) in chain.pairs
    assert vc.reference("chain")["N"] == 2 * (vc.CHAIN_BLOCKS - 1)
    # loss on and off differ; ambient rows of held intrinsics are zero
    on, off = vc.reference("bal-robust", False, True), vc.reference("bal-robust", False, False)
    assert cv.deviation(off, on, vc.case("bal-robust").pairs) > 1e-3
    amb = on["ambient"][(2, 3)]
    assert amb.shape == (9, 9) and np.all(amb[6:] == 0) and np.all(amb[:, 6:] == 0) and np.any(amb[:6, :6] != 0)
    assert on["tangent"][(2, 3)].shape == (6, 6)
    # the quaternion block: tangent 3 x 3, ambient 4 x 4 with q in its null space
    q = vc.reference("tape-quaternion", True)
    amb = q["ambient"][(0, 0)]
    assert q["tangent"][(0, 0)].shape == (3, 3) and amb.shape == (4, 4)
    x = vc.case("tape-quaternion").x[:4].astype(LD)
    assert float(np.max(np.abs(amb @ x))) <= 64 * cv.U * float(np.linalg.norm(amb.astype(np.float64)))


def test_rank_deficiency_in_the_reference():
    """An unused coordinate is an exactly zero diagonal entry: the reference names the block and the coordinate."""
    blocks = [cv.Block(2, 2, [0, 1], False, None)]
    H = np.array([[4.0, 0.0], [0.0, 0.0]])
    with pytest.raises(cv.RankDeficient) as e:
        cv.covariance(H, blocks, np.zeros(2), [0], [(0, 0)], np.float64)
    assert (e.value.block, e.value.coordinate) == (0, 1)


# ---- planted defects -------------------------------------------------------------------------------------------------------------
def _swapped(ref, key, space, value):
    out = {s: dict(ref[s]) for s in ("tangent", "ambient")}
    out[space][key] = value
    return out


def test_the_comparison_rejects_planted_defects():
    """Each defect is planted into the float64 restatement and compared with the long-double reference at the bound the device is
    held to, max(16 D, 64 u): it must be rejected; the restatement without a defect passes."""
    def verdict(name, got, with_loss=True):
        return cv.deviation(got, vc.reference(name, True, with_loss), vc.case(name).pairs), vc.tolerance(name, with_loss)

    for name in ("bal-small", "bal-robust", "bal-duplicate", "chain", "tape-quaternion"):
        dev, tol = verdict(name, vc.reference(name))
        assert dev <= tol, (name, dev, tol)
    # no loss correction under Huber
    dev, tol = verdict("bal-robust", vc.reference("bal-robust", False, False))
    print("no loss correction: %.3e against %.3e" % (dev, tol), flush=True)
    assert dev > tol
    # a missing d_i d_j
    c = vc.case("bal-small")
    got = cv.covariance(vc.normal_matrix("bal-small")[0], c.blocks, c.x, c.offsets, c.pairs, np.float64, scale=False)
    dev, tol = verdict("bal-small", got)
    print("missing d_i d_j: %.3e against %.3e" % (dev, tol), flush=True)
    assert dev > tol
    # a pair's block transposed
    ref = vc.reference("bal-small")
    dev, tol = verdict("bal-small", _swapped(ref, (2, 3), "tangent", ref["tangent"][(2, 3)].T.copy()))
    print("block transposed: %.3e against %.3e" % (dev, tol), flush=True)
    assert dev > tol
    # the second term of the duplicate pair dropped: the (camera, point) block of H as bal-small has it
    c = vc.case("bal-duplicate")
    _, cam, pt = vc.duplicate_observation()
    first, _ = cv.columns(c.blocks)
    H = vc.normal_matrix("bal-duplicate")[0].copy()
    rows, cols = slice(first[cam], first[cam] + 9), slice(first[6 + pt], first[6 + pt] + 3)
    H[rows, cols] = vc.normal_matrix("bal-small")[0][rows, cols]
    H[cols, rows] = H[rows, cols].T
    dev, tol = verdict("bal-duplicate", cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, np.float64))
    print("second term of the duplicate pair dropped: %.3e against %.3e" % (dev, tol), flush=True)
    assert dev > tol
    # the last part of the hub's diagonal dropped: its last two terms
    c = vc.case("chain")
    hub_cols = np.arange(first_col(c, cc.CHAIN_HUB), first_col(c, cc.CHAIN_HUB) + 2)
    seen = []

    def record(mine, index):
        for J, cols in mine:
            if np.array_equal(cols, hub_cols):
                seen.append(J.T @ J)
        return mine
    H = cv.normal_matrix(c.model(), c.x, c.blocks, np.float64, defect=record)[0]
    assert len(seen) == 322
    H[np.ix_(hub_cols, hub_cols)] -= seen[-1] + seen[-2]
    try:   # (what is left is no Gram matrix any more: a failed factorisation rejects the defect as well)
        dev, tol = verdict("chain", cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, np.float64))
    except cv.RankDeficient:
        dev, tol = float("inf"), vc.tolerance("chain")
    print("last part of the hub's diagonal dropped: %.3e against %.3e" % (dev, tol), flush=True)
    assert dev > tol
    # ambient returned where tangent was asked for
    ref = vc.reference("tape-quaternion")
    dev, tol = verdict("tape-quaternion", _swapped(ref, (0, 1), "tangent", ref["ambient"][(0, 1)]))
    assert dev > tol


def first_col(c, b):
    return cv.columns(c.blocks)[0][b]
