"""Covariance with the Schur elimination on the device (sk_covariance_options_set_schur_elimination) on the cases of
tests/covariance_schur_cases.py: those of tests/covariance_cases.py, bal-landmark and bal-wide (33 054 columns).

    (i) inversion  the device's blocks against the long-double inverse of J^T J formed from the values that sk_problem_evaluate
                   returns at the same point (bal-wide: against the long-double ELIMINATION of those values — a dense inverse of
                   33 054 columns is not a test).  Bound per case: max(16 D, 64 u), D the deviation of the float64 restatement OF
                   THIS ROUTE (tests/covariance_schur_reference.py) from its long-double run, computed here, never taken from the
                   device;
    (ii) end to end the same blocks against the independent reference (its own Jacobian): the bound of (i) plus kappa_2 of the scaled
                   normal matrix times the Jacobian tolerance of tests/evaluate_reference.py (1e-11); kappa_2 is the restatement's
                   estimate from below (power iterations), so the bound is never wider than with the exact value;
    cross-route    option on against option off on every case the dense route takes: within the sum of the two routes' bounds;
    structure      two computes return the same bytes, (b, a) is (a, b) transposed bitwise, constant blocks are exact zeros, the
                   stats agree with the plan, an unreferenced moving block is reported by block and coordinate, the quaternion
                   block is eliminated and lifted to 4 x 4 of rank 3, bal-duplicate's (g, e) tile sums two residual blocks,
                   get_matrix over mixed E and F blocks equals the assembled blocks bitwise.

SKERES_COVARIANCE_ERROR_FILE=<path>: case, D, the observed deviations and their ratios to the bounds are appended there
(profiles/covariance_schur_error.txt is such a record)."""
import functools
import os

import numpy as np
import pytest

import skeres_amd as sk
import covariance_reference as cv
import covariance_cases as vc
import covariance_schur_cases as scs
import covariance_schur_reference as sr
from evaluate_reference import TOL_JAC

pytestmark = pytest.mark.gpu
LD = np.longdouble
VARIANTS = [(name, True) for name in sorted(scs.CASES)] + [("bal-robust", False)]


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
def _run(name, apply_loss=True, schur=True):
    """One compute of the case on the device, and the Jacobian sk_problem_evaluate returns at the same point; shared."""
    c = scs.case(name)
    cov, ok, problem, params, h, keep = vc.compute(c, apply_loss=apply_loss, options=scs.options(schur))
    assert ok, cov.lastError()
    return dict(cov=cov, problem=problem, params=params, h=h, keep=keep, blocks=vc.device_blocks(c, cov, h),
                jacobian=vc.device_jacobian(c, problem, h, apply_loss) if schur else None)


@functools.lru_cache(maxsize=None)
def _dense_bound(name, apply_loss=True):
    """max(16 D, 64 u) of the dense route (tests/test_gpu_covariance.py) on a case it takes."""
    if name in vc.CASES:
        return vc.tolerance(name, apply_loss)
    c = scs.case(name)
    refs = []
    for T in (np.float64, LD):
        H, _ = cv.normal_matrix(c.model(apply_loss), c.x, c.blocks, T)
        refs.append(cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, T))
    return max(16 * cv.deviation(refs[0], refs[1], c.pairs), 64 * cv.U)


# ---- (i) and (ii) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,apply_loss", VARIANTS)
def test_inversion_and_end_to_end(name, apply_loss):
    c = scs.case(name)
    run = _run(name, apply_loss)
    D, tol = scs.self_deviation(name, apply_loss), scs.tolerance(name, apply_loss)
    # (i): the long-double inverse of J^T J formed from the device's own values
    if name in scs.DENSE:
        own = cv.covariance(cv.normal_matrix_from_crs(run["jacobian"], c.blocks), c.blocks, c.x, c.offsets, c.pairs, LD)
    else:
        own = sr.eliminate(sr.crs_coo(run["jacobian"], c.blocks), c.blocks, c.x, c.offsets, c.pairs, LD, order=scs.problem_order(name))
    dev_i = cv.deviation(run["blocks"], own, c.pairs)
    # (ii): the independent reference
    ref = scs.reference(name, True, apply_loss)
    jac_term = ref["kappa"] * TOL_JAC
    dev_ii = cv.deviation(run["blocks"], ref, c.pairs)
    _record("%-16s loss %d  D %.3e  (i) device %.3e  bound %.3e  ratio %.3f  |  (ii) device %.3e  bound %.3e + kappa_2 %.3e x %.0e = %.3e  ratio %.3f"
            % (name, apply_loss, D, dev_i, tol, dev_i / tol, dev_ii, tol, ref["kappa"], TOL_JAC, tol + jac_term, dev_ii / (tol + jac_term)))
    assert dev_i <= tol, (name, dev_i, tol)
    assert dev_ii <= tol + jac_term, (name, dev_ii, tol + jac_term)
    assert np.array_equal(run["params"].toArray(len(c.x)), c.x)   # the point is read, never written


@pytest.mark.parametrize("name,apply_loss", [(n, l) for n, l in VARIANTS if n in scs.DENSE])
def test_the_two_routes_agree(name, apply_loss):
    c = scs.case(name)
    on, off = _run(name, apply_loss)["blocks"], _run(name, apply_loss, False)["blocks"]
    ref = scs.reference(name, True, apply_loss)
    bound = scs.tolerance(name, apply_loss) + _dense_bound(name, apply_loss)
    worst, bitwise = 0.0, True
    for space in ("tangent", "ambient"):
        for a, b in c.pairs:
            worst = max(worst, cv.metric(on[space][(a, b)], off[space][(a, b)], ref[space][(a, a)], ref[space][(b, b)]))
            bitwise = bitwise and on[space][(a, b)].tobytes() == off[space][(a, b)].tobytes()
    _record("%-16s loss %d  cross-route %.3e  bound %.3e  ratio %.3f  bitwise %d" % (name, apply_loss, worst, bound, worst / bound, bitwise))
    assert worst <= bound
    assert _run(name, apply_loss, False)["cov"].stat("schur_elimination") == 0 and _run(name, apply_loss)["cov"].stat("schur_elimination") == 1


# ---- structure -------------------------------------------------------------------------------------------------------------------
def test_two_computes_return_the_same_bytes():
    for name in ("bal-landmark", "chain"):
        c = scs.case(name)
        a = _run(name)["blocks"]
        cov, ok, problem, params, h, keep = vc.compute(c, options=scs.options())
        assert ok
        b = vc.device_blocks(c, cov, h)
        again = cov.compute([(h[p], h[q]) for p, q in c.pairs], problem)   # and on the same object
        assert again
        d = vc.device_blocks(c, cov, h)
        for space in ("tangent", "ambient"):
            for key in c.pairs:
                assert a[space][key].tobytes() == b[space][key].tobytes() == d[space][key].tobytes(), (name, space, key)


@pytest.mark.parametrize("name", ["bal-landmark", "tape-quaternion", "chain", "bal-wide"])
def test_both_orders_are_transposes_bitwise(name):
    run, c = _run(name), scs.case(name)
    cov, h = run["cov"], run["h"]
    for a, b in c.pairs:
        for get in (cov.getCovarianceBlock, cov.getCovarianceBlockInTangentSpace):
            assert get(h[a], h[b]).tobytes() == np.ascontiguousarray(get(h[b], h[a]).T).tobytes(), (a, b)
    for a in sorted({q for ab in c.pairs for q in ab}):
        if (a, a) in c.pairs:
            for get in (cov.getCovarianceBlock, cov.getCovarianceBlockInTangentSpace):
                t = get(h[a], h[a])
                assert np.array_equal(t, t.T), a


def test_constant_blocks_are_exact_zeros():
    b = _run("bal-landmark")["blocks"]
    assert b["tangent"][(0, 0)].shape == (9, 9) and not np.any(b["tangent"][(0, 0)]) and not np.any(b["ambient"][(0, 0)])
    run, c = _run("bal-robust"), scs.case("bal-robust")
    pt5 = 16 + 5
    for a in c.all_of:
        key = (min(a, pt5), max(a, pt5))
        assert not np.any(run["blocks"]["tangent"][key]) and not np.any(run["blocks"]["ambient"][key])


@pytest.mark.parametrize("name", sorted(scs.CASES))
def test_stats_agree_with_the_plan(name):
    run, ref = _run(name), scs.reference(name, True)
    cov = run["cov"]
    plan = sk.Covariance.eliminationPlan(run["problem"])
    assert cov.stat("columns") == ref["N"] and cov.stat("selected_columns") == ref["k"] and cov.stat("schur_elimination") == 1
    assert cov.stat("eliminated_blocks") == plan["num_eliminated"] == len(ref["E"])
    assert cov.stat("reduced_columns") == plan["reduced_columns"] == ref["reduced_columns"]
    assert cov.stat("schur_terms") == plan["schur_terms"] == ref["schur_terms"]
    ratio = cov.stat("reciprocal_pivot_ratio")
    print(name, "reciprocal pivot ratio", ratio, "reference", ref["ratio"], [cov.stat("phase_seconds_%d" % i) for i in range(5)], flush=True)
    assert 0.5 * ref["ratio"] <= ratio <= 2 * ref["ratio"]
    assert all(cov.stat("phase_seconds_%d" % i) >= 0 for i in range(5)) and cov.stat("phase_seconds_2") > 0


def test_unreferenced_block_is_reported_by_block_and_coordinate():
    c = scs.case("curve")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    extra = sk.RichDoubleArray.fromArray([1.0, 2.0])
    problem.addParameterBlock(extra, 2)
    assert sk.Covariance.eliminationPlan(problem)["eliminated_of_block"][2] == 1     # degree 0: it joins E first
    cov = sk.Covariance(scs.options())
    assert cov.compute([(h[0], h[1])], problem) is False
    assert "rank deficient" in cov.lastError() and "parameter block 2" in cov.lastError() and "coordinate 0" in cov.lastError()
    problem.setParameterBlockConstant(extra)
    assert cov.compute([(h[0], h[1]), (extra, h[0])], problem) is True
    assert not np.any(cov.getCovarianceBlock(extra, h[0])) and cov.getCovarianceBlock(h[0], extra).shape == (1, 2)


def test_quaternion_block_is_eliminated_and_lifted():
    run, c = _run("tape-quaternion"), scs.case("tape-quaternion")
    ref = scs.reference("tape-quaternion", True)
    assert ref["E"] == [0] and list(sk.Covariance.eliminationPlan(run["problem"])["eliminated_of_block"]) == [1, 0]
    amb, tan = run["blocks"]["ambient"][(0, 0)], run["blocks"]["tangent"][(0, 0)]
    assert tan.shape == (3, 3) and amb.shape == (4, 4) and run["blocks"]["ambient"][(0, 1)].shape == (4, 3)
    q = c.x[:4]
    assert float(np.max(np.abs(amb @ q))) <= 64 * cv.U * float(np.linalg.norm(amb))
    assert np.linalg.matrix_rank(amb, tol=1e-9 * np.linalg.norm(amb)) == 3
    assert cv.deviation(run["blocks"], ref, c.pairs, spaces=("ambient",)) <= scs.tolerance("tape-quaternion") + ref["kappa"] * TOL_JAC


def test_a_tile_built_from_two_residual_blocks():
    """bal-duplicate: (camera, point) of the repeated observation is one (g, e) tile that sums two residual blocks."""
    c = scs.case("bal-duplicate")
    _, cam, pt = vc.duplicate_observation()
    C_ = 6
    run, ref = _run("bal-duplicate"), scs.reference("bal-duplicate", True)
    assert C_ + pt in ref["E"] and cam in ref["F"]
    single = _run("bal-small")["blocks"]["tangent"][(cam, cam)] if (cam, cam) in scs.case("bal-small").pairs else None
    key = (cam, C_ + pt)
    assert key in c.pairs
    bound = scs.tolerance("bal-duplicate") + ref["kappa"] * TOL_JAC
    assert cv.metric(run["blocks"]["tangent"][key], ref["tangent"][key], ref["tangent"][(cam, cam)], ref["tangent"][(C_ + pt, C_ + pt)]) <= bound
    if single is not None:
        assert not np.array_equal(single, run["blocks"]["tangent"][(cam, cam)])     # the second observation moved it


def test_get_matrix_over_mixed_blocks_equals_the_assembled_blocks_bitwise():
    c = scs.case("bal-small")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    order = [6 + 7, 2, 6 + 5, 0, 3]                       # points (E), moving cameras (F) and a constant camera, in an order of its own
    cov = sk.Covariance(scs.options())
    assert cov.compute([h[b] for b in order], problem)
    for get_m, get_b in ((cov.getCovarianceMatrixInTangentSpace, cov.getCovarianceBlockInTangentSpace), (cov.getCovarianceMatrix, cov.getCovarianceBlock)):
        M = get_m([h[b] for b in order])
        rows = [np.concatenate([get_b(h[a], h[b]) for b in order], axis=1) for a in order]
        assert M.tobytes() == np.ascontiguousarray(np.concatenate(rows, axis=0)).tobytes()
        assert M.shape == (3 + 9 + 3 + 9 + 9,) * 2 and np.array_equal(M, M.T) and not np.any(M[15:24])
