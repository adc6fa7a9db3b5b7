"""Covariance with the Schur elimination, without a device: the eliminated set that sk_covariance_elimination_plan reports against the
restatement's own greedy set on every case of tests/covariance_schur_cases.py, the setter, the default route's refusal untouched, the
refusals of the new route from host data alone, and the comparison metric shown to reject defects planted in the restatement's
own output (tests/covariance_schur_reference.py) at the tolerance the device is held to."""
import ctypes as C

import numpy as np
import pytest

import skeres_amd as sk
import covariance_reference as cv
import covariance_cases as vc
import covariance_schur_cases as scs
import covariance_schur_reference as sr

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _status(fn):
    with pytest.raises(sk.SkeresError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("name", sorted(scs.CASES))
def test_elimination_plan_equals_the_restatement(name):
    c = scs.case(name)
    problem, params, keep = c.build()
    got = sk.Covariance.eliminationPlan(problem)
    order = scs.problem_order(name)
    want = sr.plan(scs.model_coo(name), c.blocks, order)
    print(name, "E", want["num_eliminated"], "reduced columns", want["reduced_columns"], "Schur terms", want["schur_terms"], flush=True)
    assert np.array_equal(got["eliminated_of_block"][list(order)], want["eliminated_of_block"])
    assert got["num_eliminated"] == want["num_eliminated"] and got["reduced_columns"] == want["reduced_columns"]
    assert got["schur_terms"] == want["schur_terms"]


def test_cases_exercise_what_they_are_there_for():
    C_, P = scs.LANDMARK_CAMERAS, scs.LANDMARK_POINTS
    p = sr.plan(scs.model_coo("bal-landmark"), scs.case("bal-landmark").blocks, scs.problem_order("bal-landmark"))
    assert list(p["eliminated_of_block"]) == [-1, -1] + [0] * (C_ - 2) + [1] * (P + 1)      # the points, the landmark of 68 frames among them
    assert p["reduced_columns"] == 9 * (C_ - 2)
    p = sr.plan(scs.model_coo("bal-wide"), scs.case("bal-wide").blocks, scs.problem_order("bal-wide"))
    assert p["reduced_columns"] == 54 and p["num_eliminated"] == scs.WIDE_POINTS
    assert 54 + 3 * scs.WIDE_POINTS == 33054 > 32768
    p = sr.plan(scs.model_coo("chain"), scs.case("chain").blocks, scs.problem_order("chain"))
    import cgnr_cases as cc
    assert p["eliminated_of_block"][cc.CHAIN_HUB] == 0 and p["eliminated_of_block"][vc.CHAIN_HELD] == -1     # the hub stays in F
    assert p["num_eliminated"] >= 300
    p = sr.plan(scs.model_coo("tape-quaternion"), scs.case("tape-quaternion").blocks, scs.problem_order("tape-quaternion"))
    assert list(p["eliminated_of_block"]) == [1, 0]                                         # the quaternion block is eliminated


def test_setter_and_plan_arguments():
    o = sk.Covariance.Options()
    o.schurElimination(True)
    o.schurElimination(False)
    lib = sk.lib()
    assert lib.sk_covariance_options_set_schur_elimination(None, 1) == 1
    assert lib.sk_covariance_elimination_plan(None, None, None, None, None) == 1
    c = scs.case("curve")
    problem, params, keep = c.build()
    n = C.c_int(-1)
    assert lib.sk_covariance_elimination_plan(problem._h, None, C.byref(n), None, None) == 0 and n.value == 1     # every output may be NULL


def _above_the_cap():
    x = sk.RichDoubleArray.ofSize(16 * 2049)
    problem = sk.Problem()
    for i in range(2049):
        problem.addParameterBlock(x.slice(16 * i), 16)
    return x, problem


def test_the_default_still_refuses_above_the_cap():
    """tests/test_covariance_cpu.py's refusal restated: the default route is untouched, and its message points at the setter."""
    x, problem = _above_the_cap()
    msg = _status(lambda: sk.Covariance().compute([x.slice(0)], problem))
    assert "status 4" in msg and "32768" in msg and "32784" in msg and "reduced camera system is not built" in msg
    assert "sk_covariance_options_set_schur_elimination" in msg
    o = scs.options(False)
    assert "status 4" in _status(lambda: sk.Covariance(o).compute([x.slice(0)], problem))


def test_bal_wide_passes_the_plan():
    """33 054 columns: the default refuses from host data; with the option the plan is accepted and the compute goes to the device."""
    c = scs.case("bal-wide")
    problem, params, keep = c.build()
    h = vc.handles(c, params)
    pp = (C.POINTER(C.c_double) * 1)(h[2].cast())
    lib = sk.lib()
    assert lib.sk_covariance_compute(sk.Covariance()._h, problem._h, pp, pp, 1) == 4 and b"33054" in lib.sk_last_error()
    cov = sk.Covariance(scs.options())
    rc = lib.sk_covariance_compute(cov._h, problem._h, pp, pp, 1)
    if sk.device_count() == 0:
        assert rc == 2 and b"no HIP device" in lib.sk_last_error()
    else:
        assert rc == 0, lib.sk_last_error()


def test_refusals_from_host_data_alone():
    cov = sk.Covariance(scs.options())
    # 2049 blocks of 16 that no residual block names: an independent set — nothing is left after the elimination, the plan passes
    x, problem = _above_the_cap()
    plan = sk.Covariance.eliminationPlan(problem)
    assert plan["num_eliminated"] == 2049 and plan["reduced_columns"] == 0 and plan["schur_terms"] == 0
    # more than 32 768 columns left after the elimination: a path of 4100 blocks of 16 keeps every other block, 2050 of them
    n = 4100
    y = sk.RichDoubleArray.ofSize(16 * n)
    problem = sk.Problem()
    f = _pair_functor()
    offs = np.stack([16 * np.arange(n - 1, dtype=np.int64), 16 * np.arange(1, n, dtype=np.int64)], axis=1)
    problem.addResidualBlocksTraced(f, np.zeros((n - 1, 0)), None, y, offs)
    msg = _status(lambda: cov.compute([y.slice(0)], problem))
    assert "status 4" in msg and "32768" in msg and "32800" in msg and "after the elimination" in msg
    msg = _status(lambda: sk.Covariance.eliminationPlan(problem))
    assert "after the elimination" in msg
    # a tangent size above 16 and dense rows, as without the option
    z = sk.RichDoubleArray.ofSize(17)
    problem = sk.Problem()
    problem.addParameterBlock(z, 17)
    msg = _status(lambda: cov.compute([z], problem))
    assert "status 4" in msg and "17" in msg
    from skeres_amd import dense_synth  # noqa: F401  (the functor's home)
    w = sk.RichDoubleArray.ofSize(4)
    problem = sk.Problem()
    problem.addDenseRows(10, np.array([[1.0, 0.0, 0.5], [1.0, 1.0, -0.5]]), None, w, 4)
    msg = _status(lambda: cov.compute([w], problem))
    assert "status 4" in msg and "dense" in msg


def _pair_functor():
    class Pair(sk.TracedCostFunctor):
        """r = x_0 - y_0 over two 16-blocks."""

        def __init__(self):
            super().__init__(1, 16, 16)

        def apply(self, x, y):
            return [x[0] - y[0]]
    return Pair()


# ---- the restatement itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scs.DENSE)
def test_restatement_against_the_dense_reference(name):
    """In long double the elimination and the dense inverse of tests/covariance_reference.py are the same blocks: far inside the
    bound the device is held to (both carry kappa_2 u of long double)."""
    c = scs.case(name)
    r = scs.reference(name, True)
    if name in vc.CASES:
        dense = vc.reference(name, True)
    else:
        H, _ = cv.normal_matrix(c.model(True), c.x, c.blocks, LD)
        dense = cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, LD)
    dev = cv.deviation(r, dense, c.pairs)
    print(name, "elimination against the dense inverse, long double", dev, "D", scs.self_deviation(name), "kappa_2", dense["kappa"], "estimate", r["kappa"], flush=True)
    assert dev <= scs.tolerance(name) / 64
    assert 0.5 * dense["kappa"] <= r["kappa"] <= 1.001 * dense["kappa"]      # the estimate comes from below
    assert scs.self_deviation(name) <= 1e-9


@pytest.mark.parametrize("defect", ["drop_term", "no_delta", "flip_fe", "truncate"])
def test_planted_defects_are_rejected(defect):
    """bal-landmark (its landmark has 68 F-neighbours: "truncate" drops four of them): each defect moves some requested block by more
    than the bound."""
    name = "bal-landmark"
    c = scs.case(name)
    bad = sr.eliminate(scs.model_coo(name), c.blocks, c.x, c.offsets, c.pairs, LD, defect=defect, order=scs.problem_order(name))
    dev = cv.deviation(bad, scs.reference(name, True), c.pairs)
    tol = scs.tolerance(name) + scs.reference(name, True)["kappa"] * 1e-11
    print(defect, dev, "bound", tol, flush=True)
    assert dev > tol
