"""DOGLEG without a device: the option setters through the C ABI, and the reference of tests/dogleg_reference.py on the cases of
tests/dogleg_cases.py — where the inputs of tests/test_gpu_dogleg.py were chosen."""
import numpy as np
import pytest

import oracle
import skeres_amd as sk
import step_check as sc
import dogleg_reference as dr
import dogleg_cases as dc


def test_option_setters_through_the_c_abi(built):
    lib = sk.lib()
    o = sk.Solver.Options()
    assert o.trustRegionStrategyType() == sk.TrustRegionStrategyType.LEVENBERG_MARQUARDT == 0   # the default
    assert o.doglegType() == sk.DoglegType.TRADITIONAL_DOGLEG == 0
    for v in (sk.TrustRegionStrategyType.DOGLEG, 1, sk.TrustRegionStrategyType.LEVENBERG_MARQUARDT):
        assert lib.sk_options_set_trust_region_strategy_type(o._h, v) == 0
        assert o.trustRegionStrategyType() == v
    for v in (sk.DoglegType.SUBSPACE_DOGLEG, sk.DoglegType.TRADITIONAL_DOGLEG):
        assert lib.sk_options_set_dogleg_type(o._h, v) == 0
        assert o.doglegType() == v
    for v in (-1, 2, 7):
        assert lib.sk_options_set_trust_region_strategy_type(o._h, v) == 1   # SK_ERR_INVALID_ARGUMENT
        assert b"trust region strategy" in lib.sk_last_error()
        assert lib.sk_options_set_dogleg_type(o._h, v) == 1
        with pytest.raises(ValueError):
            o.setTrustRegionStrategyType(v)
        with pytest.raises(ValueError):
            o.setDoglegType(v)
    assert o.trustRegionStrategyType() == 0 and o.doglegType() == 0         # a refused value changes nothing
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    o.setDoglegType(sk.DoglegType.TRADITIONAL_DOGLEG)
    assert o.trustRegionStrategyType() == 1


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_double_and_long_double_references_agree_ten_times_inside_the_tolerances(built, name):
    sc._require_long_double()
    kmax = dc.CASES[name]["kmax"]
    _, log = dc.reference(name)
    _, log_ld = dc.reference(name, True)
    dc.compare_logs(log, log_ld, kmax, factor=0.1)
    assert all(e["step_is_valid"] for e in log)


@pytest.mark.parametrize("name", sorted(dc.DENSE_CASES))
def test_dense_references_agree_ten_times_inside_the_tolerances(built, name):
    kmax = dc.DENSE_CASES[name]["kmax"]
    log, log_ld = dc.dense_reference(name)[1], dc.dense_reference(name, True)[1]
    dc.compare_logs(log, log_ld, kmax, factor=0.1)
    if name == "curve-fitting":
        assert [bool(e["step_is_successful"]) for e in log[1:]] == [False] * 11 + [True] * 3
        assert [bool(e["reused"]) for e in log[1:]] == [False] + [True] * 11 + [False] * 2
        assert log[11]["branch"] == log[12]["branch"] == "cauchy" and log[1]["branch"] == "gn"
    else:
        assert all(e["step_is_successful"] and e["branch"] == "gn" for e in log[1:])


def _branches(name):
    return [e.get("branch") for e in dc.reference(name)[1][1:]]


def test_the_cases_take_every_branch_and_a_rejection_followed_by_an_acceptance(built):
    """A case that stops exercising what it is there for fails here."""
    taken = set()
    for name in dc.CASES:
        taken |= set(_branches(name))
    assert {"gn", "cauchy", "interpolated"} <= taken, taken
    assert set(_branches("small")) == {"gn"}
    assert "cauchy" in _branches("small-radius-1") and "interpolated" in _branches("small-radius-1")
    for name in ("plans", "plans-jacobi-off", "robust"):
        assert set(_branches(name)) == {"gn"}
    # from radius 1: retained points, Jacobi scaling off and held coordinates under truncated Cauchy and interpolated steps
    assert _branches("plans-radius-1") == _branches("plans-jacobi-off-radius-1") == ["cauchy"] * 5 + ["interpolated"]
    assert _branches("robust-radius-1") == ["cauchy"] * 5 + ["interpolated", "gn"]
    for name in ("plans-radius-1", "plans-jacobi-off-radius-1", "robust-radius-1"):
        assert all(e["step_is_successful"] for e in dc.reference(name)[1])
    # with Jacobi scaling off diag is far from 1 and spread over three decades (with it: 0.53 to 1)
    model = dc.model("plans-jacobi-off-radius-1")
    diag = np.sqrt(sc._column_sq_norms(model, dc.problem("plans-jacobi-off-radius-1").parameters))[model.free]
    assert diag.min() > 1 and diag.max() > 1e3 * diag.min()
    log = dc.reference("rejecting")[1]
    assert [bool(e["step_is_successful"]) for e in log[1:]] == [True, True, True, True, False, False, True]
    assert [bool(e["reused"]) for e in log[1:]] == [False, False, False, False, False, True, True]
    assert log[7]["branch"] == "interpolated" and log[5]["branch"] == "gn"
    # the radius halves at every rejection, and a reused step keeps its Jacobian's scalars
    assert log[5]["trust_region_radius"] == 0.5 * log[4]["trust_region_radius"] and log[6]["trust_region_radius"] == 0.5 * log[5]["trust_region_radius"]
    assert log[5]["g_g"] == log[6]["g_g"] == log[7]["g_g"]
    # held coordinates of the robust case never move
    for name in ("robust", "robust-radius-1"):
        x, _ = dc.reference(name)
        free = dc.model(name).free
        assert np.array_equal(x[~free], dc.problem(name).parameters[~free]) and (~free).sum() == 18 + 3 * 14 + 3


@pytest.mark.parametrize("name", ["small-radius-1", "rejecting", "plans-radius-1", "plans-jacobi-off-radius-1", "robust-radius-1"])
def test_cauchy_identity_and_model_cost_change_of_the_reference(built, name):
    """In long double: w . r = -|g_hat|^2, and the model cost change as the quadratic in (a, b) over the five products equals
    -m . (r + m / 2) formed from the step itself."""
    sc._require_long_double()
    for e in dc.reference(name, True)[1][1:]:
        assert abs(e["w_r"] + e["g_g"]) <= 1e-12 * e["g_g"], (name, e["w_r"], e["g_g"])
        a, b = np.longdouble(e["a"]), np.longdouble(e["b"])
        w_r, m_r, w_w, w_m, m_m = e["products"]
        quadratic = -(a * w_r + b * m_r + (a * a * w_w + 2 * a * b * w_m + b * b * m_m) / 2)
        want = e["model_cost_change_ld"]
        assert want > 0 and abs(quadratic - want) <= 1e-10 * want, (name, e["branch"], float(quadratic), float(want))


def test_powell_reaches_its_minimum(built):
    """EX/Powell.scala's problem under the reference: cost below 1e-20."""
    blocks = [(oracle.POWELL_F1, [], [0, 1], None), (oracle.POWELL_F2, [], [2, 3], None), (oracle.POWELL_F3, [], [1, 2], None),
              (oracle.POWELL_F4, [], [0, 3], None)]
    model = sc.BlocksModel([1, 1, 1, 1], blocks)
    x0 = np.array([3.0, -1.0, 0.0, 1.0])
    for dtype in (np.float64, np.longdouble):
        x, log = dr.solve(model, dr.blocks_cost(model), x0, dict(max_num_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0,
                                                                  gradient_tolerance=1e-30), dtype=dtype)
        assert log[-1]["cost"] < 1e-20, log[-1]["cost"]


def test_i_dogleg_reaches_the_mu_loop(built):
    """No other case of tests/dogleg_cases.py takes a second turn of `mu *= 10 while the damped system is not positive definite`
    (asserted here); i-dogleg takes five at iteration 1 and one each at iterations 2 and 4, in double and in long double alike, every
    decision of the quotient at least 15 % from 2^-1075, the silent component's columns exactly zero and its gradient exactly zero."""
    for other in sorted(set(dc.CASES) - {"i-dogleg"}):
        assert all(e.get("solves", 1) <= 1 for e in dc.reference(other)[1]), other
    c = dc.CASES["i-dogleg"]
    prob, cols = dc.silent_component("i-dogleg")
    for long_double in (False, True):
        x, log = dc.reference("i-dogleg", long_double)
        assert [e["solves"] for e in log[1:]] == list(c["solves"])
        for e, mu in zip(log[1:], c["mus"]):
            assert e["step_is_valid"] and e["step_is_successful"] and not e["reused"]
            *failed, held = e["quotients"]
            assert held[0] == pytest.approx(mu, rel=1e-12) and held[1] > 0.0 and held[2] >= 1.15 and held[3] == 3
            for _, quotient, over_half_ulp, zero_columns in failed:
                assert quotient == 0.0 and over_half_ulp <= 0.85 and zero_columns == 3
        assert np.array_equal(x[cols].view(np.uint64), prob.parameters[cols].view(np.uint64))   # the component never moves
    assert dc.model("i-dogleg").free.all()   # no inert coordinate
