"""Parameter bounds without a device: the setters and getters through the C ABI and api.py, the feasibility failures, and the
reference of tests/bounds_reference.py on the cases of tests/bounds_cases.py — the conditions the inputs of
tests/test_gpu_bounds.py were chosen under, and what every case is there to exercise."""
import math

import numpy as np
import pytest

import skeres_amd as sk
import step_check as sc
import bounds_reference as br
import bounds_cases as bc

INF = float("inf")


def _curve_problem():
    m, c = sk.DoubleArray(1), sk.DoubleArray(1)
    m.set(0, 0.0)
    c.set(0, 0.0)
    p = sk.Problem()
    loss = sk.PredefinedLossFunctions.trivialLoss()
    p.addResidualBlock(sk.ExponentialResidual(0.0, 1.0).toAutoDiffCostFunction(), loss, m, c)
    return p, m, c, loss


def test_c_abi_setters_and_getters_round_trip(built):
    lib = sk.lib()
    p, m, c, loss = _curve_problem()
    for v in (m, c):    # nothing set: -/+ infinity
        assert lib.sk_problem_get_parameter_lower_bound(p._h, v.cast(), 0) == -INF
        assert lib.sk_problem_get_parameter_upper_bound(p._h, v.cast(), 0) == INF
    assert lib.sk_problem_set_parameter_lower_bound(p._h, c.cast(), 0, 0.25) == 0
    assert lib.sk_problem_set_parameter_upper_bound(p._h, c.cast(), 0, 2.0) == 0
    assert lib.sk_problem_get_parameter_lower_bound(p._h, c.cast(), 0) == 0.25
    assert lib.sk_problem_get_parameter_upper_bound(p._h, c.cast(), 0) == 2.0
    assert lib.sk_problem_get_parameter_lower_bound(p._h, m.cast(), 0) == -INF     # the other block is untouched
    # -/+ infinity removes a bound
    assert lib.sk_problem_set_parameter_lower_bound(p._h, c.cast(), 0, -INF) == 0
    assert lib.sk_problem_get_parameter_lower_bound(p._h, c.cast(), 0) == -INF
    assert lib.sk_problem_get_parameter_upper_bound(p._h, c.cast(), 0) == 2.0
    assert lib.sk_problem_set_parameter_upper_bound(p._h, c.cast(), 0, INF) == 0
    assert lib.sk_problem_get_parameter_upper_bound(p._h, c.cast(), 0) == INF
    assert lib.sk_problem_set_parameter_upper_bound(p._h, m.cast(), 0, INF) == 0     # ... also where none was set


def test_c_abi_refuses_unknown_blocks_indices_and_nan(built):
    lib = sk.lib()
    p, m, c, loss = _curve_problem()
    other = sk.DoubleArray(1)
    for setter in (lib.sk_problem_set_parameter_lower_bound, lib.sk_problem_set_parameter_upper_bound):
        assert setter(p._h, other.cast(), 0, 1.0) == 1                                # SK_ERR_INVALID_ARGUMENT
        assert b"not part of the problem" in lib.sk_last_error()
        for index in (-1, 1, 9):
            assert setter(p._h, c.cast(), index, 1.0) == 1
            assert b"outside the parameter block" in lib.sk_last_error()
        assert setter(p._h, c.cast(), 0, float("nan")) == 1
        assert b"NaN" in lib.sk_last_error()
    for getter in (lib.sk_problem_get_parameter_lower_bound, lib.sk_problem_get_parameter_upper_bound):
        assert math.isnan(getter(p._h, other.cast(), 0)) and b"not part of the problem" in lib.sk_last_error()
        assert math.isnan(getter(p._h, c.cast(), 1)) and b"outside the parameter block" in lib.sk_last_error()
    assert lib.sk_problem_get_parameter_lower_bound(p._h, c.cast(), 0) == -INF       # a refused call changes nothing
    assert lib.sk_problem_get_parameter_upper_bound(p._h, c.cast(), 0) == INF


def test_bound_before_and_after_the_blocks_first_residual_block(built):
    cam, pt, late = sk.DoubleArray(9), sk.DoubleArray(3), sk.DoubleArray(3)
    p = sk.Problem()
    p.addParameterBlock(cam, 9)                      # a block without a residual block yet
    p.setParameterUpperBound(cam, 6, 1200.0)
    p.setParameterLowerBound(cam, 7, 0.0)
    loss = sk.PredefinedLossFunctions.trivialLoss()
    p.addResidualBlock(sk.SnavelyReprojectionError(0.0, 0.0).toAutoDiffCostFunction(), loss, cam, pt)
    assert p.getParameterUpperBound(cam, 6) == 1200.0 and p.getParameterLowerBound(cam, 7) == 0.0
    p.setParameterLowerBound(pt, 2, -3.0)             # a block that came with a residual block
    p.addResidualBlock(sk.SnavelyReprojectionError(1.0, 1.0).toAutoDiffCostFunction(), loss, cam, late)
    p.setParameterUpperBound(late, 0, 5.0)            # ... and one added after other blocks got their bounds
    assert p.getParameterLowerBound(pt, 2) == -3.0 and p.getParameterUpperBound(late, 0) == 5.0
    assert p.getParameterLowerBound(late, 0) == -INF and p.getParameterUpperBound(pt, 2) == INF
    assert [p.getParameterLowerBound(cam, k) for k in range(9)] == [-INF] * 7 + [0.0, -INF]


def test_api_methods(built):
    p, m, c, loss = _curve_problem()
    p.setParameterLowerBound(c, 0, 0.3)
    p.setParameterUpperBound(c, 0, 2)
    assert (p.getParameterLowerBound(c, 0), p.getParameterUpperBound(c, 0)) == (0.3, 2.0)
    assert (p.getParameterLowerBound(m, 0), p.getParameterUpperBound(m, 0)) == (-INF, INF)
    with pytest.raises(ValueError, match="outside the parameter block"):
        p.setParameterLowerBound(c, 1, 0.0)
    with pytest.raises(ValueError, match="NaN"):
        p.setParameterUpperBound(c, 0, float("nan"))
    with pytest.raises(ValueError, match="not part of the problem"):
        p.getParameterLowerBound(sk.DoubleArray(1), 0)
    names = sk.Solver.Summary().iterations.__code__.co_consts
    assert any("step_size" in str(n) for n in names) and any("line_search_evaluations" in str(n) for n in names)


def _solve(p):
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
    s = sk.Solver.Summary()
    sk.ceres.solve(o, p, s)
    return s


def test_infeasible_problems_end_in_failure_with_the_parameters_untouched(built):
    """Decided before anything touches a device: a variable block with lower >= upper, a constant block outside its bounds."""
    p, m, c, loss = _curve_problem()
    c.set(0, 0.125)
    p.setParameterLowerBound(c, 0, 1.0)
    p.setParameterUpperBound(c, 0, 1.0)
    s = _solve(p)
    assert s.terminationType() == sk.TerminationType.FAILURE
    assert "block 1, index 0" in s.message() and "lower bound" in s.message()
    assert (m.get(0), c.get(0)) == (0.0, 0.125)
    assert s.iterations() == []

    p, m, c, loss = _curve_problem()
    m.set(0, 0.5)
    p.setParameterUpperBound(m, 0, 0.25)
    p.setParameterBlockConstant(m)
    s = _solve(p)
    assert s.terminationType() == sk.TerminationType.FAILURE
    assert "block 0, index 0" in s.message() and "constant" in s.message()
    assert (m.get(0), c.get(0)) == (0.5, 0.0)

    cam, pt = sk.DoubleArray(9), sk.DoubleArray(3)    # a coordinate held by a subset parameterization
    cam.set(6, 500.0)
    p = sk.Problem()
    p.addResidualBlock(sk.SnavelyReprojectionError(0.0, 0.0).toAutoDiffCostFunction(), sk.PredefinedLossFunctions.trivialLoss(), cam, pt)
    p.setParameterization(cam, sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8]))
    p.setParameterLowerBound(cam, 6, 600.0)
    s = _solve(p)
    assert s.terminationType() == sk.TerminationType.FAILURE and "block 0, index 6" in s.message()
    assert cam.get(6) == 500.0


def test_line_search_of_the_reference_on_closed_forms():
    """phi(alpha) = (alpha - 0.25)^2 + 1 from f0 = phi(0): the quadratic through (0, f0, g0) and (1, phi(1)) IS phi, so the second
    trial is its minimiser 0.25; a phi that is not finite is bisected; a phi far above f0 takes the lower limit 1e-3 alpha."""
    phi = lambda a: (a - 0.25) ** 2 + 1.0
    alpha, value, trials, margins, unclamped = br.line_search(phi, phi(0.0), -0.5, 1.0)
    assert [t[0] for t in trials] == [1.0, 0.25] and alpha == 0.25 and value == 1.0 and unclamped == [0.25]
    alpha, _, trials, _, _ = br.line_search(lambda a: INF if a > 0.2 else phi(a), phi(0.0), -0.5, 1.0)
    assert [t[0] for t in trials] == [1.0, 0.5, 0.25, 0.125] and alpha == 0.125
    alpha, _, trials, _, unclamped = br.line_search(lambda a: 1e9 if a > 0.5 else phi(a), phi(0.0), -0.5, 1.0)
    assert [t[0] for t in trials] == [1.0, 1e-3] and alpha == 1e-3 and unclamped[0] < 1e-3
    # no descent direction: alpha = 1, one evaluation; a search that fails (phi never below f0): alpha = 1 again, evaluated once more
    assert br.line_search(phi, phi(0.0), 0.5, 1.0)[0] == 1.0 and len(br.line_search(phi, phi(0.0), 0.5, 1.0)[2]) == 1
    alpha, _, trials, _, _ = br.line_search(lambda a: 2.0 + a, 2.0, -1.0, 1e12)
    assert alpha == 1.0 and len(trials) == 22 and trials[-1][0] == 1.0
    alpha, _, trials, _, _ = br.line_search(lambda a: 2.0 + a, 2.0, -1.0, 1e-9)     # the minimum step size: alpha max |delta| < 1e-9
    assert alpha == 1.0 and len(trials) == 1


@pytest.mark.parametrize("name", bc.ALL)
def test_cases_satisfy_the_conditions_they_were_chosen_under(built, name):
    """Double and long double take the same decision at every trial of every iteration and agree ten times inside the device
    tolerances on every compared field; every Armijo test is decided by a margin of at least 1e-6 of f0; every alpha has the same
    bits whatever the rounding of phi (tests/bounds_cases.py: violations)."""
    sc._require_long_double()
    assert bc.violations(name) == []
    # feasible as the solver judges it: every held coordinate inside its bounds, lower < upper everywhere else
    if name in bc.CASES:
        x0, (lo, hi), free = bc.problem(name).parameters, bc.box(name), bc.model(name).free
    else:
        (_, _, x0, lo, hi, _), free = bc.dense_problem(name), bc.dense_model(name).free
    assert np.all((x0 >= lo) & (x0 <= hi) | free) and np.all(lo < hi)
    assert all(e["step_is_valid"] for e in bc.any_reference(name)[1])


def test_what_the_cases_are_there_to_exercise(built):
    ref = {name: bc.any_reference(name) for name in bc.ALL}
    # wide bounds: the log of the unbounded loop, bit for bit — but for the gradient norm, where x - (x - g) is g rounded at the
    # magnitude of x (focal lengths of 1e3 against gradients of 1 to 1e3: a few units of 1e-13)
    unbounded = bc.reference("small-inactive", unbounded=True)[1]
    assert len(unbounded) == len(ref["small-inactive"][1])
    for a, b in zip(ref["small-inactive"][1], unbounded):
        assert all(a[f] == b[f] for f in list(bc.TOL) + ["step_size", "line_search_evaluations", "step_is_successful"] if f != "gradient_max_norm")
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-12 * b["gradient_max_norm"]
        assert a["step_size"] == 1.0 and a["active_bounds"] == 0
    # an infeasible start: x0 outside the box, the projected point inside, its cost the initial cost
    for name in ("small-infeasible-start", "tape"):
        prob, (lo, hi) = bc.problem(name), bc.box(name)
        x0 = prob.parameters
        outside = (x0 < lo) | (x0 > hi)
        assert outside[:9 * prob.num_cameras].sum() == 2 and outside[9 * prob.num_cameras:].sum() == 5
        start = bc.reference(name, kmax=0)
        assert np.array_equal(start[0], br.project(x0, lo, hi)) and len(start[1]) == 1
        assert start[1][0]["active_bounds"] == 7 and start[1][0]["cost"] == ref[name][1][0]["cost"]
        assert sum(e["step_is_successful"] for e in ref[name][1][1:]) >= 3
    # active focal bounds at the end
    for name in ("active-intrinsics", "plans-retained", "plans-jacobi-off"):
        x, log = ref[name]
        lo, hi = bc.box(name)
        C = bc.problem(name).num_cameras
        f = 9 * np.arange(C) + 6
        assert log[-1]["active_bounds"] > 0 and np.sum(x[f] == hi[f]) == np.sum(np.isfinite(hi[f])) == len(range(2, C, 3))
    assert np.sum(ref["active-intrinsics"][0][9 * np.arange(16) + 7] == 0.0) > 0          # k1 >= 0 binds too
    # the retained plan's candidates and an eliminated point are boxed
    prob = bc.problem("plans-retained")
    lo, hi = bc.box("plans-retained")
    boxed = [q for q in range(prob.num_points) if np.isfinite(lo[9 * prob.num_cameras + 3 * q])]
    assert sorted(boxed) == sorted(bc.widest_tracks(prob, 4) + [7])
    # contraction: alpha < 1 in a bundle-adjustment case; trials whose cost is not finite on the dense path
    assert sum(e["step_size"] < 1.0 for e in ref["contracting"][1]) >= 2
    assert all(e["step_size"] == 1e-3 and e["line_search_evaluations"] == 2 for e in ref["contracting"][1] if e["step_size"] < 1.0)
    over = ref["curve-fitting-overflow"][1]
    assert sum(not np.isfinite(t[1]) for t in over[1]["trials"]) == 8 and over[1]["step_size"] == 2.0 ** -8 and over[1]["step_is_successful"]
    assert over[2]["step_size"] == 1e-3
    # the robust case: bounds on free coordinates only, some of them active
    free = bc.model("robust-subset").free
    lo, hi = bc.box("robust-subset")
    assert not np.any(np.isfinite(lo[~free]) | np.isfinite(hi[~free])) and ref["robust-subset"][1][-1]["active_bounds"] > 0
    # the dense path
    x, log = ref["hello-world"]
    assert x[0] == 7.0 and log[-1]["cost"] == 4.5 and log[-1]["gradient_max_norm"] == 0.0 and log[-1]["active_bounds"] == 1
    x, log = ref["powell"]
    assert x[0] == 0.5 and x[3] == 0.25 and log[-1]["active_bounds"] == 3
    x, log = ref["curve-fitting"]
    assert x[1] == 0.3 and all(e["active_bounds"] == 1 for e in log)
    assert (~bc.dense_model("dense-tangent").free).sum() == 2 * 9 + 4 * 3 and ref["dense-tangent"][1][0]["active_bounds"] == 7
