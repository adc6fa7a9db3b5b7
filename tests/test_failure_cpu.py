"""The failure-path reference (tests/failure_reference.py) and its cases (tests/failure_cases.py), on the CPU: the reference agrees
with itself in double and long double on every discrete field of every case and reaches the branch the case is there for; no
decision of a case is borderline; the reference reproduces oracle/lm.cpp where the oracle can express the case; and the comparison
that tests/test_gpu_failure.py holds the device to rejects planted defects."""
import copy

import numpy as np
import pytest

import oracle
import failure_cases as fc
import failure_reference as fr
from helpers import curve_fitting_data

REFERENCED = [n for n in fc.names() if fc.CASES[n].get("reference_of", n) == n]
MARGIN = 0.1          # of the step length: how far a candidate lands from its barrier
RHO_MARGIN = 0.05     # how far a decisive relative decrease stays from min_relative_decrease


@pytest.fixture(scope="module", autouse=True)
def _oracle(built):
    return built


@pytest.mark.parametrize("name", REFERENCED)
def test_double_and_long_double_agree_and_reach_the_branch(name):
    d, ld = fc.reference(name), fc.reference(name, True)
    assert fr.discrete(d) == fr.discrete(ld)
    assert d["reached"] == ld["reached"]
    assert fc.CASES[name]["reach"] <= d["reached"], (fc.CASES[name]["reach"], d["reached"])
    assert set(d["reached"]) <= set(fr.BRANCHES)
    for a, b in zip(d["log"], ld["log"]):   # the two trajectories are one: ten times inside what the device is held to
        assert abs(a["cost"] - b["cost"]) <= 0.1 * fc.TOL["cost"] * abs(b["cost"])
        assert a["radius_exact"] == b["radius_exact"]
        if a["radius_exact"]:
            assert a["trust_region_radius"] == b["trust_region_radius"]   # bitwise
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 0.1 * fc.TOL_RADIUS_ROUNDED * b["trust_region_radius"]
    if fc.CASES[name]["kind"] in "abg" and name != "a-rows-inf":
        assert d["termination"] == fr.FAILURE and d["message"] == fr.MSG_INITIAL and not d["log"]
        assert np.array_equal(fc.bits(d["x"]), fc.bits(fc.start(name)))
    if fc.CASES[name].get("converges"):
        assert d["termination"] == fr.CONVERGENCE
    if fc.CASES[name]["kind"] == "e":
        assert d["termination"] == fr.FAILURE and d["message"] == fr.MSG_EVALUATION and d["final_cost"] is None
        assert d["num_successful_steps"] == 1 and len(d["log"]) == 2   # the second accepted step is neither counted nor logged
        assert not np.array_equal(d["x"], d["log"][1]["candidate"])    # ... and its point is the one returned


@pytest.mark.parametrize("name", [n for n in REFERENCED if "barrier" in fc.CASES[n]])
def test_no_decision_is_borderline(name):
    c = fc.CASES[name]
    for long_double in (False, True):
        run = fc.reference(name, long_double)
        m = fc.margins(name, run)
        print(name, "long double" if long_double else "double", [(k, round(float(v), 3), f) for k, v, f in m], flush=True)
        for k, v, failed in m:
            assert (v <= -MARGIN) if failed else (v >= MARGIN), (k, v, failed)
        if c.get("failed_candidates") is not None:   # the first candidates fail, then one is accepted
            assert [f for _, _, f in m][:c["failed_candidates"] + 1] == [True] * c["failed_candidates"] + [False]
            assert run["log"][c["failed_candidates"] + 1]["step_is_successful"]
            for e in run["log"][1:c["failed_candidates"] + 1]:
                assert e["step_is_valid"] and e["cost_change"] == e["cost"] - fr.DBL_MAX
        decided = [e for e in run["log"][1:] if e["step_is_valid"] and not e["candidate_failed"] and e["relative_decrease"] != 0.0]
        assert decided
        for e in decided:
            assert abs(e["relative_decrease"] - 1e-3) >= RHO_MARGIN, e["relative_decrease"]


@pytest.mark.parametrize("name", fc.names(kind="f"))
def test_radius_recurrence_of_invalid_steps(name):
    run = fc.reference(name)
    limit = fc.options(name).get("max_num_consecutive_invalid_steps", 5)
    r0 = 1e4
    want = [r0, r0 / 2, r0 / 8, r0 / 64, r0 / 1024][:limit]
    want.append(want[-1])   # the step that ends the solve leaves the radius alone
    assert [e["trust_region_radius"] for e in run["log"]] == want
    assert run["message"] == fr.MSG_INVALID % limit and run["num_unsuccessful_steps"] == 0
    assert np.array_equal(fc.bits(run["x"]), fc.bits(fc.start(name)))
    # the overflow is there: a Jacobian entry of 1e160 beside a finite cost and a finite gradient
    assert run["log"][0]["cost"] < 1e6 and np.isfinite(run["log"][0]["gradient_max_norm"])
    assert max(float(np.max(np.abs(J))) for _, terms in fc.model(name).chunks(fc.start(name)) for J, _ in terms) == fc.BIG


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against oracle/lm.cpp
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_run(x, s, x0):
    names = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_valid", "step_is_successful")
    log = [{nm: getattr(s.iterations[i], nm) for nm in names} for i in range(s.num_logged)]
    return dict(x=np.asarray(x), log=log, termination={oracle.CONVERGENCE: fr.CONVERGENCE, oracle.NO_CONVERGENCE: fr.NO_CONVERGENCE, oracle.FAILURE: fr.FAILURE}[s.termination_type],
                message=s.message.decode(), num_successful_steps=s.num_successful_steps, num_unsuccessful_steps=s.num_unsuccessful_steps,
                final_cost=s.final_cost if s.num_logged else float("nan"))


@pytest.mark.parametrize("name", fc.names(kind="a", backend="DENSE_QR") + fc.names(kind="a", backend="DENSE_SCHUR"))
def test_oracle_on_case_a(name):
    x0 = fc.start(name)
    if fc.CASES[name]["backend"] == "DENSE_QR":
        x, s = oracle.solve([1, 1], x0, [(oracle.EXPONENTIAL, [xv, yv], [0, 1]) for xv, yv in curve_fitting_data()])
    else:
        prob = fc._prob(fc.CASES[name])
        x, s = oracle.solve_bal(prob.num_cameras, prob.num_points, prob.camera_index, prob.point_index, prob.observations, x0)
    fc.compare(_oracle_run(x, s, x0), fc.reference(name), x0, show=name)


@pytest.mark.parametrize("x0", [(0.0, 0.0), (-3.0, 8.0)])
def test_oracle_on_curve_fitting_with_rejected_steps(x0):
    """The oracle has no compiled functor with a barrier (case c cannot be expressed through oracle.solve); what it can express
    of the loop beyond case a is a trajectory with rejected steps: EX/CurveFitting.scala from (0, 0) rejects five candidates."""
    x0 = np.array(x0)
    data = curve_fitting_data()
    x, s = oracle.solve([1, 1], x0, [(oracle.EXPONENTIAL, [xv, yv], [0, 1]) for xv, yv in data])
    ref = fr.solve(fr.CallableModel(2, [(fc._exponential_host(xv, yv), [0, 1], [1, 1]) for xv, yv in data]), x0)
    if x0[0] == 0.0:
        assert "rejected" in ref["reached"] and ref["num_unsuccessful_steps"] >= 5
    # (The oracle sums in another order than numpy, and this problem's trajectories drift apart — the costs by 5e-13 at the eighth iteration
    # from (-3, 8), a rejected-then-accepted region where rho is 0.11 — so the radius behind an unclamped update is held to the project's
    # tolerance for oracle comparisons, as the dogleg tests hold it; the device cases are held to fc.TOL_RADIUS_ROUNDED.)
    fc.compare(_oracle_run(x, s, x0), ref, x0, show="curve-fitting", tol_radius_rounded=fc.TOL["trust_region_radius"])


# ---------------------------------------------------------------------------------------------------------------------------
# planted defects: the comparison must reject each
# ---------------------------------------------------------------------------------------------------------------------------
def _as_device(ref, name):
    run = copy.deepcopy({k: v for k, v in ref.items() if k != "reached"})
    run["reached"] = ref["reached"]
    run["final_cost"] = ref["final_cost"] if ref["final_cost"] is not None else float("nan")
    xs, x = [fc.start(name)], fc.start(name)
    for e in run["log"][1:]:
        x = e["candidate"] if e["step_is_successful"] else x
        xs.append(x)
    run["xs"] = xs
    return run


def _failed_as_invalid(run):
    for e in run["log"]:
        if e.get("candidate_failed"):
            e.update(step_is_valid=0, cost_change=0.0, step_norm=0.0, relative_decrease=0.0)


def _radius_kept(run):
    for k, e in enumerate(run["log"]):
        if e.get("candidate_failed"):
            e["trust_region_radius"] = run["log"][k - 1]["trust_region_radius"]


def _flag_stays_set(run):
    k = max(k for k, e in enumerate(run["log"]) if e.get("candidate_failed")) + 1
    run["log"][k].update(step_is_valid=0, step_is_successful=0, cost_change=0.0, step_norm=0.0, relative_decrease=0.0)


def _slightly_wrong_radius(run):
    run["log"][-1]["trust_region_radius"] *= 1 + 1e-13


PLANTED = {
    "a failed candidate counted as an invalid step": ("c-DENSE_QR", _failed_as_invalid),
    "the radius not reduced after a failed candidate": ("c-DENSE_QR", _radius_kept),
    "a failure flag that stays set for the following step": ("c-DENSE_QR", _flag_stays_set),
    "a failed candidate counted as an invalid step (DENSE_SCHUR)": ("c-DENSE_SCHUR", _failed_as_invalid),
    "a radius off by 1e-13": ("c-DENSE_QR", _slightly_wrong_radius),
}


@pytest.mark.parametrize("defect", sorted(PLANTED))
def test_planted_defect_in_the_log_is_rejected(defect):
    name, plant = PLANTED[defect]
    ref = fc.reference(name)
    run = _as_device(ref, name)
    fc.compare(run, ref, fc.start(name))   # unharmed, it passes
    plant(run)
    with pytest.raises(AssertionError):
        fc.compare(run, ref, fc.start(name))


# ---------------------------------------------------------------------------------------------------------------------------
# case i: invalid linear solves followed by valid ones (the silent co-axial component of tests/failure_cases.py)
# ---------------------------------------------------------------------------------------------------------------------------
I_REFERENCED = [n for n in fc.names(kind="i") if fc.CASES[n]["reference_of"] == n]
QUOTIENT_MARGIN = 0.05   # how far min_lm_diagonal / radius stays from 2^-1075 wherever the radius carries a rounding


def episodes(log):
    """[(first, last)] of the runs of consecutive invalid entries of a log."""
    out, k = [], 1
    while k < len(log):
        if not log[k]["step_is_valid"]:
            first = k
            while k + 1 < len(log) and not log[k + 1]["step_is_valid"]:
                k += 1
            out.append((first, k))
        k += 1
    return out


@pytest.mark.parametrize("name", I_REFERENCED)
def test_i_the_silent_component_is_what_the_case_says(name):
    """The oracle's Jacobian at x0: the on-axis points' z columns, and no others, are exactly zero (so no camera column is), and
    the residuals of the component's own points are exactly zero, with them (where the component has no generic point) its gradient."""
    c, comp = fc.CASES[name], fc.component(name)
    prob, x0 = fc._prob(c), fc.start(name)
    n = prob.num_parameters
    colsq, grad = np.zeros(n, dtype=fc.LD), np.zeros(n, dtype=fc.LD)
    own = np.isin(prob.point_index, comp["on_axis"] + comp["off_axis"])
    assert own.sum() == 2 * len(comp["on_axis"] + comp["off_axis"]) and set(prob.camera_index[own]) == set(comp["cameras"])
    at = 0
    for r, terms in fc.model(name).chunks(x0):
        assert not np.any(r[own[at:at + len(r)]])   # exactly zero, whatever the loss
        at += len(r)
        for J, first in terms:
            for b in range(J.shape[0]):
                colsq[first[b]:first[b] + J.shape[2]] += np.sum(J[b] * J[b], axis=0)
                grad[first[b]:first[b] + J.shape[2]] += J[b].T @ r[b]
    assert sorted(np.flatnonzero(colsq == 0).tolist()) == sorted(comp["zero_columns"])
    assert np.all(colsq[:9 * prob.num_cameras] > 0)
    if not c.get("generic"):
        assert not np.any(grad[comp["columns"]])
        assert not np.any(np.isin(prob.camera_index[~own], comp["cameras"]))


@pytest.mark.parametrize("name", I_REFERENCED)
def test_i_every_decision_of_the_quotient_is_exact_or_far(name):
    c = fc.CASES[name]
    comp = fc.component(name)
    for long_double in (False, True):
        run = fc.reference(name, long_double)
        log = run["log"]
        print(name, "long double" if long_double else "double",
              [(k, e["radius_used"] / fc.R_STAR, e["radius_used_exact"], round(e["zero_quotient_over_half_ulp"], 4), e["zero_columns"]) for k, e in enumerate(log) if k], flush=True)
        for k, e in enumerate(log[1:], 1):
            underflows = e["zero_quotient"] == 0.0
            assert underflows == (e["zero_quotient_over_half_ulp"] <= 1.0)   # (ties to even: 2^-1075 itself rounds to 0)
            if e["radius_used_exact"]:   # a radius reached by powers of two and by x 3: the same bits on the device, the decision exact
                assert e["radius_used"] == log[k - 1]["trust_region_radius"] and log[k - 1]["radius_exact"]
            else:
                assert abs(e["zero_quotient_over_half_ulp"] - 1.0) >= QUOTIENT_MARGIN, (k, e["zero_quotient_over_half_ulp"])
            # the quotient alone decides: no solve of these cases is invalid for another reason
            assert bool(e["step_is_valid"]) == (not (e["zero_columns"] and underflows)), k
            if e["step_is_valid"] and e["relative_decrease"] != 0.0:
                assert abs(e["relative_decrease"] - 1e-3) >= RHO_MARGIN, (k, e["relative_decrease"])
        ep = episodes(log)
        assert len(ep) >= c["episodes"] and (c["episodes"] != 1 or (len(ep) == 1 and ep[0][0] == 1)), ep
        assert ep[0][0] == 1 and ep[0][1] >= 2   # at least two invalid solves at iteration 1
        for first, last in ep:
            assert last + 1 < len(log) and log[last + 1]["step_is_valid"] and log[last + 1]["step_is_successful"], (first, last)
        if c["episodes"] > 1:
            accepted_before = [sum(int(e["step_is_successful"]) for e in log[1:first]) for first, _ in ep]
            assert {a % 2 for a in accepted_before} == {0, 1}, accepted_before   # both parities of the replayed graph
            assert log[1]["zero_columns"] == log[-1]["zero_columns"] == len(comp["zero_columns"])   # the zero columns persist
            x = run["x"]
            assert np.array_equal(fc.bits(x[comp["columns"]]), fc.bits(fc.start(name)[comp["columns"]]))   # the component never moves
        else:
            assert log[-1]["zero_columns"] == 0   # its cameras moved with the first accepted step


def _invalid_moved_by_an_ulp(run):
    k = next(k for k, e in enumerate(run["log"]) if not e["step_is_valid"])
    run["xs"][k] = run["xs"][k].copy()
    run["xs"][k][7] = np.nextafter(run["xs"][k][7], np.inf)


def _invalid_entry_missing(run):
    k = next(k for k, e in enumerate(run["log"]) if not e["step_is_valid"])
    del run["log"][k]
    del run["xs"][k]


@pytest.mark.parametrize("defect", ["an invalid iteration that moved x by one ulp", "a log with one invalid entry missing"])
def test_i_planted_defect_in_the_log_is_rejected(defect):
    name = "i-once"
    ref = fc.reference(name)
    run = _as_device(ref, name)
    fc.compare(run, ref, fc.start(name))
    (_invalid_moved_by_an_ulp if "ulp" in defect else _invalid_entry_missing)(run)
    with pytest.raises(AssertionError):
        fc.compare(run, ref, fc.start(name))


def _recovery_step(name, radius, stale=None):
    """The step of case `name` from x0 at `radius` through the Schur complement of the dense normal equations, in double: x0 - s y.
    stale: (camera a, camera b, 9 x 9 block) added to S[a, b] and its transpose to S[b, a] before the reduced solve."""
    import step_check as sc
    c = fc.CASES[name]
    prob, x0, model = fc._prob(c), fc.start(name), fc.model(name)
    n, nc = prob.num_parameters, 9 * prob.num_cameras
    s = np.asarray(sc.jacobi_scale(model, x0), dtype=np.float64)
    rows = []
    res = []
    for r, terms in model.chunks(x0):
        for b in range(r.shape[0]):
            row = np.zeros((r.shape[1], n))
            for J, first in terms:
                row[:, first[b]:first[b] + J.shape[2]] = np.asarray(J[b], dtype=np.float64)
            rows.append(row * s)
            res.append(np.asarray(r[b], dtype=np.float64))
    J, r = np.concatenate(rows), np.concatenate(res)
    colsq = np.sum(J * J, axis=0)
    D2 = np.clip(colsq, c["options"]["min_lm_diagonal"], 1e32) / radius
    D2[colsq == 0] = 1.0   # (y_j = 0 under any positive diagonal)
    A, g = J.T @ J + np.diag(D2), J.T @ r
    App_inv = np.linalg.inv(A[nc:, nc:])
    S = A[:nc, :nc] - A[:nc, nc:] @ App_inv @ A[nc:, :nc]
    if stale is not None:
        a, b, block = stale
        S[9 * a:9 * a + 9, 9 * b:9 * b + 9] += block
        S[9 * b:9 * b + 9, 9 * a:9 * a + 9] += block.T
    yc = np.linalg.solve(S, g[:nc] - A[:nc, nc:] @ App_inv @ g[nc:])
    yp = App_inv @ (g[nc:] - A[nc:, :nc] @ yc)
    return x0 - s * np.concatenate([yc, yp]), S


@pytest.mark.parametrize("defect", ["none", "the previous radius's diagonal", "a stale block in S"])
def test_i_planted_defect_in_the_recovery_step_is_rejected(defect):
    """The step check that tests/test_gpu_failure.py holds the first valid step after an episode to: it passes a step computed
    from the system of the recovery radius, and rejects one computed with the diagonal of the radius before (the last invalid
    solve's) or from an S in which a block that should be zero kept an earlier assembly's entries."""
    import step_check as sc
    name = "i-once"
    ref, x0 = fc.reference(name), fc.start(name)
    k = episodes(ref["log"])[0][1] + 1
    radius, previous = ref["log"][k - 1]["trust_region_radius"], ref["log"][k - 2]["trust_region_radius"]
    assert previous == 4 * radius
    stale = None
    if defect.startswith("a stale"):
        _, S = _recovery_step(name, radius)
        comp = fc.component(name)
        a, b = 0, comp["cameras"][0]   # two cameras that share no point: their block of S is zero
        assert not np.any(S[9 * a:9 * a + 9, 9 * b:9 * b + 9])
        stale = (a, b, S[9:18, 0:9].copy())   # what the block of cameras (1, 0) holds
    x1, _ = _recovery_step(name, previous if defect.startswith("the previous") else radius, stale)
    kw = dict(min_lm_diagonal=fc.CASES[name]["options"]["min_lm_diagonal"])
    if defect == "none":
        print(sc.check(fc.model(name), x0, x0, x1, ref["log"], k, **kw))
        return
    with pytest.raises(AssertionError):
        sc.check(fc.model(name), x0, x0, x1, ref["log"], k, **kw)


def test_nan_dropped_from_the_gradient_norm_is_rejected():
    """What a device that reduces max |g| with fmax makes of case g: the evaluation passes for finite, the NaN reaches the
    factorisation, five invalid steps, FAILURE.  The invariants hold; the comparison still rejects the run."""
    name = "g-DENSE_QR-recorded"
    ref, x0 = fc.reference(name), fc.start(name)
    entry = dict(cost=1.0, cost_change=0.0, gradient_max_norm=3.0, step_norm=0.0, relative_decrease=0.0, trust_region_radius=1e4, step_is_valid=1, step_is_successful=1)
    log = [entry] + [dict(entry, step_is_valid=0, step_is_successful=0, trust_region_radius=r) for r in (5e3, 1250.0, 156.25, 9.765625, 9.765625)]
    run = dict(x=x0.copy(), xs=[x0.copy()] * 6, log=log, termination=fr.FAILURE, message=fr.MSG_INVALID % 5, num_successful_steps=0, num_unsuccessful_steps=0, final_cost=1.0)
    with pytest.raises(AssertionError):
        fc.compare(run, ref, x0)
    run = dict(x=x0.copy(), xs=[x0.copy()], log=[], termination=fr.FAILURE, message=fr.MSG_INITIAL, num_successful_steps=0, num_unsuccessful_steps=0, final_cost=float("nan"))
    fc.compare(run, ref, x0)   # the exact outcome


@pytest.mark.parametrize("defect", ["the pre-step point not restored on FAILURE", "a non-finite value written back", "CONVERGENCE where the reference fails"])
def test_planted_defect_in_what_is_written_back_is_rejected(defect):
    name = "f-DENSE_QR-n3"
    ref, x0 = fc.reference(name), fc.start(name)
    run = _as_device({k: (v if k != "log" else [dict(e) for e in v]) for k, v in ref.items()}, name)
    run["xs"] = [x0.copy() for _ in run["log"]]
    fc.compare(run, ref, x0)
    if defect.startswith("the pre-step"):
        run["x"] = np.nextafter(x0, 2.0)
    elif defect.startswith("a non-finite"):
        run["x"] = x0.copy()
        run["x"][1] = np.nan
    else:
        run["termination"] = fr.CONVERGENCE
    with pytest.raises(AssertionError):
        fc.compare(run, ref, x0)


def test_nan_is_compared_by_its_bits():
    name = "a-DENSE_QR-nan"
    ref, x0 = fc.reference(name), fc.start(name)
    run = dict(x=x0.copy(), xs=[x0.copy()], log=[], termination=fr.FAILURE, message=fr.MSG_INITIAL, num_successful_steps=0, num_unsuccessful_steps=0, final_cost=float("nan"))
    fc.compare(run, ref, x0)
    run["x"] = x0.copy()
    run["x"].view(np.uint64)[0] ^= np.uint64(1)   # another NaN
    assert np.isnan(run["x"][0])
    with pytest.raises(AssertionError):
        fc.compare(run, ref, x0)
