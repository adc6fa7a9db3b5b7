"""CGNR with the Schur elimination, without a device: the option and its default, the elimination that sk_cgnr_elimination_plan
reports from host data against the reference's own greedy set (tests/cgnr_schur_reference.py) and against
sk_covariance_elimination_plan, the conditions under which the cases of tests/cgnr_schur_cases.py were chosen, the gain in CG
iterations over tests/cgnr_reference.py, and three planted defects that the device comparison must reject."""
import ctypes as C

import numpy as np
import pytest

import skeres_amd as sk
import cgnr_reference as cr
import cgnr_cases as cc
import cgnr_schur_cases as k

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_option_validation_and_default():
    lib = sk.api.lib()
    assert lib.sk_options_set_schur_elimination(None, 1) == 1          # SK_ERR_INVALID_ARGUMENT
    o = sk.Solver.Options()
    for on in (True, False, 1, 0, 7):
        o.setSchurElimination(on)
    # (the default, off, and that the option changes nothing under another solver type show on the device: tests/test_gpu_cgnr_schur.py)
    problem, params, _, keep = k.build_device("bal-small")
    n = C.c_int(-1)
    assert lib.sk_cgnr_elimination_plan(None, None, None, None, None, None) == 1
    assert lib.sk_cgnr_elimination_plan(problem._h, None, C.byref(n), None, None, None) == 0 and n.value == 40   # every output may be NULL
    assert lib.sk_cgnr_elimination_plan(problem._h, None, None, None, None, None) == 0
    # the names that stay as they are
    with pytest.raises(sk.SkeresError, match="not implemented"):
        o.setLinearSolverType(sk.LinearSolverType.ITERATIVE_SCHUR)
    with pytest.raises(ValueError):
        o.setPreconditionerType(2)


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_elimination_plan_against_the_reference(name):
    problem, params, _, keep = k.build_device(name)
    got, want = sk.Solver.cgnrEliminationPlan(problem), k.plan(name)
    order = k.problem_order(name)
    of_block = got["eliminated_of_block"][list(order)]                 # in the case's block order
    print(name, {f: got[f] for f in got if f != "eliminated_of_block"}, flush=True)
    assert np.array_equal(of_block, want["eliminated_of_block"])
    for f in ("num_eliminated", "reduced_columns", "long_eliminated_blocks", "fe_pairs"):
        assert got[f] == want[f], (f, got[f], want[f])
    # the covariance's elimination takes the same set where it accepts the problem (the greedy rule is one function)
    cov = sk.Covariance.eliminationPlan(problem)
    assert np.array_equal(cov["eliminated_of_block"], got["eliminated_of_block"])
    assert cov["num_eliminated"] == got["num_eliminated"] and cov["reduced_columns"] == got["reduced_columns"]


def test_cases_reach_their_paths():
    assert k.plan("landmark")["long_eliminated_blocks"] == 1 and k.plan("quaternion")["long_eliminated_blocks"] == 1
    assert k.plan("quaternion")["E"] == [0]                            # the parameterized block, tangent size 3
    p = k.plan("chain")
    assert p["reduced_columns"] > 4096 and len(p["F"]) > 256           # a dot chunk, an update workgroup
    assert k.plan("all-eliminated")["F"] == [] and k.plan("all-eliminated")["reduced_columns"] == 0
    assert [e["linear_solver_iterations"] for e in k.reference("all-eliminated")[1][1:]] == [0, 0]
    assert [e["cg_status"] for e in k.reference("all-eliminated")[1][1:]] == [cr.CONVERGED, cr.CONVERGED]
    assert any(e["step_is_successful"] for e in k.reference("all-eliminated")[1][1:])
    # bal-robust: a camera's pair list has more than 128 pairs (three parts); bal-duplicate: one pair with two residual blocks
    prob = k.bal_problem("bal-robust")
    assert max(len(set(prob.point_index[prob.camera_index == c].tolist())) for c in range(2, prob.num_cameras)) > 128
    prob = k.bal_problem("bal-duplicate")
    pairs = list(zip(prob.camera_index.tolist(), prob.point_index.tolist()))
    assert len(pairs) - len(set(pairs)) == 1 and k.plan("bal-duplicate")["fe_pairs"] == k.plan("bal-small")["fe_pairs"]
    its = [e["linear_solver_iterations"] for e in k.reference("bal-reset")[1][1:]]
    assert its[0] == 15 and max(its) >= 11                             # the reset at iteration 10, a second batch
    assert [e["linear_solver_iterations"] for e in k.reference("bal-limit")[1][2:]] == [3] * 3
    assert any(e["cg_status"] == cr.ITERATION_LIMIT for e in k.reference("bal-limit")[1])
    assert any(not e["step_is_successful"] for e in k.reference("chain")[1])


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_reference_in_double_and_long_double(name):
    """cgnr_cases' rule: the same CG counts and endings in both, zeta away from eta at the stopping iteration and the one before,
    and the two logs ten times inside the tolerances the device is held to."""
    (_, a), (_, b) = k.reference(name), k.reference(name, True)
    eta = k.CASES[name].get("options", {}).get("eta", 0.1)
    assert len(a) == len(b) == k.CASES[name]["kmax"] + 1
    for i, (ea, eb) in enumerate(zip(a, b)):
        assert ea["linear_solver_iterations"] == eb["linear_solver_iterations"], i
        assert ea["cg_status"] == eb["cg_status"] and ea["step_is_valid"] == eb["step_is_valid"] and ea["step_is_successful"] == eb["step_is_successful"], i
        for e in (ea, eb):
            for z in e["zetas"][-2:]:
                assert abs(z - eta) > k.ZETA_MARGIN * eta, (i, e["zetas"][-2:])
    dev = cc.deviation(a, b)
    print(name, {f: "%.2e" % v for f, v in dev.items()}, [e["linear_solver_iterations"] for e in a], flush=True)
    for f, t in k.TOL.items():
        assert dev[f] <= t / 10, (f, dev[f])


@pytest.mark.parametrize("name", ["bal-reset", "bal-robust"])
def test_fewer_cg_iterations_than_the_full_system(name):
    schur = sum(e["linear_solver_iterations"] for e in k.reference(name)[1])
    full = sum(e["linear_solver_iterations"] for e in k.full_reference(name)[1])
    print("%s: CG iterations with the elimination %d, on the full system %d" % (name, schur, full), flush=True)
    assert schur < full


def _rejected(name, defect, **override):
    """True when the comparison the device is held to (cgnr_cases.compare_logs) rejects the reference with the defect."""
    good, bad = k.reference(name, **override)[1], k.reference(name, defect=defect, **override)[1]
    try:
        cc.compare_logs(bad, good, len(good) - 1)
    except AssertionError:
        return True
    return False


def test_planted_defects_are_rejected():
    # block-diag(U) in place of block-diag(S): another CG count on bal-reset's first solve
    good, bad = k.reference("bal-reset")[1], k.reference("bal-reset", defect="diag_u")[1]
    print("bal-reset first solve: block-diag(S) %d iterations, block-diag(U) %d" % (good[1]["linear_solver_iterations"], bad[1]["linear_solver_iterations"]), flush=True)
    assert (good[1]["linear_solver_iterations"], bad[1]["linear_solver_iterations"]) == (15, 17)
    assert _rejected("bal-reset", "diag_u")
    # W_ge squared per residual block instead of per pair: only the repeated observation tells
    assert _rejected("bal-duplicate", "per_slot") and not _rejected("bal-small", "per_slot")
    # the back-substitution left out
    assert _rejected("bal-small", "no_backsub")
    # ... and the step by itself (tests/test_gpu_cgnr_schur.py) tells both of the last two
    for name, defect in (("bal-duplicate", "per_slot"), ("bal-small", "no_backsub")):
        o = dict(max_num_iterations=1, max_linear_solver_iterations=1)
        ya, yb = k.reference(name, True, **o)[1][1]["scaled_step"], k.reference(name, True, defect=defect, **o)[1][1]["scaled_step"]
        na, nb = ya / ya[int(np.argmax(np.abs(ya)))], yb / yb[int(np.argmax(np.abs(yb)))]      # each to a largest entry of 1
        assert float(np.max(np.abs(na - nb))) > 1e-8


def test_step_by_itself_in_double_and_long_double():
    """What tests/test_gpu_cgnr_schur.py compares the device's step with: the normalised full step of one CG iteration, the same
    in double and in long double to 1e-9 (the device is held to 1e-8); its E part is not zero."""
    o = dict(max_num_iterations=1, max_linear_solver_iterations=1)
    a, b = k.reference("bal-small", **o)[1][1], k.reference("bal-small", True, **o)[1][1]
    assert a["linear_solver_iterations"] == 1 and a["cg_status"] == cr.ITERATION_LIMIT
    ya, yb = a["scaled_step"], b["scaled_step"]
    i = int(np.argmax(np.abs(yb)))
    assert float(np.max(np.abs(ya / ya[i] - yb / yb[i]))) <= 1e-9
    prob = k.bal_problem("bal-small")
    assert np.count_nonzero(yb[9 * prob.num_cameras:]) == 3 * prob.num_points and np.count_nonzero(yb) == k.model("bal-small").free.sum()
    assert np.all(b["first_direction"][9 * prob.num_cameras:] == 0)


def test_refusals_decided_without_a_device():
    """cgnr_refusal's, unchanged, with the option on: by the solver and by sk_cgnr_elimination_plan."""
    def refused(options, problem, message):
        with pytest.raises(sk.SkeresError, match=message) as e:
            sk.StepSolver(options, problem)
        assert "status 4" in str(e.value)
    import evaluate_cases as ec
    hosted, _, _, keep = ec.bal_host().build()
    refused(k.device_options("bal-small"), hosted, "host-evaluated")
    with pytest.raises(sk.SkeresError, match="host-evaluated"):
        sk.Solver.cgnrEliminationPlan(hosted)
    problem, params, _, keep2 = k.build_device("bal-small")
    o = k.device_options("bal-small")
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    refused(o, problem, "CGNR with DOGLEG")
    o = k.device_options("bal-small")
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    refused(o, problem, "world of 2 ranks")
    problem.setParameterLowerBound(params.slice(9 * 3), 0, -10.0)
    refused(k.device_options("bal-small"), problem, "parameter bounds under CGNR")
    with pytest.raises(sk.SkeresError, match="parameter bounds under CGNR"):
        sk.Solver.cgnrEliminationPlan(problem)
