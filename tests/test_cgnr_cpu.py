"""CGNR without a device: the reference (tests/cgnr_reference.py) against itself in double and in long double on every case of
tests/cgnr_cases.py, what each case is there to exercise, the validation of the four options, and the refusals that are decided
from host data alone (before a device is touched)."""
import numpy as np
import pytest

import skeres_amd as sk
import oracle
import cgnr_reference as cr
import cgnr_cases as cc

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_reference_in_double_and_long_double(name):
    """Per compared LM iteration the two take the same number of CG iterations and end the same way; zeta at the stopping
    iteration and at the one before stays away from eta by a relative 1e-3 in both (so the device, a third rounding of the same
    loop, stops where they do); and the two logs agree ten times inside the tolerances the device is held to."""
    kmax = cc.CASES[name]["kmax"]
    (_, a), (_, b) = cc.reference(name), cc.reference(name, True)
    eta = cc.CASES[name].get("options", {}).get("eta", 0.1)
    assert len(a) == len(b)
    if name != "at-optimum":
        assert len(a) == kmax + 1
    for k, (ea, eb) in enumerate(zip(a, b)):
        assert ea["linear_solver_iterations"] == eb["linear_solver_iterations"], (k, ea["linear_solver_iterations"], eb["linear_solver_iterations"])
        assert ea["cg_status"] == eb["cg_status"] and ea["step_is_valid"] == eb["step_is_valid"] and ea["step_is_successful"] == eb["step_is_successful"], k
        for e in (ea, eb):
            for z in e["zetas"][-2:]:
                assert abs(z - eta) > cc.ZETA_MARGIN * eta, (k, e["zetas"][-2:])
    dev = cc.deviation(a, b)
    print(name, {f: "%.2e" % v for f, v in dev.items()}, [e["linear_solver_iterations"] for e in a], flush=True)
    for f, t in cc.TOL.items():
        assert dev[f] <= t / 10, (f, dev[f])


def test_cases_exercise_what_they_are_there_for():
    its = lambda name: [e["linear_solver_iterations"] for e in cc.reference(name)[1][1:]]
    status = lambda name: [e["cg_status"] for e in cc.reference(name)[1][1:]]
    assert all(s == cr.CONVERGED for s in status("bal-small")) and all(s == cr.CONVERGED for s in status("bal-identity"))
    assert max(its("bal-reset")) >= 11                          # the residual reset at iteration 10, a solve of more than one batch
    assert its("bal-limit") == [3] * cc.CASES["bal-limit"]["kmax"] and all(s == cr.ITERATION_LIMIT for s in status("bal-limit"))
    assert all(e["step_is_valid"] for e in cc.reference("bal-limit")[1])    # the step of a solve that hit the limit is used
    assert any(e["step_is_successful"] for e in cc.reference("bal-limit")[1][1:])
    # the robust case: held coordinates never move in the reference either
    free = cc.model("bal-robust").free
    assert (~free).sum() == 63
    assert np.array_equal(cc.reference("bal-robust")[0][~free], cc.x0("bal-robust")[~free])
    # chain: n crosses a 4096 chunk; a hub with a long slot list; single-slot ends; reversed pairs
    case = cc._chain()
    assert len(case.x) == 4200 and len(case.sizes) == 2100
    count = np.zeros(2100, dtype=int)
    for blk in case.blocks:
        for q in blk[2]:
            count[q] += 1
    assert count[cc.CHAIN_HUB] >= 300 and count[0] == 1 and count[2099] == 1 and sorted(set(count.tolist())) == [1, 2, 3, count[cc.CHAIN_HUB]]
    assert sum(1 for blk in case.blocks if blk[2][0] > blk[2][1]) >= 400
    assert any(not e["step_is_successful"] for e in cc.reference("chain")[1])    # a rejected step: a second solve from the same block sums


def test_zero_right_hand_side():
    """HelloWorld at x = 10: the gradient is zero, so the trust-region loop (SolverBase's, and the reference's) ends at its gradient
    test before any linear solve: one logged iteration.  The CG loop's own answer to b = 0 — status 3, step 0 — is what the
    reference's loop gives when it is called directly; the driver never reaches it, on the device either."""
    x, log = cc.reference("at-optimum")
    assert len(log) == 1 and log[0]["cost"] == 0.0 and log[0]["gradient_max_norm"] == 0.0 and x[0] == 10.0
    m = cc.model("at-optimum")
    lin = cr._linearize(m, np.array([10.0]), np.ones(1), np.float64)
    y, its, status, zetas, _ = cr.conjugate_gradients(lin, 1, np.array([1e-10]), np.zeros(1), None, cr.DEFAULTS, np.float64)
    assert status == cr.ZERO_RHS and its == 0 and y[0] == 0.0 and zetas == []


def test_first_direction_is_the_preconditioned_right_hand_side():
    """What tests/test_gpu_cgnr.py compares the device's preconditioner with: M^-1 b of iteration 1, the same in double and in long
    double to 1e-9 of its largest entry (the device is held to 1e-8)."""
    a = cc.reference("bal-small", max_num_iterations=1, max_linear_solver_iterations=1)[1][1]
    b = cc.reference("bal-small", True, max_num_iterations=1, max_linear_solver_iterations=1)[1][1]
    da, db = a["first_direction"], b["first_direction"]
    assert a["linear_solver_iterations"] == 1 and a["cg_status"] == cr.ITERATION_LIMIT
    assert float(np.max(np.abs(da - db))) <= 1e-9 * float(np.max(np.abs(db)))
    ya, yb = a["scaled_step"], b["scaled_step"]       # the step of that solve is alpha times it
    assert float(np.max(np.abs(ya / np.max(np.abs(ya)) - db / np.max(np.abs(db))))) <= 1e-9
    assert np.count_nonzero(yb) == cc.model("bal-small").free.sum()


def test_option_validation():
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.CGNR)          # (refused until this solver existed)
    for t in (sk.LinearSolverType.SPARSE_NORMAL_CHOLESKY, sk.LinearSolverType.SPARSE_SCHUR, sk.LinearSolverType.ITERATIVE_SCHUR):
        with pytest.raises(sk.SkeresError, match="not implemented"):
            o.setLinearSolverType(t)
    o.setPreconditionerType(sk.PreconditionerType.IDENTITY)
    o.setPreconditionerType(sk.PreconditionerType.JACOBI)
    for bad in (-1, 2, 5):
        with pytest.raises(ValueError):
            o.setPreconditionerType(bad)
    for bad in (0.0, -0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            o.setEta(bad)
    o.setEta(1e-8)
    o.setEta(0.1)
    with pytest.raises(ValueError):
        o.setMaxLinearSolverIterations(-1)
    with pytest.raises(ValueError):
        o.setMinLinearSolverIterations(-1)
    o.setMaxLinearSolverIterations(20)
    with pytest.raises(ValueError):
        o.setMinLinearSolverIterations(21)                   # min > max
    o.setMinLinearSolverIterations(5)
    with pytest.raises(ValueError):
        o.setMaxLinearSolverIterations(4)                    # max < min
    o.setMaxLinearSolverIterations(5)
    assert sk.PreconditionerType.IDENTITY == 0 and sk.PreconditionerType.JACOBI == 1


def _cgnr_options():
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.CGNR)
    return o


def _refused(options, problem, message):
    with pytest.raises(sk.SkeresError, match=message) as e:
        sk.StepSolver(options, problem)
    assert "status 4" in str(e.value)                        # SK_ERR_UNSUPPORTED


def test_refusals_decided_without_a_device():
    """Each of them by its message, from host data alone: the same answer with and without a device."""
    # host-evaluated residual blocks
    import evaluate_cases as ec
    problem, _, params, keep = ec.bal_host().build()
    _refused(_cgnr_options(), problem, "host-evaluated")
    # DOGLEG
    problem, params, _, keep = cc.build_device("bal-small")
    o = _cgnr_options()
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    _refused(o, problem, "CGNR with DOGLEG")
    # more than one rank
    o = _cgnr_options()
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    _refused(o, problem, "world of 2 ranks")
    # parameter bounds
    problem.setParameterLowerBound(params.slice(9 * 3), 0, -10.0)
    _refused(_cgnr_options(), problem, "parameter bounds under CGNR")
    # a block of tangent size above 16
    class Wide(sk.TracedCostFunctor):
        def __init__(self):
            super().__init__(1, 17)

        def apply(self, x):
            s = x[0]
            for i in range(1, 17):
                s = s + x[i] * x[i]
            return [s]
    wide = Wide()
    x = sk.RichDoubleArray.fromArray(np.ones(17))
    problem = sk.Problem()
    problem.addResidualBlocksTraced(wide, np.zeros((1, 0)), None, x, np.zeros((1, 1), dtype=np.int64))
    _refused(_cgnr_options(), problem, "tangent size up to 16")
    # dense rows
    x = sk.RichDoubleArray.fromArray(np.zeros(8))
    problem = sk.Problem()
    problem.addDenseRows(oracle.SYNTH_TANH_ROW, np.array([[1.0, float(i), 0.1] for i in range(4)]), None, x, 8)
    _refused(_cgnr_options(), problem, "dense-row problems")
    # (an explicit Cholesky tuning is ignored, not refused: tests/test_gpu_cgnr.py)
