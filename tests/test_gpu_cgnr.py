"""CGNR on the device against tests/cgnr_reference.py: per LM iteration the accepted / rejected pattern and the number of CG
iterations equal, cost at 1e-10, step norm, gradient max-norm, radius and relative decrease at 1e-8 (relative; the project's
tolerances for oracle comparisons).  The cases and why they are what they are: tests/cgnr_cases.py, tests/test_cgnr_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skeres_amd as sk
import cgnr_reference as cr
import cgnr_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
STATS = ("cg_iterations", "cg_iterations_last", "cg_status_last", "cg_batches", "linear_solves", "jacobian_nonzeros", "graph_replay",
         "phase_seconds_1", "phase_seconds_2", "phase_seconds_3")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _solve(name, stats=STATS, **override):
    """Steps a solver to its end.  Returns the log, x after every iteration (xs[0]: the start), the stats after every iteration
    that did not end the solve (stats[0]: after create), at the end (final), and the reports."""
    def _stats(solver):
        return {nm: solver.stat(nm) for nm in names}   # (a stat the solver does not have raises)
    names = stats
    problem, params, n, keep = cc.build_device(name)
    solver = sk.StepSolver(cc.device_options(name, **override), problem)
    xs, stats = [params.toArray(n)], [_stats(solver)]
    summary = sk.Solver.Summary()
    while not solver.step():
        solver.finish(summary)
        xs.append(params.toArray(n))
        stats.append(_stats(solver))
    solver.finish(summary)
    return dict(log=summary.iterations(), xs=xs, stats=stats, final=_stats(solver), report=summary.fullReport(), summary=summary)


@pytest.fixture(scope="module")
def runs():
    """The device run of a case, once per module."""
    cache = {}

    def run(name, **override):
        key = (name, tuple(sorted(override.items())))
        if key not in cache:
            cache[key] = _solve(name, **override)
        return cache[key]
    return run


@pytest.mark.parametrize("name", sorted(n for n in cc.CASES if n != "at-optimum"))
def test_trajectories(runs, name):
    run, ref = runs(name), cc.reference(name)[1]
    kmax = cc.CASES[name]["kmax"]
    cc.compare_logs(run["log"], ref, kmax, show=name)
    pre = cc.CASES[name].get("options", {}).get("preconditioner", "jacobi").upper()
    assert "CGNR" in run["report"] and pre in run["report"] and ("IDENTITY" if pre == "JACOBI" else "JACOBI") not in run["report"]
    total = sum(e["linear_solver_iterations"] for e in ref)
    assert run["final"]["cg_iterations"] == total and ("% 12d" % total) in run["report"]
    assert run["final"]["graph_replay"] == 0
    assert run["final"]["linear_solves"] == kmax
    assert run["final"]["cg_status_last"] == ref[-1]["cg_status"]
    for k in range(1, len(run["stats"])):   # the log's field is the solver's counter of that iteration
        assert run["stats"][k]["cg_iterations_last"] == run["log"][k]["linear_solver_iterations"] == ref[k]["linear_solver_iterations"]
        assert run["stats"][k]["cg_status_last"] == ref[k]["cg_status"]
        for p in (1, 2, 3):
            assert run["stats"][k]["phase_seconds_%d" % p] > run["stats"][k - 1]["phase_seconds_%d" % p]
    for k in range(1, len(run["xs"])):      # a rejected step leaves x alone
        if not run["log"][k]["step_is_successful"]:
            assert np.array_equal(run["xs"][k], run["xs"][k - 1])


def test_statuses_and_structure(runs):
    assert all(s["cg_status_last"] == cr.CONVERGED for s in runs("bal-small")["stats"][1:])
    assert all(s["cg_status_last"] == cr.ITERATION_LIMIT and s["cg_iterations_last"] == 3 for s in runs("bal-limit")["stats"][1:])
    assert any(e["step_is_successful"] for e in runs("bal-limit")["log"][1:])     # the step of a solve that hit the limit is used
    assert runs("bal-small")["stats"][0]["cg_status_last"] == -1                   # no linear solve yet
    prob = cc.bal_problem("bal-small")
    # the full camera + point system: two rows of 9 + 3 entries per observation, less the constant cameras' 9
    const = sum(int(np.sum(prob.camera_index == c)) for c in (0, 1))
    assert runs("bal-small")["final"]["jacobian_nonzeros"] == 2 * (12 * prob.num_observations - 9 * const)
    assert runs("chain")["final"]["jacobian_nonzeros"] == 3 * 4 * len(cc._chain().blocks)
    # bal-reset: a solve of more than ten iterations (the residual reset) and of more than one batch of eight
    st = runs("bal-reset")["stats"]
    assert max(s["cg_iterations_last"] for s in st) >= 11
    assert st[-1]["cg_batches"] == sum(-(-int(e["linear_solver_iterations"]) // 8) for e in runs("bal-reset")["log"][1:])


def test_robust_loss_subset_and_constant_point(runs):
    run = runs("bal-robust")
    free, x0 = cc.model("bal-robust").free, cc.x0("bal-robust")
    assert (~free).sum() == 63
    for x in run["xs"]:
        assert np.array_equal(x[~free], x0[~free])      # bitwise
    assert not np.array_equal(run["xs"][-1][free], x0[free])


def test_at_optimum(runs):
    """HelloWorld at x = 10: zero gradient.  SolverBase's gradient test ends the solve before a linear solve is enqueued, as in
    the reference (tests/test_cgnr_cpu.py: test_zero_right_hand_side), so the CG loop's status 3 (zero right-hand side) is not
    reachable through the driver: the solver reports no linear solve and no status."""
    run = runs("at-optimum")
    assert len(run["log"]) == len(cc.reference("at-optimum")[1]) == 1
    assert run["summary"].terminationType() == sk.TerminationType.CONVERGENCE and "Gradient tolerance" in run["summary"].message()
    assert run["final"]["linear_solves"] == 0 and run["final"]["cg_iterations"] == 0 and run["final"]["cg_status_last"] == -1
    assert run["xs"][-1][0] == 10.0 and run["log"][0]["cost"] == 0.0


def test_same_bytes_for_every_batch_size(tmp_path):
    """bal-reset and chain with SK_CGNR_BATCH = 1, 3 and the default: x after every LM iteration bitwise equal.  The developer
    variables are read once per process, so each setting runs in a process of its own (tests/cgnr_worker.py)."""
    worker = os.path.join(ROOT, "tests", "cgnr_worker.py")
    got = {}
    for mode in ("1", "3", ""):
        path = str(tmp_path / ("batch_%s.npz" % (mode or "default")))
        env = dict(os.environ)
        env.pop("SK_CGNR_BATCH", None)
        if mode:
            env["SK_CGNR_BATCH"] = mode
        out = subprocess.run([sys.executable, worker, path, "bal-reset", "chain"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        got[mode] = np.load(path)
    for name in ("bal-reset", "chain"):
        for mode in ("1", "3"):
            assert np.array_equal(got[mode][name + "/xs"], got[""][name + "/xs"]), (name, mode)
            assert np.array_equal(got[mode][name + "/cg"], got[""][name + "/cg"])
        cg = got[""][name + "/cg"][1:]
        assert got[""][name + "/xs"].shape[0] == cc.CASES[name]["kmax"] + 1 and not np.array_equal(got[""][name + "/xs"][0], got[""][name + "/xs"][-1])
        for mode, size in (("1", 1), ("3", 3), ("", 8)):   # reads of the done flag: one per batch
            assert got[mode][name + "/batches"][0] == sum(-(-int(k) // size) for k in cg), (name, mode)


def test_two_solves_return_the_same_bytes(runs):
    for name in ("bal-robust", "chain"):
        a, b = runs(name), _solve(name)
        assert len(a["xs"]) == len(b["xs"])
        for xa, xb in zip(a["xs"], b["xs"]):
            assert np.array_equal(xa, xb)
        assert [e["cost"] for e in a["log"]] == [e["cost"] for e in b["log"]]


def test_preconditioner_by_itself(runs):
    """bal-small at iteration 1 with max_linear_solver_iterations = 1: the step is alpha M^-1 b, so the device's first CG direction
    is its step (x_1 - x_0) / s up to the factor alpha.  Against the reference's M^-1 b in long double, both scaled to a largest
    entry of 1: 1e-8, the project's tolerance for a step (the reference's own double and long double differ by less than 1e-9:
    tests/test_cgnr_cpu.py)."""
    run = runs("bal-small", max_num_iterations=1, max_linear_solver_iterations=1)
    assert run["log"][1]["step_is_successful"] and run["final"]["cg_status_last"] == cr.ITERATION_LIMIT
    ref = cc.reference("bal-small", True, max_num_iterations=1, max_linear_solver_iterations=1)[1][1]
    model = cc.model("bal-small")
    import step_check as sc
    s = sc.jacobi_scale(model, cc.x0("bal-small"))
    y = (run["xs"][1].astype(LD) - run["xs"][0].astype(LD)) / s
    d = ref["first_direction"]
    assert np.all(y[~model.free] == 0) and np.all(d[~model.free] == 0)
    k = int(np.argmax(np.abs(d)))
    err = float(np.max(np.abs(y / y[k] - d / d[k])))
    print("preconditioner: largest deviation of the normalised direction %.3e" % err, flush=True)
    assert err <= 1e-8


def test_chain_against_dense_normal_cholesky(runs):
    """No comparison with a factorisation solver tighter than the reference allows: `chain` solved to convergence by CGNR and by
    DENSE_NORMAL_CHOLESKY; the final costs agree within ten times the relative gap between the reference's own CGNR and
    exact-step final costs (computed and printed by tests/cgnr_cases.py)."""
    gap = cc.chain_final_cost_gap()
    a = runs("chain", max_num_iterations=50)
    b = _solve("chain", stats=("linear_solves",), max_num_iterations=50, linear_solver_type=sk.LinearSolverType.DENSE_NORMAL_CHOLESKY)
    ca, cb = a["summary"].finalCost(), b["summary"].finalCost()
    print("chain: CGNR %.17g in %d iterations, DENSE_NORMAL_CHOLESKY %.17g in %d; relative difference %.3e, allowed %.3e"
          % (ca, len(a["log"]) - 1, cb, len(b["log"]) - 1, abs(ca - cb) / cb, 10 * gap), flush=True)
    assert a["summary"].terminationType() == b["summary"].terminationType() == sk.TerminationType.CONVERGENCE
    assert abs(ca - cb) <= 10 * gap * cb
    assert b["log"][1]["linear_solver_iterations"] == 0 and a["log"][1]["linear_solver_iterations"] > 0   # field 10: 0 for the other solvers


def test_refusals_and_ignored_tuning():
    """The refusals are decided from host data (tests/test_cgnr_cpu.py has each by its message); with a device present they are
    the same.  An explicit Cholesky tuning is ignored."""
    problem, params, n, keep = cc.build_device("bal-small")
    o = cc.device_options("bal-small")
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    with pytest.raises(sk.SkeresError, match="CGNR with DOGLEG"):
        sk.StepSolver(o, problem)
    o = cc.device_options("bal-small")
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    with pytest.raises(sk.SkeresError, match="world of 2 ranks"):
        sk.StepSolver(o, problem)
    import evaluate_cases as ec
    hosted, _, _, keep2 = ec.bal_host().build()
    with pytest.raises(sk.SkeresError, match="host-evaluated"):
        sk.StepSolver(cc.device_options("bal-small"), hosted)
    o = cc.device_options("bal-small")
    o.setCholeskyTuning(2, False)
    summary = sk.Solver.Summary()
    sk.ceres.solve(o, problem, summary)
    assert [e["cost"] for e in summary.iterations()] == [e["cost"] for e in _solve("bal-small")["log"]]
    problem.setParameterLowerBound(params.slice(9 * 3), 0, -10.0)
    with pytest.raises(sk.SkeresError, match="parameter bounds under CGNR"):
        sk.StepSolver(cc.device_options("bal-small"), problem)


def test_twenty_thousand_blocks():
    """A chain of 20 000 blocks (n = 40 000): the dense path's normal matrix alone would be 12.8 GB.  Solved until the gradient's
    max-norm is below 1e-3 (from about 7 at the start: the chain's minimiser is one of a family, and along that family
    Gauss-Newton steps gain slowly, so a tighter tolerance measures patience, not the solver): the accepted costs fall
    monotonically and the solve takes a few seconds."""
    import time
    case = cc.chain_case(num_blocks=20000, hub_blocks=5000)
    problem, _, params, keep = case.build()
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.CGNR)
    o.setGradientTolerance(1e-3)
    o.setFunctionTolerance(1e-14)
    o.setParameterTolerance(1e-14)
    o.setMaxNumIterations(100)
    summary = sk.Solver.Summary()
    t = time.time()
    sk.ceres.solve(o, problem, summary)
    seconds = time.time() - t
    log = summary.iterations()
    print("20000 blocks: %d iterations, %d CG iterations, cost %.6e -> %.6e, gradient %.3e, %.2f s" % (
        len(log) - 1, sum(e["linear_solver_iterations"] for e in log), log[0]["cost"], summary.finalCost(), log[-1]["gradient_max_norm"], seconds), flush=True)
    assert summary.terminationType() == sk.TerminationType.CONVERGENCE and "Gradient tolerance" in summary.message(), summary.message()
    accepted = [e["cost"] for e in log if e["step_is_successful"]]
    assert len(accepted) >= 3 and all(b < a for a, b in zip(accepted, accepted[1:]))
    assert log[-1]["gradient_max_norm"] <= 1e-3 < log[0]["gradient_max_norm"]
    assert seconds < 60
