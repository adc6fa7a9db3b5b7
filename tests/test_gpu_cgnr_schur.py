"""CGNR with the Schur elimination on the device against tests/cgnr_schur_reference.py: per LM iteration the accepted / rejected
pattern, the number of CG iterations and the CG status equal, cost at 1e-10, step norm, gradient max-norm, radius and relative
decrease at 1e-8 (cgnr_cases.TOL).  The cases and why they are what they are: tests/cgnr_schur_cases.py, tests/test_cgnr_schur_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skeres_amd as sk
import cgnr_reference as cr
import cgnr_cases as cc
import cgnr_schur_cases as k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
STATS = ("cg_iterations", "cg_iterations_last", "cg_status_last", "cg_batches", "linear_solves", "graph_replay", "schur_elimination",
         "eliminated_blocks", "reduced_columns", "schur_diagonal_pairs")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _solve(name, schur=True, stats=STATS, **override):
    """Steps a solver to its end.  Returns the log, x after every iteration (xs[0]: the start), the stats after every iteration
    that did not end the solve (stats[0]: after create), at the end (final), and the reports."""
    def _stats(solver):
        return {nm: solver.stat(nm) for nm in stats}
    problem, params, n, keep = k.build_device(name)
    solver = sk.StepSolver(k.device_options(name, schur, **override), problem)
    xs, st = [params.toArray(n)], [_stats(solver)]
    summary = sk.Solver.Summary()
    while not solver.step():
        solver.finish(summary)
        xs.append(params.toArray(n))
        st.append(_stats(solver))
    solver.finish(summary)
    return dict(log=summary.iterations(), xs=xs, stats=st, final=_stats(solver), report=summary.fullReport(), summary=summary)


@pytest.fixture(scope="module")
def runs():
    """The device run of a case, once per module."""
    cache = {}

    def run(name, schur=True, **override):
        key = (name, schur, tuple(sorted(override.items())))
        if key not in cache:
            cache[key] = _solve(name, schur, **override)
        return cache[key]
    return run


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_trajectories(runs, name):
    run, ref, plan = runs(name), k.reference(name)[1], k.plan(name)
    kmax = k.CASES[name]["kmax"]
    cc.compare_logs(run["log"], ref, kmax, show=name)
    total = sum(e["linear_solver_iterations"] for e in ref)
    assert run["final"]["cg_iterations"] == total and run["final"]["linear_solves"] == kmax and run["final"]["graph_replay"] == 0
    for i in range(1, len(run["stats"])):
        assert run["stats"][i]["cg_iterations_last"] == run["log"][i]["linear_solver_iterations"] == ref[i]["linear_solver_iterations"]
        assert run["stats"][i]["cg_status_last"] == ref[i]["cg_status"], i
    assert run["final"]["cg_status_last"] == ref[-1]["cg_status"]
    for i in range(1, len(run["xs"])):      # a rejected step leaves x alone
        if not run["log"][i]["step_is_successful"]:
            assert np.array_equal(run["xs"][i], run["xs"][i - 1])
    # the stats and the report's line
    for st in run["stats"] + [run["final"]]:
        assert st["schur_elimination"] == 1 and st["eliminated_blocks"] == plan["num_eliminated"] and st["reduced_columns"] == plan["reduced_columns"]
        assert st["schur_diagonal_pairs"] == plan["fe_pairs"]
    line = [ln for ln in run["report"].splitlines() if ln.startswith("Schur elimination")]
    assert len(line) == 1 and ("%d blocks eliminated" % plan["num_eliminated"]) in line[0] and ("%d reduced columns" % plan["reduced_columns"]) in line[0]
    pre = k.CASES[name].get("options", {}).get("preconditioner", "jacobi").upper()
    assert "CGNR" in run["report"] and pre in run["report"] and ("% 12d" % total) in run["report"]
    if name == "all-eliminated":            # the back-substitution alone: no batch was enqueued
        assert run["final"]["cg_batches"] == 0 and total == 0


def test_fewer_iterations_and_two_batches(runs):
    st = runs("bal-reset")["stats"]
    assert max(s["cg_iterations_last"] for s in st) >= 11
    assert st[-1]["cg_batches"] == sum(-(-int(e["linear_solver_iterations"]) // 8) for e in runs("bal-reset")["log"][1:])
    for name in ("bal-reset", "bal-robust"):
        full = runs(name, None)
        assert full["final"]["schur_elimination"] == 0 and full["final"]["eliminated_blocks"] == 0 and "Schur elimination" not in full["report"]
        print("%s: CG iterations with the elimination %d, without %d" % (name, runs(name)["final"]["cg_iterations"], full["final"]["cg_iterations"]), flush=True)
        assert runs(name)["final"]["cg_iterations"] < full["final"]["cg_iterations"]


def test_step_by_itself(runs):
    """bal-small at iteration 1 with max_linear_solver_iterations = 1: the step is (alpha M^-1 s, its back-substitution).  Against
    the long-double reference's scaled step, both scaled to a largest entry of 1: 1e-8, the project's tolerance for a step (the
    reference's own double and long double differ by less than 1e-9: tests/test_cgnr_schur_cpu.py)."""
    import step_check as sc
    run = runs("bal-small", max_num_iterations=1, max_linear_solver_iterations=1)
    assert run["log"][1]["step_is_successful"] and run["final"]["cg_status_last"] == cr.ITERATION_LIMIT
    ref = k.reference("bal-small", True, max_num_iterations=1, max_linear_solver_iterations=1)[1][1]
    model = k.model("bal-small")
    s = sc.jacobi_scale(model, k.x0("bal-small"))
    y = (run["xs"][1].astype(LD) - run["xs"][0].astype(LD)) / s
    d = ref["scaled_step"]
    assert np.all(y[~model.free] == 0) and np.all(d[~model.free] == 0)
    i = int(np.argmax(np.abs(d)))
    C = k.bal_problem("bal-small").num_cameras
    err = np.abs(y / y[i] - d / d[i])
    print("step: largest deviation of the normalised step %.3e on F, %.3e on E" % (float(np.max(err[:9 * C])), float(np.max(err[9 * C:]))), flush=True)
    assert float(np.max(err)) <= 1e-8


def test_two_solves_return_the_same_bytes(runs):
    for name in ("bal-robust", "landmark", "chain"):
        a, b = runs(name), _solve(name)
        assert len(a["xs"]) == len(b["xs"])
        for xa, xb in zip(a["xs"], b["xs"]):
            assert np.array_equal(xa, xb)
        assert [e["cost"] for e in a["log"]] == [e["cost"] for e in b["log"]]


def test_same_bytes_for_every_batch_size(tmp_path):
    """bal-reset and chain with SK_CGNR_BATCH = 1, 3 and the default: x after every LM iteration bitwise equal.  The developer
    variables are read once per process, so each setting runs in a process of its own (tests/cgnr_schur_worker.py)."""
    worker = os.path.join(ROOT, "tests", "cgnr_schur_worker.py")
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
        assert got[""][name + "/xs"].shape[0] == k.CASES[name]["kmax"] + 1 and not np.array_equal(got[""][name + "/xs"][0], got[""][name + "/xs"][-1])
        for mode, size in (("1", 1), ("3", 3), ("", 8)):   # reads of the done flag: one per batch
            assert got[mode][name + "/batches"][0] == sum(-(-int(n) // size) for n in cg), (name, mode)


def test_option_off_is_the_default_path(runs):
    """With the option explicitly off, x after every iteration equals the default CGNR run bitwise."""
    for name in ("bal-robust", "chain", "quaternion"):
        off, default = runs(name, False), runs(name, None)
        assert len(off["xs"]) == len(default["xs"]) > 1
        for xa, xb in zip(off["xs"], default["xs"]):
            assert np.array_equal(xa, xb)
        assert off["final"] == default["final"] and off["final"]["schur_elimination"] == 0
        assert off["report"].splitlines()[:12] == default["report"].splitlines()[:12] and "Schur elimination" not in off["report"]
        assert not all(np.array_equal(xa, xb) for xa, xb in zip(off["xs"], runs(name)["xs"]))    # ... and the option does change the step


def test_against_dense_schur(runs):
    """bal-small solved to convergence with and without the elimination and by DENSE_SCHUR: the final costs agree within ten
    times the relative gap between the reference's own Schur-CG and exact-step final costs (tests/cgnr_schur_cases.py)."""
    gap = k.final_cost_gap("bal-small")
    a, b = runs("bal-small", True, max_num_iterations=50), runs("bal-small", None, max_num_iterations=50)
    d = _solve("bal-small", None, stats=("linear_solves",), max_num_iterations=50, linear_solver_type=sk.LinearSolverType.DENSE_SCHUR)
    ca, cb, cd = a["summary"].finalCost(), b["summary"].finalCost(), d["summary"].finalCost()
    print("bal-small: CGNR with the elimination %.17g in %d iterations, without %.17g in %d, DENSE_SCHUR %.17g in %d; relative differences %.3e %.3e, allowed %.3e"
          % (ca, len(a["log"]) - 1, cb, len(b["log"]) - 1, cd, len(d["log"]) - 1, abs(ca - cd) / cd, abs(cb - cd) / cd, 10 * gap), flush=True)
    assert a["summary"].terminationType() == b["summary"].terminationType() == d["summary"].terminationType() == sk.TerminationType.CONVERGENCE
    assert abs(ca - cd) <= 10 * gap * cd and abs(cb - cd) <= 10 * gap * cd and abs(ca - cb) <= 10 * gap * cb
    # under another solver type the option has no effect: the same bytes
    on = _solve("bal-small", True, stats=("linear_solves",), max_num_iterations=50, linear_solver_type=sk.LinearSolverType.DENSE_SCHUR)
    assert len(on["xs"]) == len(d["xs"]) and all(np.array_equal(xa, xb) for xa, xb in zip(on["xs"], d["xs"])) and "Schur elimination" not in on["report"]


def test_untouched_blocks_keep_their_bits(runs):
    run = runs("bal-robust")
    free, x0 = k.model("bal-robust").free, k.x0("bal-robust")
    assert (~free).sum() == 63
    for x in run["xs"]:
        assert np.array_equal(x[~free], x0[~free])      # bitwise: constant cameras, a constant point, held intrinsics
    assert not np.array_equal(run["xs"][-1][free], x0[free])


def test_refusals():
    """Decided from host data with the option on, with the messages of today."""
    problem, params, n, keep = k.build_device("bal-small")
    o = k.device_options("bal-small")
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    with pytest.raises(sk.SkeresError, match="CGNR with DOGLEG"):
        sk.StepSolver(o, problem)
    o = k.device_options("bal-small")
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    with pytest.raises(sk.SkeresError, match="world of 2 ranks"):
        sk.StepSolver(o, problem)
    import evaluate_cases as ec
    hosted, _, _, keep2 = ec.bal_host().build()
    with pytest.raises(sk.SkeresError, match="host-evaluated"):
        sk.StepSolver(k.device_options("bal-small"), hosted)
    problem.setParameterLowerBound(params.slice(9 * 3), 0, -10.0)
    with pytest.raises(sk.SkeresError, match="parameter bounds under CGNR"):
        sk.StepSolver(k.device_options("bal-small"), problem)
