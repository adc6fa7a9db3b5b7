"""The failure paths of the trust-region loop on the device, through StepSolver, against tests/failure_reference.py: an evaluation
that fails at the start or after an accepted step, candidates that cannot be evaluated, linear solves that are not valid — until
the solve gives up (case f), or followed by valid ones on every plan of the reduced system (case i) — and what is written back in
each case — on DENSE_QR, DENSE_NORMAL_CHOLESKY, DENSE_SCHUR and dense rows.  The cases, their margins and
the comparison (exact discrete fields and messages, the radius to 1e-14, the continuous fields to the dogleg case file's
tolerances, untouched points by their bits): tests/failure_cases.py; that the comparison rejects planted defects:
tests/test_failure_cpu.py.  Observed deviations: profiles/failure_paths.txt."""
import numpy as np
import pytest

import skeres_amd as sk
import failure_cases as fc
import failure_reference as fr
import step_check as sc

pytestmark = pytest.mark.gpu

SCHUR_STATS = ("graph_replay", "tape_blocks", "host_callback_blocks", "cholesky_columns_resident", "retained_points", "dissected")
DENSE_STATS = ("tape_blocks",)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _run(name):
    c = fc.CASES[name]
    stats = SCHUR_STATS if c["backend"] == "DENSE_SCHUR" else DENSE_STATS if c["backend"] != "ROWS" else ()
    run = fc.device_run(name, stats)
    worst = {}
    try:
        fc.compare(run, fc.reference(name), fc.start(name), show=name, worst=worst)
    finally:
        print("worst", name, run["termination"], "|", run["message"], "|", " ".join("%s %.3g" % kv for kv in sorted(worst.items())), flush=True)
    return run


@pytest.mark.parametrize("name", fc.names(kind="a"))
def test_a_non_finite_initial_parameter(name):
    run = _run(name)
    x0 = fc.start(name)
    assert np.array_equal(fc.bits(run["x"]), fc.bits(x0))
    if name != "a-rows-inf":   # (tanh(inf) = 1: that evaluation succeeds, with a zero gradient)
        assert run["message"] == fr.MSG_INITIAL and run["log"] == []


@pytest.mark.parametrize("name", fc.names(kind="b"))
def test_b_director_block_fails_on_its_first_call(name):
    run = _run(name)
    assert run["message"] == fr.MSG_INITIAL and run["log"] == []
    if fc.CASES[name]["backend"] == "DENSE_SCHUR":
        assert run["stats"]["host_callback_blocks"] == len(fc.host_blocks(name))


@pytest.mark.parametrize("name", fc.names(kind="c"))
def test_c_barrier_in_a_recorded_functor(name):
    c = fc.CASES[name]
    run = _run(name)
    nblocks = 20 if c["backend"] != "DENSE_SCHUR" else fc._prob(c).num_observations
    assert run["stats"]["tape_blocks"] == nblocks
    if "replay" in c:
        # A recorded functor (like a director block) switches the replay of the iteration as a hipGraph off, whatever the option says
        # (BalSolver::setup), and the compiled Snavely functor has no barrier: no failed candidate reaches a replayed graph through the
        # public interface (open: tests/failure_cases.py).
        assert run["stats"]["graph_replay"] == 0
    k = c["failed_candidates"]
    for e in run["log"][1:k + 1]:   # rejected as VALID steps of cost DBL_MAX
        assert e["step_is_valid"] and not e["step_is_successful"] and e["cost_change"] == e["cost"] - fr.DBL_MAX
    assert run["log"][k + 1]["step_is_successful"] and run["termination"] == fr.CONVERGENCE


@pytest.mark.parametrize("name", fc.names(kind="d"))
def test_d_director_block_fails_beyond_the_barrier(name):
    c = fc.CASES[name]
    run = _run(name)
    k = c["failed_candidates"]
    for e in run["log"][1:k + 1]:
        assert e["step_is_valid"] and not e["step_is_successful"] and e["cost_change"] == e["cost"] - fr.DBL_MAX
    assert run["log"][k + 1]["step_is_successful"] and run["termination"] == fr.CONVERGENCE
    if c["backend"] == "DENSE_SCHUR":
        assert run["stats"]["host_callback_blocks"] == len(fc.host_blocks(name)) and run["stats"]["graph_replay"] == 0


@pytest.mark.parametrize("name", fc.names(kind="e"))
def test_e_evaluation_after_an_accepted_step_fails(name):
    run = _run(name)
    ref = fc.reference(name)
    assert run["message"] == fr.MSG_EVALUATION and len(run["log"]) == 2 and run["num_successful_steps"] == 1
    assert not np.array_equal(run["x"], run["xs"][1])   # the accepted candidate came back, not the point before it
    # what the device returns where the contract leaves it open: the cost of the last point whose evaluation succeeded
    assert run["final_cost"] == run["log"][1]["cost"] and abs(run["final_cost"] - ref["log"][1]["cost"]) <= fc.TOL["cost"] * ref["log"][1]["cost"]


@pytest.mark.parametrize("name", fc.names(kind="f"))
def test_f_every_linear_solve_is_invalid(name):
    c = fc.CASES[name]
    run = _run(name)
    limit = fc.options(name).get("max_num_consecutive_invalid_steps", 5)
    assert run["message"] == fr.MSG_INVALID % limit and len(run["log"]) == limit + 1
    assert [e["trust_region_radius"] for e in run["log"]] == [e["trust_region_radius"] for e in fc.reference(name)["log"]]   # powers of two: exact
    for x in run["xs"]:
        assert np.array_equal(fc.bits(x), fc.bits(fc.start(name)))
    if c["backend"] == "DENSE_SCHUR":
        assert run["stats"]["cholesky_columns_resident"] == 0 and run["stats"]["tape_blocks"] == fc._prob(c).num_observations


@pytest.mark.parametrize("name", fc.names(kind="g"))
def test_g_non_finite_jacobian_beside_finite_residuals(name):
    """Held to the level fc.G_LEVEL names for the backend: "exact" is the whole comparison (_run), "invariants" its first part."""
    c = fc.CASES[name]
    if fc.G_LEVEL[c["backend"]] == "exact":
        run = _run(name)
        assert run["message"] == fr.MSG_INITIAL and run["log"] == []
    else:
        run = fc.device_run(name)
        assert run["termination"] == fr.FAILURE and np.isfinite(run["final_cost"])
    assert np.array_equal(fc.bits(run["x"]), fc.bits(fc.start(name)))


@pytest.mark.parametrize("name", fc.names(kind="h"))
def test_h_failed_candidates_then_recovery_under_forced_plans(name):
    c = fc.CASES[name]
    run = _run(name)
    if "setRetainedPoints" in c["knobs"]:
        assert run["stats"]["retained_points"] == 3
    else:
        assert run["stats"]["dissected"] == 1
    assert run["stats"]["cholesky_columns_resident"] > 0   # (a failed pivot releases the chain's waiters through their counters: DESIGN.md section 4)
    k = c["failed_candidates"]
    assert [bool(e["step_is_successful"]) for e in run["log"][1:k + 2]] == [False] * k + [True]
    # the step after the rejected ones solves ITS normal equations: nothing of the failed candidates stayed in the envelope
    model = fc.model(name)
    e = sc.check(model, run["xs"][0], run["xs"][k], run["xs"][k + 1], run["log"], k + 1)
    print("step_check", name, e, flush=True)
    e = sc.check(model, run["xs"][0], run["xs"][k + 1], run["xs"][k + 2], run["log"], k + 2)
    print("step_check", name, e, flush=True)


# ---------------------------------------------------------------------------------------------------------------------------
# case i: linear solves that are not valid, then valid ones, several times, on every plan (tests/failure_cases.py; the device runs
# are tests/failure_worker.py's, in a process of their own)
# ---------------------------------------------------------------------------------------------------------------------------
LOG_BITS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")
COMPARE = {"eq": lambda a, b: a == b, "gt": lambda a, b: a > b}


def _worker(name, tmp_path):
    import os
    import pickle
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "run.pickle")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "failure_worker.py"), name, path], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "FAILURE_WORKER_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "timed out" not in out.stderr, out.stderr[-3000:]   # (the chain's and the back-substitution's time-outs say so on stderr)
    with open(path, "rb") as f:
        return pickle.load(f)


def _episodes(log):
    """[(first, last)] of the runs of consecutive invalid entries."""
    out = []
    for k in range(1, len(log)):
        if not log[k]["step_is_valid"]:
            if out and out[-1][1] == k - 1:
                out[-1] = (out[-1][0], k)
            else:
                out.append((k, k))
    return out


@pytest.mark.parametrize("name", fc.names(kind="i"))
def test_i_invalid_solves_then_valid_ones(name, tmp_path):
    c, comp = fc.CASES[name], fc.component(name)
    x0, ref = fc.start(name), fc.reference(name)
    got = _worker(name, tmp_path)
    run, twin = got["run"], got["twin"]
    log = run["log"]
    # the log against the reference (discrete fields and messages exact, the radius exact where the reference's is, x untouched by its
    # bits over every invalid iteration)
    worst = {}
    try:
        fc.compare(run, ref, x0, show=name, worst=worst)
    finally:
        print("worst", name, run["termination"], "|", run["message"], "|", " ".join("%s %.3g" % kv for kv in sorted(worst.items())), flush=True)
    # the radius sequence of these cases is exact (powers of two and x 3) and the decisions hang on its bits: equal to the reference's by its bits
    for k, (e, r) in enumerate(zip(log, ref["log"])):
        assert r["radius_exact"] and np.array_equal(fc.bits(e["trust_region_radius"]), fc.bits(r["trust_region_radius"])), (k, e["trust_region_radius"], r["trust_region_radius"])
    xs = run["xs"] + [run["x"]] * (len(log) - len(run["xs"]))   # x after iteration k
    for k in range(1, len(log)):
        if not log[k]["step_is_valid"]:
            assert np.array_equal(fc.bits(xs[k]), fc.bits(xs[k - 1])), k
    ep = _episodes(log)
    accepted_before = [sum(int(bool(e["step_is_successful"])) for e in log[1:first]) for first, _ in ep]
    print("record", name, "episodes", ep, "parity of the graph at each", [a % 2 for a in accepted_before], flush=True)
    assert len(ep) >= c["episodes"] and ep[0][0] == 1 and ep[0][1] >= 2
    # the zero columns on the device, at x0 and at the final x; the component, where nothing couples it to the rest, by its bits
    assert all(count > 0 and zero for count, zero in got["zero"][0]), got["zero"]
    if c.get("generic"):
        assert len(ep) == 1 and not any(zero for _, zero in got["zero"][1]), got["zero"]
    else:
        assert all(count > 0 and zero for count, zero in got["zero"][1]), got["zero"]
        assert np.array_equal(fc.bits(run["x"][comp["columns"]]), fc.bits(x0[comp["columns"]]))
        assert {a % 2 for a in accepted_before} == {0, 1}, accepted_before
    # no retry: a factorisation enqueued again after a time-out of the chain counts twice
    assert run["stats"]["linear_solves"] == 0 and run["end_stats"]["linear_solves"] == len(log) - 1, (run["end_stats"], len(log))
    assert twin["end_stats"]["linear_solves"] == len(twin["log"]) - 1, (twin["end_stats"], len(twin["log"]))
    # the plan
    for stat, (op, value) in c.get("plan", {}).items():
        assert COMPARE[op](run["stats"][stat], value), (stat, run["stats"])
        if stat in ("cholesky_columns_resident", "graph_replay"):   # ... and still at the end: nothing switched the resident chain, or the replay, off
            assert run["end_stats"][stat] == run["stats"][stat], (run["stats"], run["end_stats"])
    retained = None
    if "retained_points" in got:
        retained = got["retained_points"]
        assert len(retained) == run["stats"]["retained_points"] and not set(retained) & set(comp["on_axis"]), retained
    if c.get("replay"):   # the second invalid solve of iteration 1 ran the graph that the first one captured
        assert not log[1]["step_is_valid"] and not log[2]["step_is_valid"]
    # the first valid step after each episode, and the accepted step after it, solve THEIR normal equations
    model = sc.BalModel(fc._prob(c), loss=c.get("loss"), retained=retained)
    scale = sc.jacobi_scale(model, x0)
    accepted = [k for k in range(1, len(log)) if log[k]["step_is_successful"]]
    checked = []
    for _, last in ep:
        k = last + 1
        assert log[k]["step_is_valid"] and log[k]["step_is_successful"], k
        for kk in [k] + [j for j in accepted if j > k][:1]:
            if kk not in checked:
                e = sc.check(model, x0, xs[kk - 1], xs[kk], log, kk, scale=scale, min_lm_diagonal=c["options"]["min_lm_diagonal"])
                print("step_check", name, kk, "eta %.3g floor %.3g" % (e["eta"], e["floor"]), flush=True)
                checked.append(kk)
    # nothing stayed behind: a fresh solver started at the radius of the first valid solve logs the same bits from there on
    k0 = got["first_valid"]
    assert k0 == ep[0][1] + 1 and len(twin["log"]) == len(log) - (k0 - 1), (k0, len(twin["log"]), len(log))
    for j in range(1, len(twin["log"])):
        a, b = twin["log"][j], log[k0 - 1 + j]
        assert bool(a["step_is_valid"]) == bool(b["step_is_valid"]) and bool(a["step_is_successful"]) == bool(b["step_is_successful"]), j
        for f in LOG_BITS:
            assert np.array_equal(fc.bits(a[f]), fc.bits(b[f])), (j, f, a[f], b[f])
    assert np.array_equal(fc.bits(twin["x"]), fc.bits(run["x"]))
    assert twin["termination"] == run["termination"]
