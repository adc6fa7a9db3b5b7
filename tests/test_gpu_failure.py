"""The failure paths of the trust-region loop on the device, through StepSolver, against tests/failure_reference.py: an evaluation
that fails at the start or after an accepted step, candidates that cannot be evaluated, linear solves that are not valid, and
what is written back in each case — on DENSE_QR, DENSE_NORMAL_CHOLESKY, DENSE_SCHUR and dense rows.  The cases, their margins and
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
