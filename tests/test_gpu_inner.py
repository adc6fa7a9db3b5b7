"""Inner iterations on the device (sk_options_set_use_inner_iterations under CGNR) against tests/inner_reference.py, which solves the
blocks one after the other: per LM iteration the accepted / rejected pattern, the number of CG iterations and the lock-step rounds
equal, cost at 1e-10, step norm, gradient max-norm, radius and relative decrease at 1e-8 (cgnr_cases.TOL); after the first
refinement every block's inner iteration count and status equal and the refined point at 1e-8.  The cases and why they are what
they are: tests/inner_cases.py, tests/test_inner_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skeres_amd as sk
import cgnr_cases as cc
import inner_cases as k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("cg_iterations", "linear_solves", "inner_iteration_steps", "inner_iteration_rounds", "inner_iterations_enabled", "inner_iteration_groups")
POINT_TOL = 1e-8   # |a - b| <= POINT_TOL (|b| + 1) per coordinate: the project's tolerance for a step, absolute below 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _solve(name, inner=True, schur=None, **override):
    """Steps a solver to its end.  Returns the log, x after every iteration (xs[0]: the start), the blocks' inner iterations and
    statuses after the first iteration, the stats at the end and the report."""
    problem, params, n, keep = k.build_device(name)
    o = k.device_options(name, inner, schur, **override)
    if inner:
        k.set_caller_ordering(name, o, params)
    solver = sk.StepSolver(o, problem)
    xs, blocks = [params.toArray(n)], None
    summary = sk.Solver.Summary()
    while not solver.step():
        solver.finish(summary)
        xs.append(params.toArray(n))
        if inner and blocks is None:
            blocks = solver.innerIterationBlocks()
    solver.finish(summary)
    if inner and blocks is None:
        blocks = solver.innerIterationBlocks()
    return dict(log=summary.iterations(), xs=xs, blocks=blocks, final={nm: solver.stat(nm) for nm in STATS}, report=summary.fullReport(), summary=summary)


@pytest.fixture(scope="module")
def runs():
    """The device run of a case, once per module."""
    cache = {}

    def run(name, inner=True, schur=None, **override):
        key = (name, inner, schur, tuple(sorted(override.items())))
        if key not in cache:
            cache[key] = _solve(name, inner, schur, **override)
        return cache[key]
    return run


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_trajectories(runs, name):
    run, ref = runs(name), k.reference(name)[1]
    kmax = len(ref) - 1
    for i in range(kmax + 1):
        print("%s k=%d rounds %d / %d" % (name, i, run["log"][i]["inner_iteration_rounds"] if i < len(run["log"]) else -1, ref[i]["inner_iteration_rounds"]), flush=True)
    cc.compare_logs(run["log"], ref, kmax, show=name)
    for i in range(kmax + 1):
        assert int(run["log"][i]["inner_iteration_rounds"]) == ref[i]["inner_iteration_rounds"], i
    refined = [e for e in ref if e["inner_blocks"] is not None]
    assert run["final"]["inner_iteration_steps"] == len(refined) >= 1
    assert run["final"]["inner_iteration_rounds"] == sum(e["inner_iteration_rounds"] for e in ref)
    assert run["final"]["inner_iteration_groups"] == len(k.groups(name))
    # the first refinement: every block's iterations and status, the refined point (iteration 1 is refined in every case)
    assert ref[1]["inner_blocks"] is not None and ref[1]["step_is_successful"]
    order, (its, status) = k.problem_order(name), run["blocks"]
    in_groups = {b for g in k.groups(name) for b in g}
    assert set(ref[1]["inner_blocks"]) == in_groups
    for b in range(len(order)):
        want = ref[1]["inner_blocks"].get(b, (-1, -1))
        assert (int(its[order[b]]), int(status[order[b]])) == tuple(want), (b, its[order[b]], status[order[b]], want)
    x, want = run["xs"][1], ref[1]["refined_point"]
    err = np.abs(x - want) / (np.abs(want) + 1)
    print("%s: refined point, largest deviation %.3e" % (name, float(np.max(err))), flush=True)
    assert float(np.max(err)) <= POINT_TOL
    line = [ln for ln in run["report"].splitlines() if ln.startswith("Inner iterations")]
    assert len(line) == 1 and ("%d groups" % len(k.groups(name))) in line[0] and ("%d rounds" % run["final"]["inner_iteration_rounds"]) in line[0]


def test_write_back_returns_the_refined_point(runs):
    """x after iteration 1 is the refined candidate, not the trust-region step's: it differs from the run without the option."""
    for name in ("bal-small", "quaternion"):
        on, off = runs(name), runs(name, False)
        assert off["log"][1]["step_is_successful"] and not np.array_equal(on["xs"][1], off["xs"][1])
        assert on["log"][1]["cost"] < off["log"][1]["cost"]


def test_tolerance_switches_the_refinement_off(runs):
    run = runs("bal-tolerance")
    rounds = [int(e["inner_iteration_rounds"]) for e in run["log"]]
    assert rounds[1] > 0 and all(r == 0 for r in rounds[2:]) and len(rounds) == 4
    assert run["final"]["inner_iterations_enabled"] == 0 and run["final"]["inner_iteration_steps"] == 1 and "switched off" in run["report"]
    assert runs("bal-small")["final"]["inner_iterations_enabled"] == 1


def test_two_solves_return_the_same_bytes(runs):
    for name in ("bal-robust", "chain"):
        a, b = runs(name), _solve(name)
        assert len(a["xs"]) == len(b["xs"])
        for xa, xb in zip(a["xs"], b["xs"]):
            assert np.array_equal(xa, xb)
        assert [e["cost"] for e in a["log"]] == [e["cost"] for e in b["log"]]


def test_same_bytes_for_every_batch_size(tmp_path):
    """bal-small and chain with SK_INNER_BATCH = 1, 3 and the default: x after every LM iteration bitwise equal.  The developer
    variables are read once per process, so each setting runs in a process of its own (tests/inner_worker.py)."""
    worker = os.path.join(ROOT, "tests", "inner_worker.py")
    got = {}
    for mode in ("1", "3", ""):
        path = str(tmp_path / ("batch_%s.npz" % (mode or "default")))
        env = dict(os.environ)
        env.pop("SK_INNER_BATCH", None)
        if mode:
            env["SK_INNER_BATCH"] = mode
        out = subprocess.run([sys.executable, worker, path, "bal-small", "chain"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        got[mode] = np.load(path)
    for name in ("bal-small", "chain"):
        for mode in ("1", "3"):
            assert np.array_equal(got[mode][name + "/xs"], got[""][name + "/xs"]), (name, mode)
            assert np.array_equal(got[mode][name + "/rounds"], got[""][name + "/rounds"])
        assert got[""][name + "/rounds"][1] > 0 and not np.array_equal(got[""][name + "/xs"][0], got[""][name + "/xs"][-1])


def test_option_off_is_the_parent_path(runs):
    """With the option explicitly off, x after every iteration equals the run that never names it, bitwise, with the elimination
    on and off; the report has no inner-iterations line."""
    for name, schur in (("bal-robust", False), ("bal-robust", True), ("chain", False), ("quaternion", True)):
        off, default = runs(name, False, schur), runs(name, None, schur)
        assert len(off["xs"]) == len(default["xs"]) > 1
        for xa, xb in zip(off["xs"], default["xs"]):
            assert np.array_equal(xa, xb)
        assert [e["cost"] for e in off["log"]] == [e["cost"] for e in default["log"]]
        assert all(int(e["inner_iteration_rounds"]) == 0 for e in off["log"])
        assert off["final"]["inner_iteration_steps"] == 0 and off["final"]["inner_iterations_enabled"] == 0
        assert off["report"].splitlines()[:12] == default["report"].splitlines()[:12] and "Inner iterations" not in off["report"] + default["report"]
