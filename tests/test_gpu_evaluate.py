"""Problem::Evaluate on the device (sk_problem_evaluate) against the numpy reference of tests/evaluate_reference.py on the cases of
tests/evaluate_cases.py: every case, equal bytes on a repeated call, every combination of NULL outputs, consistency with the
solvers' own iteration 0, a failing callback, and the JNI thunks through the mock JVM.

SKERES_EVALUATE_ERROR_FILE=<path>: the largest observed ratio to each bound, per case, is appended there
(profiles/evaluate_error.txt is such a record)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import skeres_amd as sk
from evaluate_cases import CASES, case
from evaluate_reference import check, reference_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _got(out):
    got = {k: out[k] for k in ("cost", "residuals", "gradient") if k in out}
    if "jacobian" in out:
        got.update(rows=out["jacobian"].rows, cols=out["jacobian"].cols, values=out["jacobian"].values)
    return got


def _record(name, ratios):
    line = "%-20s %s" % (name, "  ".join("%s %.3e" % (k, ratios[k]) for k in ("residuals", "jacobian", "gradient", "cost") if k in ratios))
    print(line)
    path = os.environ.get("SKERES_EVALUATE_ERROR_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_reference(name):
    c = case(name)
    problem, options, params, keep = c.build()
    out = problem.evaluate(options)
    ratios = check(reference_of(name), _got(out), c)
    _record(name, ratios)
    assert np.array_equal(params.toArray(len(c.x)), c.x)   # the point is read, never written


def test_two_calls_return_the_same_bytes():
    c = case("bal_small")
    problem, options, params, keep = c.build()
    a, b = problem.evaluate(options), problem.evaluate(options)
    assert a["cost"].hex() == b["cost"].hex()
    for k in ("residuals", "gradient"):
        assert a[k].tobytes() == b[k].tobytes()
    assert a["jacobian"].values.tobytes() == b["jacobian"].values.tobytes()


def test_every_combination_of_null_outputs():
    c = case("curve_robust")
    ref = reference_of("curve_robust")
    problem, options, params, keep = c.build()
    full = problem.evaluate(options)
    plain = problem.evaluate(options, True, True, False, False)   # no Jacobian path: the functors run in double, not on Jets
    for want in itertools.product([False, True], repeat=4):
        out = problem.evaluate(options, *want)
        assert set(out) == {k for k, w in zip(("cost", "residuals", "gradient", "jacobian"), want) if w}
        check(ref, _got(out), c)
        # what is asked for does not depend on what else is asked for, bit for bit, among the calls that form a Jacobian and among
        # those that do not
        same = full if (want[2] or want[3]) else plain
        if want[0]:
            assert out["cost"].hex() == same["cost"].hex()
        if want[1]:
            assert out["residuals"].tobytes() == same["residuals"].tobytes()
        if want[2]:
            assert out["gradient"].tobytes() == full["gradient"].tobytes()
        if want[3]:
            assert out["jacobian"].values.tobytes() == full["jacobian"].values.tobytes()


@pytest.mark.parametrize("name,solver", [("curve_robust", "DENSE_QR"), ("bal_small", "DENSE_SCHUR")])
def test_iteration_0_of_the_solver_agrees(name, solver):
    """sk_solver_create + finish: the iteration-0 cost is Evaluate's cost (1e-11 relative) and gradient_max_norm is max_j |gradient_j|
    (1e-10 relative) — the solver's figure is the same J^T r, unscaled."""
    c = case(name)
    problem, options, params, keep = c.build()
    out = problem.evaluate(options, jacobian=False)
    o = sk.Solver.Options()
    o.setLinearSolverType(getattr(sk.LinearSolverType, solver))
    step = sk.StepSolver(o, problem)
    summary = sk.Solver.Summary()
    step.finish(summary)
    it0 = summary.iterations()[0]
    gmax = float(np.max(np.abs(out["gradient"])))
    print(name, it0["cost"], out["cost"], it0["gradient_max_norm"], gmax)
    assert abs(it0["cost"] - out["cost"]) <= 1e-11 * abs(out["cost"])
    assert abs(it0["gradient_max_norm"] - gmax) <= 1e-10 * gmax


def test_a_failing_callback_is_reported():
    from evaluate_cases import bal_host
    problem, options, params, keep = bal_host(failing=True).build()
    cost = C.c_double()
    rc = sk.lib().sk_problem_evaluate(problem._h, None, C.byref(cost), None, None, None)
    assert rc == 5 and b"reported failure" in sk.lib().sk_last_error()


def test_powell_through_the_jni_thunks(tmp_path_factory, built):
    """skEvaluateOptions* / skProblemEvaluate* of bindings/jni/skeres_amd_jni.c against the mock JNIEnv of tests/jni_stub, as
    CeresProblem.evaluate of Native.scala calls them."""
    from test_jni_mock import Jni, K_DOUBLE, K_INT, K_LONG, ROOT
    import subprocess
    lib = str(tmp_path_factory.mktemp("jni_evaluate") / "libskeres_amd_jni_mock.so")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "bindings", "jni", "skeres_amd_jni.c"), os.path.join(ROOT, "tests", "jni_stub", "mock_jvm.c"),
           "-L", os.path.join(ROOT, "skeres_amd"), "-lskeres_amd", "-Wl,-rpath," + os.path.join(ROOT, "skeres_amd"), "-o", lib]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    jni = Jni(lib)
    c = case("powell")
    ref = reference_of("powell")
    x = jni.call("skArrayNew", 4)
    jni.call("skArrayCopyIn", x, jni.array(K_DOUBLE, c.x), 4, restype=None)
    problem, costs = jni.call("skProblemNew"), []
    for fid, consts, pbs, loss, kind in c.blocks:
        cost = jni.call("skCostFunctionNewAutodiff", fid, jni.array(K_DOUBLE, []))
        v = jni.call("skPtrvecNew")
        for b in pbs:
            jni.call("skPtrvecAdd", v, jni.call("skArraySlice", x, b), restype=None)
        jni.call("skProblemAddResidualBlock", problem, cost, 0, v)
        jni.call("skPtrvecFree", v, restype=None)
        costs.append(cost)
    assert jni.exception() is None
    o = jni.call("skEvaluateOptionsNew")
    assert jni.call("skEvaluateOptionsSetApplyLossFunction", o, 1, restype=C.c_int) == 0
    sizes = jni.array(K_LONG, [0, 0, 0])
    assert jni.call("skProblemEvaluateSizes", problem, o, sizes, restype=C.c_int) == 0
    num_rows, num_cols, nnz = (int(v) for v in jni.array_values(sizes, K_LONG, 3))
    assert (num_rows, num_cols, nnz) == (4, 4, 8)
    rows, cols = jni.array(K_INT, np.zeros(num_rows + 1)), jni.array(K_INT, np.zeros(nnz))
    assert jni.call("skProblemEvaluateStructure", problem, o, rows, cols, restype=C.c_int) == 0
    cost, r, g, v = (jni.array(K_DOUBLE, np.zeros(n)) for n in (1, num_rows, num_cols, nnz))
    assert jni.call("skProblemEvaluate", problem, o, cost, r, g, v, restype=C.c_int) == 0 and jni.exception() is None
    got = {"cost": float(jni.array_values(cost, K_DOUBLE, 1)[0]), "residuals": jni.array_values(r, K_DOUBLE, num_rows),
           "gradient": jni.array_values(g, K_DOUBLE, num_cols), "values": jni.array_values(v, K_DOUBLE, nnz),
           "rows": jni.array_values(rows, K_INT, num_rows + 1), "cols": jni.array_values(cols, K_INT, nnz)}
    check(ref, got, c)
    # null outputs and null options; an id out of range is an IllegalArgumentException
    assert jni.call("skProblemEvaluate", problem, 0, cost, None, None, None, restype=C.c_int) == 0
    assert float(jni.array_values(cost, K_DOUBLE, 1)[0]) == got["cost"]
    assert jni.call("skEvaluateOptionsSetResidualBlocks", o, jni.array(K_INT, [7]), restype=C.c_int) == 0
    assert jni.call("skProblemEvaluateSizes", problem, o, sizes, restype=C.c_int) != 0
    assert jni.exception()[0] == "java/lang/IllegalArgumentException"
    for cf in costs:
        jni.call("skCostFunctionFree", cf, restype=None)
    for h, free in ((o, "skEvaluateOptionsFree"), (problem, "skProblemFree"), (x, "skArrayFree")):
        jni.call(free, h, restype=None)
    assert jni.clean()


def test_launch_timing_reports_the_phases_of_the_last_call():
    c = case("wide_column")
    problem, _, params, keep = c.build()
    options = sk.Problem.EvaluateOptions()
    assert options.launchSeconds() == [0.0] * 6
    options.setLaunchTiming(True)
    timed = problem.evaluate(options)
    seconds = options.launchSeconds()   # uploads, evaluation, finish, gradient, cost, downloads
    assert all(0.0 <= s < 1.0 for s in seconds) and seconds[1] > 0 and seconds[2] > 0 and seconds[3] > 0
    plain = problem.evaluate()
    assert timed["jacobian"].values.tobytes() == plain["jacobian"].values.tobytes() and timed["gradient"].tobytes() == plain["gradient"].tobytes()
