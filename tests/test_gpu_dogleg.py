"""DOGLEG on the device against tests/dogleg_reference.py: per iteration cost 1e-10, step norm, gradient max-norm, radius and
relative decrease 1e-8 (relative; the project's tolerances for oracle comparisons), the accepted / rejected pattern equal.  The
cases and why they are what they are: tests/dogleg_cases.py, tests/test_dogleg_cpu.py."""
import numpy as np
import pytest

import skeres_amd as sk
from skeres_amd import bal, dense_synth
import oracle
from helpers import sk_loss
import dogleg_reference as dr
import dogleg_cases as dc

pytestmark = pytest.mark.gpu

DOGLEG_STATS = ("linear_solves", "dogleg_reused_steps", "dogleg_mu", "phase_seconds_2", "dogleg_w_r", "dogleg_m_r", "dogleg_w_w", "dogleg_w_m",
                "dogleg_m_m", "dogleg_g_g", "dogleg_g_p", "dogleg_p_p", "dogleg_a", "dogleg_b")
PLAN_STATS = ("retained_points", "dissected", "cholesky_columns_resident", "graph_replay", "tape_blocks", "host_callback_blocks")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _build(prob, loss=None, subset=False, const_cams=dc.CONST_CAMS, const_pts=(), tape=False, keep=None):
    C = prob.num_cameras
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    if tape:
        from skeres_amd.examples.traced_functors import TracedSnavelyReprojectionError
        f = TracedSnavelyReprojectionError(0.0, 0.0)
        keep.append(f)
        problem.addResidualBlocksTraced(f, prob.observations, None, params, offs)
    else:
        problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations,
                                  sk_loss(loss) if loss else sk.PredefinedLossFunctions.trivialLoss(), params, offs)
    if subset:
        fixed = sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8])
        for i in range(C):
            if i not in const_cams:
                problem.setParameterization(params.slice(9 * i), fixed)
    for i in const_cams:
        problem.setParameterBlockConstant(params.slice(9 * i))
    for q in const_pts:
        problem.setParameterBlockConstant(params.slice(9 * C + 3 * q))
    return problem, params


def _options(kmax, dogleg=True, knobs=None, **opt):
    assert set(opt) <= {"initial_trust_region_radius", "jacobi_scaling"}, opt   # (anything else goes through knobs)
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
    if dogleg:
        o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
        o.setDoglegType(sk.DoglegType.TRADITIONAL_DOGLEG)
    o.setMaxNumIterations(kmax)
    if "initial_trust_region_radius" in opt:
        o.setInitialTrustRegionRadius(opt["initial_trust_region_radius"])
    if "jacobi_scaling" in opt:
        o.setJacobiScaling(opt["jacobi_scaling"])
    for k, v in (knobs or {}).items():
        getattr(o, k)(*v) if isinstance(v, tuple) else getattr(o, k)(v)
    return o


def _stats(solver, names):
    return {nm: solver.stat(nm) for nm in names}   # (a stat the solver does not have raises)


def _solve(problem, params, n, options, names=DOGLEG_STATS, plan_names=PLAN_STATS):
    """Steps a solver to its end.  Returns the log, x after every iteration (x[0]: the start), the named stats after every
    iteration that did not end the solve (stats[0]: after create) and at the end (final), the plan's stats and the full report."""
    solver = sk.StepSolver(options, problem)
    plan = _stats(solver, plan_names)
    xs, stats = [params.toArray(n)], [_stats(solver, names)]
    summary = sk.Solver.Summary()
    while not solver.step():
        solver.finish(summary)
        xs.append(params.toArray(n))
        stats.append(_stats(solver, names))
    solver.finish(summary)
    return dict(log=summary.iterations(), xs=xs, stats=stats, final=_stats(solver, names), plan=plan, report=summary.fullReport())


@pytest.fixture(scope="module")
def runs():
    """The device run of a case under given knobs, once per module."""
    cache = {}

    def run(name, tape=False, **knobs):
        key = (name, tape, tuple(sorted((k, repr(v)) for k, v in knobs.items())))
        if key not in cache:
            c, prob = dc.CASES[name], dc.problem(name)
            keep = []
            problem, params = _build(prob, loss=c.get("loss"), subset=c.get("subset", False), const_pts=c.get("const_pts", ()), tape=tape, keep=keep)
            cache[key] = _solve(problem, params, prob.num_parameters, _options(c["kmax"], knobs=knobs, **c.get("options", {})))
        return cache[key]
    return run


def _against_reference(name, run):
    dc.compare_logs(run["log"], dc.reference(name)[1], dc.CASES[name]["kmax"], show=name)
    assert "DOGLEG (TRADITIONAL)" in run["report"] and "LEVENBERG_MARQUARDT" not in run["report"]
    assert run["plan"]["graph_replay"] == 0


@pytest.mark.parametrize("name", ["small", "small-radius-1", "rejecting"])
def test_auto_plan_trajectories(runs, name):
    _against_reference(name, runs(name))


# the forced plans on (150, 3000, 14000) from the default radius (Gauss-Newton steps inside the region), and the two that bear on
# the new kernels from radius 1 as well (truncated Cauchy steps, then an interpolated one: tests/dogleg_cases.py)
FORCED = {"retained": ("plans", {"setRetainedPoints": ("on", 4)}), "dissection": ("plans", {"setCholeskyDissection": "on"}),
          "resident-off": ("plans", {"setResidentKernels": False}), "jacobi-off": ("plans-jacobi-off", {}),
          "retained-radius-1": ("plans-radius-1", {"setRetainedPoints": ("on", 4)}), "jacobi-off-radius-1": ("plans-jacobi-off-radius-1", {})}


@pytest.mark.parametrize("variant", sorted(FORCED))
def test_forced_plans_trajectories(runs, variant):
    name, knobs = FORCED[variant]
    run = runs(name, **knobs)
    print(variant, run["plan"], flush=True)
    if variant.startswith("retained"):
        assert run["plan"]["retained_points"] == 3   # (a pseudo-camera holds three points)
    if variant == "dissection":
        assert run["plan"]["dissected"] == 1
    if variant == "resident-off":
        assert run["plan"]["cholesky_columns_resident"] == 0
    _against_reference(name, run)


@pytest.mark.parametrize("name", ["robust", "robust-radius-1"])
def test_robust_loss_subset_and_constant_point(runs, name):
    run = runs(name)
    _against_reference(name, run)
    free = dc.model(name).free
    x0 = dc.problem(name).parameters
    assert (~free).sum() == 63
    for x in run["xs"]:
        assert np.array_equal(x[~free], x0[~free])      # bitwise
    assert not np.array_equal(run["xs"][-1][free], x0[free])


def test_tape_functor(runs):
    run = runs("small-radius-1", tape=True)
    assert run["plan"]["tape_blocks"] == dc.problem("small-radius-1").num_observations
    _against_reference("small-radius-1", run)


def test_graph_replay_option_runs_launch_by_launch():
    """BAL-49's shape replays its LM iteration as a hipGraph; under DOGLEG the launches are enqueued one by one whatever the option says."""
    prob = bal.generate(49, 7776, 31843, seed=49)
    out = []
    for on in (True, False):
        problem, params = _build(prob)
        out.append(_solve(problem, params, prob.num_parameters, _options(3, knobs={"setGraphReplay": on})))
        assert out[-1]["plan"]["graph_replay"] == 0
    dc.compare_logs(out[0]["log"], out[1]["log"], 3, tol={f: 1e-10 for f in dc.TOL}, show="bal49")
    problem, params = _build(prob)
    lm = sk.StepSolver(_options(3, dogleg=False, knobs={"setGraphReplay": True}), problem)
    assert lm.stat("graph_replay") == 1                # (what the option does for Levenberg-Marquardt)


def test_rejected_steps_reuse_the_factorisation(runs):
    run, ref = runs("rejecting"), dc.reference("rejecting")[1]
    st = run["stats"]
    assert len(st) == 8
    followers = [k for k in range(2, 8) if not ref[k - 1]["step_is_successful"]]
    assert followers == [6, 7]
    for k in followers:   # the iteration that follows a rejection: no factorisation, nothing in the Cholesky phase
        assert st[k]["linear_solves"] == st[k - 1]["linear_solves"], k
        assert st[k]["phase_seconds_2"] == st[k - 1]["phase_seconds_2"], k
        assert st[k]["dogleg_reused_steps"] == st[k - 1]["dogleg_reused_steps"] + 1
    for k in range(1, 6):
        assert st[k]["linear_solves"] == st[k - 1]["linear_solves"] + 1 and st[k]["phase_seconds_2"] > st[k - 1]["phase_seconds_2"]
    assert st[7]["dogleg_reused_steps"] == sum(1 for e in ref[1:] if e["reused"]) == 2
    assert st[7]["dogleg_mu"] == pytest.approx(1e-8)


@pytest.mark.parametrize("which", ["rejecting", "small-radius-1", "robust", "robust-radius-1"] + sorted(FORCED))
def test_identities_of_the_products(runs, which):
    """Per linear solve w . r = -|g_hat|^2; per accepted step the model cost change from the five products and (a, b) equals
    -m . (r + m / 2), m formed in long double at the device's own step (x_k - x_{k-1})."""
    name, knobs = FORCED.get(which, (which, {}))
    run, model = runs(name, **knobs), dc.model(name)
    jac = dc.CASES[name].get("options", {}).get("jacobi_scaling", True)
    checked = 0
    for k in range(1, len(run["xs"])):
        s = run["stats"][k]
        print(which, k, s, flush=True)
        assert abs(s["dogleg_w_r"] + s["dogleg_g_g"]) <= 1e-10 * s["dogleg_g_g"], k
        branch = dc.reference(name)[1][k]["branch"]   # the device took the reference's branch
        assert (a_b_of(s) == (0.0, 1.0)) == (branch == "gn") and (s["dogleg_b"] == 0.0) == (branch == "cauchy"), (k, branch)
        if not run["log"][k]["step_is_successful"]:
            assert np.array_equal(run["xs"][k], run["xs"][k - 1])
            continue
        a, b = s["dogleg_a"], s["dogleg_b"]
        mcc = -(a * s["dogleg_w_r"] + b * s["dogleg_m_r"] + 0.5 * (a * a * s["dogleg_w_w"] + 2 * a * b * s["dogleg_w_m"] + b * b * s["dogleg_m_m"]))
        want = dr.model_cost_change(model, run["xs"][0], run["xs"][k - 1], run["xs"][k], jac)
        print(which, k, "model cost change %.17g / %.17g" % (mcc, want), flush=True)
        assert abs(mcc - want) <= 1e-10 * abs(want), (k, mcc, want)
        assert abs(run["log"][k]["cost_change"] / run["log"][k]["relative_decrease"] - want) <= 1e-10 * abs(want)
        checked += 1
    assert checked == sum(1 for e in dc.reference(name)[1][1:] if e["step_is_successful"]) >= 2


def a_b_of(s):
    return s["dogleg_a"], s["dogleg_b"]


def _dense_sk_problem(name):
    sizes, _, x0 = dc.dense_problem(name)
    x = sk.DoubleArray(len(x0))
    x.copyFrom(x0)
    problem = sk.Problem()
    if name == "powell":
        problem.addResidualBlock(sk.PowellF1().toAutoDiffCostFunction(), None, x, x.slice(1))
        problem.addResidualBlock(sk.PowellF2().toAutoDiffCostFunction(), None, x.slice(2), x.slice(3))
        problem.addResidualBlock(sk.PowellF3().toAutoDiffCostFunction(), None, x.slice(1), x.slice(2))
        problem.addResidualBlock(sk.PowellF4().toAutoDiffCostFunction(), None, x, x.slice(3))
    else:
        from helpers import curve_fitting_data
        for xv, yv in curve_fitting_data():
            problem.addResidualBlock(sk.ExponentialResidual(xv, yv).toAutoDiffCostFunction(), None, x, x.slice(1))
    return problem, x, len(x0)


@pytest.mark.parametrize("solver", ["DENSE_QR", "DENSE_NORMAL_CHOLESKY"])
@pytest.mark.parametrize("name", ["powell", "curve-fitting"])
def test_dense_jacobian_path(name, solver):
    """EX/Powell.scala and EX/CurveFitting.scala under DOGLEG; curve fitting takes eleven candidates from its first factorisation."""
    kmax = dc.DENSE_CASES[name]["kmax"]
    ref = dc.dense_reference(name)[1]
    problem, x, n = _dense_sk_problem(name)
    o = _options(kmax)
    o.setLinearSolverType(getattr(sk.LinearSolverType, solver))
    solver_ = sk.StepSolver(o, problem)
    stats = [_stats(solver_, DOGLEG_STATS)]
    while not solver_.step():
        stats.append(_stats(solver_, DOGLEG_STATS))
    summary = sk.Solver.Summary()
    solver_.finish(summary)
    assert summary.linearSolverTypeUsed() == getattr(sk.LinearSolverType, solver) and "DOGLEG (TRADITIONAL)" in summary.fullReport()
    dc.compare_logs(summary.iterations(), ref, kmax, show="%s-%s" % (name, solver))
    assert stats[-1]["dogleg_reused_steps"] == sum(1 for e in ref[1:] if e["reused"])
    assert stats[-1]["linear_solves"] == sum(1 for e in ref[1:] if not e["reused"])
    for k in range(1, kmax + 1):
        if ref[k]["reused"]:
            assert stats[k]["linear_solves"] == stats[k - 1]["linear_solves"] and stats[k]["phase_seconds_2"] == stats[k - 1]["phase_seconds_2"], k
        assert abs(stats[k]["dogleg_w_r"] + stats[k]["dogleg_g_g"]) <= 1e-10 * stats[k]["dogleg_g_g"], k


def test_powell_converges_on_the_device():
    problem, x, n = _dense_sk_problem("powell")
    o = _options(200)
    o.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
    o.setFunctionTolerance(0.0)
    o.setParameterTolerance(0.0)
    o.setGradientTolerance(1e-30)
    summary = sk.Solver.Summary()
    sk.ceres.solve(o, problem, summary)
    assert summary.finalCost() < 1e-20, summary.finalCost()


def test_levenberg_marquardt_is_untouched():
    prob = bal.generate(16, 600, 2600, seed=11)
    logs = []
    for mention in (False, True):
        problem, params = _build(prob, const_cams=())
        o = sk.Solver.Options()
        o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
        if mention:
            o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.LEVENBERG_MARQUARDT)
            o.setDoglegType(sk.DoglegType.TRADITIONAL_DOGLEG)
        run = _solve(problem, params, prob.num_parameters, o, names=("linear_solves", "dogleg_reused_steps"))
        logs.append([it["cost"] for it in run["log"]])
        assert run["final"]["linear_solves"] == len(run["log"]) - 1 and run["final"]["dogleg_reused_steps"] == 0
        assert "LEVENBERG_MARQUARDT" in run["report"] and run["plan"]["graph_replay"] == 1
    assert logs[0] == logs[1] and len(logs[0]) > 3    # bitwise


def _host_snavely_functor():
    """EX/SimpleBundleAdjuster.scala:79-119 with Rotation.scala:449-522 written out, as HOST code over a generic T
    (floats or rotation.Jet): what a user's own (9, 3) -> 2 functor looks like to the library."""
    from skeres_amd import rotation as R

    def rotate(w, pt):
        theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        if float(theta2) > np.finfo(np.float64).eps:
            theta = R.sqrt(theta2)
            c, s_ = R.cos(theta), R.sin(theta)
            ti = 1.0 / theta
            wn = [w[0] * ti, w[1] * ti, w[2] * ti]
            wxp = [wn[1] * pt[2] - wn[2] * pt[1], wn[2] * pt[0] - wn[0] * pt[2], wn[0] * pt[1] - wn[1] * pt[0]]
            tmp = (wn[0] * pt[0] + wn[1] * pt[1] + wn[2] * pt[2]) * (1.0 - c)
            return [pt[i] * c + wxp[i] * s_ + wn[i] * tmp for i in range(3)]
        wxp = [w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]]
        return [pt[i] + wxp[i] for i in range(3)]

    class HostSnavely(sk.HostAutoDiffCostFunctor):
        def __init__(self, ox, oy):
            super().__init__(2, 9, 3)
            self.ox, self.oy = ox, oy

        def apply(self, camera, point):
            p = rotate(camera[0:3], point)
            p = [p[0] + camera[3], p[1] + camera[4], p[2] + camera[5]]
            xp, yp = -p[0] / p[2], -p[1] / p[2]
            r2 = xp * xp + yp * yp
            distortion = 1.0 + r2 * (camera[7] + camera[8] * r2)
            return [(camera[6] * distortion) * xp - self.ox, (camera[6] * distortion) * yp - self.oy]
    return HostSnavely


def _refused(options, problem):
    with pytest.raises(sk.SkeresError, match="status 4") as e:   # SK_ERR_UNSUPPORTED
        sk.StepSolver(options, problem)
    assert "not supported" in str(e.value)
    summary = sk.Solver.Summary()
    with pytest.raises(sk.SkeresError, match="not supported"):
        sk.ceres.solve(options, problem, summary)


def test_refusals():
    prob = dc.problem("small")
    # SUBSPACE_DOGLEG
    problem, params = _build(prob)
    o = _options(3)
    o.setDoglegType(sk.DoglegType.SUBSPACE_DOGLEG)
    _refused(o, problem)
    # a world of two ranks
    o = _options(3)
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    _refused(o, problem)
    # dense rows
    consts, _ = dense_synth.generate(100, 30, seed=3)
    x = sk.DoubleArray(30)
    x.copyFrom(np.zeros(30))
    rows = sk.Problem()
    rows.addDenseRows(oracle.SYNTH_TANH_ROW, consts, None, x, 30)
    o = _options(3)
    o.setLinearSolverType(sk.LinearSolverType.DENSE_NORMAL_CHOLESKY)
    _refused(o, rows)
    # tangent-space blocks (here: a constant block) on the dense Jacobian path
    dense, x, _ = _dense_sk_problem("powell")
    dense.setParameterBlockConstant(x.slice(3))
    o = _options(3)
    o.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
    _refused(o, dense)
    # host-evaluated residual blocks under DENSE_SCHUR
    HostSnavely = _host_snavely_functor()
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    host = sk.Problem()
    keep = []
    loss = sk.PredefinedLossFunctions.trivialLoss()
    for i in range(prob.num_observations):
        ox, oy = prob.observations[i]
        cf = HostSnavely(ox, oy).toAutoDiffCostFunction() if i % 4 == 0 else sk.SnavelyReprojectionError(ox, oy).toAutoDiffCostFunction()
        keep.append(cf)
        host.addResidualBlock(cf, loss, params.slice(9 * int(prob.camera_index[i])), params.slice(9 * prob.num_cameras + 3 * int(prob.point_index[i])))
    _refused(_options(3), host)
    # the options that were refused still solve under Levenberg-Marquardt
    summary = sk.Solver.Summary()
    sk.ceres.solve(_options(3, dogleg=False), host, summary)
    assert summary.finalCost() < summary.initialCost()


def test_mu_loop_after_factorisations_that_fail(tmp_path):
    """Case i-dogleg (tests/dogleg_cases.py): the damped system is not positive definite at the first mu of iterations 1, 2 and 4 — a
    zero pivot in a point block, NaN rows of S, info raised, the resident chain and back-substitution running on NaN — and the loop
    factors again at ten times mu, up to five times, inside the same iteration.  The log to the reference; the number of linear solves
    of every iteration and mu after it as the reference has them (a retry after a time-out of the chain would count as a solve more);
    every iteration valid; the silent component by its bits.  The device run is tests/dogleg_worker.py's, in a process of its own."""
    import os
    import pickle
    import subprocess
    import sys
    import failure_cases as fc
    name = "i-dogleg"
    c, prob = dc.CASES[name], dc.problem(name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "run.pickle")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "dogleg_worker.py"), name, path], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DOGLEG_WORKER_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "timed out" not in out.stderr, out.stderr[-3000:]
    with open(path, "rb") as f:
        run = pickle.load(f)
    ref = dc.reference(name)[1]
    _against_reference(name, run)
    assert run["plan"]["cholesky_columns_resident"] > 0
    stats = run["stats"] + [run["final"]] * (c["kmax"] + 1 - len(run["stats"]))
    solves = [int(stats[k]["linear_solves"] - stats[k - 1]["linear_solves"]) for k in range(1, c["kmax"] + 1)]
    print(name, "linear solves per iteration", solves, "mu", [stats[k]["dogleg_mu"] for k in range(c["kmax"] + 1)], flush=True)
    assert solves == [e["solves"] for e in ref[1:]] == list(c["solves"])
    for k in range(1, c["kmax"] + 1):
        assert run["log"][k]["step_is_valid"] and run["log"][k]["step_is_successful"], k
        assert stats[k]["dogleg_mu"] == pytest.approx(ref[k]["mu"], rel=1e-12), k
    # the component never moves (its gradient is exactly zero), whatever ran on NaN before the factorisation that held
    cols = dc.silent_component(name)[1]
    assert len(run["xs"]) >= c["kmax"]
    for x in run["xs"][1:]:
        assert np.array_equal(fc.bits(x[cols]), fc.bits(prob.parameters[cols]))
        assert not np.array_equal(x, prob.parameters)
