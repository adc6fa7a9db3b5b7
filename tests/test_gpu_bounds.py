"""Parameter bounds on the device against tests/bounds_reference.py: per iteration cost 1e-10, step norm, gradient max-norm, radius
and relative decrease 1e-8 (relative; the project's tolerances for oracle comparisons); exactly equal: the accepted / rejected
pattern, the line search's alpha, the number of candidate costs and the active bounds.  The cases and the conditions they were
chosen under: tests/bounds_cases.py, tests/test_bounds_cpu.py."""
import numpy as np
import pytest

import skeres_amd as sk
from skeres_amd import bal, dense_synth
import oracle
from helpers import sk_loss
import bounds_reference as br
import bounds_cases as bc

pytestmark = pytest.mark.gpu

STATS = ("active_bounds", "line_search_evaluations", "bounded_coordinates")
PLAN_STATS = ("retained_points", "graph_replay", "tape_blocks")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _set_box(problem, params, offsets, sizes, lo, hi):
    """Every finite bound of (lo, hi) through the setters; offsets / sizes: the parameter blocks inside `params`."""
    for off, size in zip(offsets, sizes):
        for k in range(size):
            if np.isfinite(lo[off + k]):
                problem.setParameterLowerBound(params.slice(off), k, lo[off + k])
            if np.isfinite(hi[off + k]):
                problem.setParameterUpperBound(params.slice(off), k, hi[off + k])


def _build(prob, box=None, loss=None, subset=False, const_cams=bc.CONST_CAMS, const_pts=(), tape=False, keep=None):
    C, P = prob.num_cameras, prob.num_points
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
    if box is not None:
        _set_box(problem, params, [9 * i for i in range(C)] + [9 * C + 3 * q for q in range(P)], [9] * C + [3] * P, *box)
    return problem, params


def _options(kmax, solver="DENSE_SCHUR", knobs=None, **opt):
    o = sk.Solver.Options()
    o.setLinearSolverType(getattr(sk.LinearSolverType, solver))
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


def _solve(problem, params, n, options, plan_names=PLAN_STATS):
    """Steps a solver to its end.  Returns the log, x after every iteration (xs[0]: after create — the caller's array is written
    by finish only, so xs[0] is read through a finish of its own), the stats after every iteration and the plan's."""
    solver = sk.StepSolver(options, problem)
    plan = _stats(solver, plan_names)
    summary = sk.Solver.Summary()
    solver.finish(summary)
    xs, stats = [params.toArray(n)], [_stats(solver, STATS)]
    done = False
    while not done:
        done = solver.step()
        solver.finish(summary)
        if len(summary.iterations()) > len(xs):
            xs.append(params.toArray(n))
            stats.append(_stats(solver, STATS))
    return dict(log=summary.iterations(), xs=xs, stats=stats, plan=plan, summary=summary)


@pytest.fixture(scope="module")
def runs():
    """The device run of a case, once per module."""
    cache = {}

    def run(name, bounded=True, kmax=None, again=False, **more):
        key = (name, bounded, kmax, again, tuple(sorted(more.items())))
        if key not in cache:
            c, prob = bc.CASES[name], bc.problem(name)
            keep = []
            problem, params = _build(prob, box=bc.box(name) if bounded else None, loss=c.get("loss"), subset=c.get("subset", False),
                                     const_pts=c.get("const_pts", ()), tape=c.get("tape", False), keep=keep)
            cache[key] = _solve(problem, params, prob.num_parameters,
                                _options(c["kmax"] if kmax is None else kmax, knobs=dict(c.get("knobs") or {}, **more), **c.get("options", {})))
        return cache[key]
    return run


def _check_run(name, run, ref, lo, hi):
    kmax = bc.kmax_of(name)
    bc.compare_logs(run["log"], ref, kmax, show=name)
    assert len(run["stats"]) == len(run["xs"]) == kmax + 1
    total = 0
    for k in range(kmax + 1):
        print(name, k, run["stats"][k], "reference active", ref[k]["active_bounds"], flush=True)
        assert run["stats"][k]["active_bounds"] == ref[k]["active_bounds"], k
        total += int(ref[k]["line_search_evaluations"]) if k else 0
        assert run["stats"][k]["line_search_evaluations"] == total, k
        x = run["xs"][k]
        assert np.all(x >= lo) and np.all(x <= hi), k                 # feasible after every iteration, exactly
        assert int(np.sum((x == lo) | (x == hi))) == ref[k]["active_bounds"], k
    assert run["stats"][0]["bounded_coordinates"] == int(np.sum(np.isfinite(lo) | np.isfinite(hi)))


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_trajectories(runs, name):
    run = runs(name)
    _check_run(name, run, bc.reference(name)[1], *bc.box(name))
    assert run["plan"]["graph_replay"] == 0                           # under bounds: launch by launch
    if "retained" in str(bc.CASES[name].get("knobs")):
        assert run["plan"]["retained_points"] == 3                    # (a pseudo-camera holds three points)
        prob = bc.problem(name)
        assert all(np.isfinite(bc.box(name)[0][9 * prob.num_cameras + 3 * q]) for q in bc.widest_tracks(prob, 3))
    if bc.CASES[name].get("tape"):
        assert run["plan"]["tape_blocks"] == bc.problem(name).num_observations
    free = bc.model(name).free
    for x in run["xs"][1:]:                                           # a held coordinate does not move
        assert np.array_equal(x[~free], run["xs"][0][~free])


def test_projected_start_is_written_back_without_a_step(runs):
    name = "small-infeasible-start"
    prob, (lo, hi) = bc.problem(name), bc.box(name)
    run = runs(name, kmax=0)
    assert len(run["log"]) == 1 and len(run["xs"]) == 1
    want = br.project(prob.parameters, lo, hi)
    assert not np.array_equal(want, prob.parameters)
    assert np.array_equal(run["xs"][0], want)                          # min(max(x, lo), hi): exact
    ref = bc.reference(name, kmax=0)[1][0]
    assert bc.dc.close(run["summary"].initialCost(), ref["cost"], bc.TOL["cost"])
    assert run["summary"].initialCost() == run["summary"].finalCost() == run["log"][0]["cost"]
    assert run["log"][0]["step_size"] == 1.0 and run["log"][0]["line_search_evaluations"] == 1


def test_kkt_at_the_end_of_active_intrinsics(runs):
    """The projected-gradient max norm recomputed in long double from the oracle's Jacobians at the returned point."""
    name = "active-intrinsics"
    run = runs(name)
    assert run["log"][-1]["step_is_successful"]                        # (the logged norm is that of the returned point)
    want = br.projected_gradient_max_norm(bc.model(name), run["xs"][0], run["xs"][-1], *bc.box(name))
    got = run["log"][-1]["gradient_max_norm"]
    print("kkt", got, want, flush=True)
    assert abs(got - want) <= 1e-8 * want
    assert run["stats"][-1]["active_bounds"] > 0


def test_rerun_is_bitwise_equal(runs):
    a, b = runs("plans-retained"), runs("plans-retained", again=True)
    assert a is not b and len(a["log"]) == len(b["log"])
    for k in range(len(a["log"])):
        for f in list(bc.TOL) + ["cost_change", "step_size", "line_search_evaluations"]:
            assert a["log"][k][f] == b["log"][k][f], (k, f)
        assert np.array_equal(a["xs"][k], b["xs"][k])


def test_inactive_bounds_reduce_to_unbounded_levenberg_marquardt(runs):
    """Wide bounds against the same problem without any, both enqueued launch by launch (a replayed graph factors on one stream, by
    another plan): the same kernels on the same data, the cost of every iteration bit for bit."""
    a, b = runs("small-inactive"), runs("small-inactive", bounded=False, setGraphReplay=False)
    assert b["plan"]["graph_replay"] == 0 and a["plan"]["graph_replay"] == 0
    assert [e["cost"] for e in a["log"]] == [e["cost"] for e in b["log"]] and len(a["log"]) == bc.kmax_of("small-inactive") + 1
    assert all(e["step_size"] == 1.0 and e["line_search_evaluations"] == 1 for e in a["log"] + b["log"])
    assert b["stats"][-1]["bounded_coordinates"] == 0 and b["stats"][-1]["line_search_evaluations"] == 0
    for x, y in zip(a["xs"], b["xs"]):
        assert np.array_equal(x, y)


# ---- the dense Jacobian path -----------------------------------------------------------------------------------------------
def _dense_sk_problem(name):
    sizes, blocks, x0, lo, hi, pz = bc.dense_problem(name)
    keep = []
    if name == "dense-tangent":
        prob = bc.problem("small-infeasible-start")
        C, P = prob.num_cameras, prob.num_points
        x = sk.RichDoubleArray.fromArray(x0)
        problem = sk.Problem()
        loss = sk.PredefinedLossFunctions.trivialLoss()
        for o in range(prob.num_observations):
            cf = sk.SnavelyReprojectionError(*prob.observations[o]).toAutoDiffCostFunction()
            keep.append(cf)
            problem.addResidualBlock(cf, loss, x.slice(9 * int(prob.camera_index[o])), x.slice(9 * C + 3 * int(prob.point_index[o])))
        fixed = sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8])
        for i in range(C):
            if i in bc.CONST_CAMS:
                problem.setParameterBlockConstant(x.slice(9 * i))
            else:
                problem.setParameterization(x.slice(9 * i), fixed)
    else:
        x = sk.DoubleArray(len(x0))
        x.copyFrom(x0)
        problem = sk.Problem()
        if name == "powell":
            problem.addResidualBlock(sk.PowellF1().toAutoDiffCostFunction(), None, x, x.slice(1))
            problem.addResidualBlock(sk.PowellF2().toAutoDiffCostFunction(), None, x.slice(2), x.slice(3))
            problem.addResidualBlock(sk.PowellF3().toAutoDiffCostFunction(), None, x.slice(1), x.slice(2))
            problem.addResidualBlock(sk.PowellF4().toAutoDiffCostFunction(), None, x, x.slice(3))
        elif name == "hello-world":
            problem.addResidualBlock(sk.HelloCostFunctor().toAutoDiffCostFunction(), None, x)
        else:
            from helpers import curve_fitting_data
            for xv, yv in curve_fitting_data():
                problem.addResidualBlock(sk.ExponentialResidual(xv, yv).toAutoDiffCostFunction(), None, x, x.slice(1))
    offsets = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    _set_box(problem, x, [int(o) for o in offsets], sizes, lo, hi)
    return problem, x, len(x0), keep


@pytest.mark.parametrize("solver", ["DENSE_QR", "DENSE_NORMAL_CHOLESKY"])
@pytest.mark.parametrize("name", sorted(bc.DENSE_CASES))
def test_dense_jacobian_path(name, solver):
    sizes, blocks, x0, lo, hi, pz = bc.dense_problem(name)
    problem, x, n, keep = _dense_sk_problem(name)
    run = _solve(problem, x, n, _options(bc.kmax_of(name), solver=solver), plan_names=())
    assert run["summary"].linearSolverTypeUsed() == getattr(sk.LinearSolverType, solver)
    _check_run(name, run, bc.dense_reference(name)[1], lo, hi)
    free = bc.dense_model(name).free
    for xk in run["xs"][1:]:
        assert np.array_equal(xk[~free], run["xs"][0][~free])
    if name == "hello-world":
        assert run["xs"][-1][0] == 7.0 and run["summary"].finalCost() == 4.5            # exactly
        assert run["log"][-1]["gradient_max_norm"] == 0.0
        problem, x, n, keep = _dense_sk_problem(name)                                   # with iterations to spare: converged, on the bound
        summary = sk.Solver.Summary()
        sk.ceres.solve(_options(10, solver=solver), problem, summary)
        assert summary.terminationType() == sk.TerminationType.CONVERGENCE and "Gradient tolerance" in summary.message()
        assert x.get(0) == 7.0 and summary.finalCost() == 4.5 and len(summary.iterations()) == 2


# ---- what is refused ---------------------------------------------------------------------------------------------------------
def _refused(options, problem, what):
    with pytest.raises(sk.SkeresError, match="status 4") as e:   # SK_ERR_UNSUPPORTED
        sk.StepSolver(options, problem)
    assert "not supported" in str(e.value) and what in str(e.value)
    summary = sk.Solver.Summary()
    with pytest.raises(sk.SkeresError, match="not supported"):
        sk.ceres.solve(options, problem, summary)


def test_refusals():
    name = "small-infeasible-start"
    prob, box = bc.problem(name), bc.box(name)
    problem, params = _build(prob, box=box)
    # DOGLEG
    o = _options(3)
    o.setTrustRegionStrategyType(sk.TrustRegionStrategyType.DOGLEG)
    _refused(o, problem, "DOGLEG")
    # a world of two ranks
    o = _options(3)
    o.setDistributed(0, 2, lambda ptr, count, stream: None)
    _refused(o, problem, "ranks")
    # dense rows
    consts, _ = dense_synth.generate(100, 30, seed=3)
    x = sk.DoubleArray(30)
    x.copyFrom(np.zeros(30))
    rows = sk.Problem()
    rows.addDenseRows(oracle.SYNTH_TANH_ROW, consts, None, x, 30)
    rows.setParameterLowerBound(x, 3, -0.5)
    _refused(_options(3, solver="DENSE_NORMAL_CHOLESKY"), rows, "dense-row")
    # host-evaluated residual blocks under DENSE_SCHUR
    from test_gpu_dogleg import _host_snavely_functor
    HostSnavely = _host_snavely_functor()
    hparams = sk.RichDoubleArray.fromArray(prob.parameters)
    host = sk.Problem()
    keep = []
    loss = sk.PredefinedLossFunctions.trivialLoss()
    for i in range(prob.num_observations):
        ox, oy = prob.observations[i]
        cf = HostSnavely(ox, oy).toAutoDiffCostFunction() if i % 4 == 0 else sk.SnavelyReprojectionError(ox, oy).toAutoDiffCostFunction()
        keep.append(cf)
        host.addResidualBlock(cf, loss, hparams.slice(9 * int(prob.camera_index[i])), hparams.slice(9 * prob.num_cameras + 3 * int(prob.point_index[i])))
    host.setParameterUpperBound(hparams.slice(9 * 2), 6, 2000.0)
    _refused(_options(3), host, "director")
    # a bounded block with a quaternion / a homogeneous-vector parameterization
    for pz in (sk.PredefinedLocalParameterizations.quaternion(), sk.PredefinedLocalParameterizations.homogeneousVector(4)):
        q = sk.DoubleArray(4)
        q.copyFrom(np.array([1.0, 0.0, 0.0, 0.0]))
        quat = sk.Problem()
        cfs = [sk.QuaternionRotationError(p, t).toAutoDiffCostFunction() for p, t in (([1.0, 0.0, 0.0], [0.0, 1.0, 0.0]), ([0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]))]
        for cf in cfs:
            quat.addResidualBlock(cf, None, q)
        quat.setParameterization(q, pz)
        quat.setParameterLowerBound(q, 0, 0.0)
        _refused(_options(3, solver="DENSE_QR"), quat, "quaternion or homogeneous-vector")
        # ... and without the bound it solves
        quat.setParameterLowerBound(q, 0, -np.inf)
        sk.ceres.solve(_options(3, solver="DENSE_QR"), quat, sk.Solver.Summary())
