"""The cases of the termination brackets (tests/termination_check.py): per case a device runner (tests/test_gpu_termination.py) and,
where a reference model exists, runners of tests/failure_reference.py in double and long double and of the compiled oracle
(tests/test_termination_cpu.py).  The problems and device builders are those of the other suites; no generator is new here.

A case: n (the ambient parameter count: delta of the parameter bracket), K (the baseline's iterations), device (-> a runner over
the device), plan (stats a DENSE_SCHUR case must show: name -> (relation, value)), exits (the brackets the case is there for: all of
them unless its trajectory rules one out, which the case then says), reference / oracle (-> runners, or absent)."""
import functools

import numpy as np

import failure_reference as fr
import step_check as sc

LD = np.longdouble
SETTERS = dict(max_num_iterations="setMaxNumIterations", gradient_tolerance="setGradientTolerance", parameter_tolerance="setParameterTolerance",
               function_tolerance="setFunctionTolerance", min_trust_region_radius="setMinTrustRegionRadius")
ALL_EXITS = ("gradient", "radius", "function", "parameter", "order")
PLAN_STATS = ("retained_points", "dissected", "graph_replay", "cholesky_columns_resident", "segments", "tape_blocks")
CASES = {}


def _case(name, **kw):
    kw.setdefault("exits", ALL_EXITS)
    CASES[name] = dict(kw, name=name)


def names(exit=None):
    return [n for n, c in CASES.items() if exit is None or exit in c["exits"]]


# ---------------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------------
def device_runner(build, configure, stats=(), distribution=False, track_xs=True):
    """run(options) over a fresh problem and a fresh StepSolver: build() -> (problem, params, n, ...), configure() -> the case's
    sk.Solver.Options.  The run carries xs (x after create and after every logged iteration), stats (read after create) and
    idempotent: a further step() after the exit reported done and changed neither the summary nor x.  track_xs = False: finish() is
    called at the end only (a world of ranks, where it gathers the points) and the run carries no xs."""
    import skeres_amd as sk
    from failure_cases import TERMINATION

    def fields(summary, x):
        return (summary.terminationType(), summary.message(), summary.numSuccessfulSteps(), summary.numUnsuccessfulSteps(), summary.finalCost(),
                [tuple(sorted((k, v) for k, v in e.items() if "time" not in k and "seconds" not in k)) for e in summary.iterations()], x.tobytes())

    def run(opts):
        built = build()
        problem, params, n = built[0], built[1], built[2]
        o = configure()
        for k, v in opts.items():
            getattr(o, SETTERS[k])(v)
        solver = sk.StepSolver(o, problem)
        st = {}
        for nm in stats:
            st[nm] = solver.stat(nm)
        if distribution:   # (a world of ranks: the distribution set-up chose)
            st["distribution"] = solver.distribution()[0]
        summary = sk.Solver.Summary()
        xs = []
        if track_xs:
            solver.finish(summary)
            xs.append(params.toArray(n))
        steps = 0
        while not solver.step():
            if track_xs:
                solver.finish(summary)
                xs.append(params.toArray(n))
            steps += 1
            assert steps <= 200, "the solve does not return"
        solver.finish(summary)
        x = params.toArray(n)
        if track_xs and len(summary.iterations()) > len(xs):   # (a tolerance exit logs its iteration and leaves x where it was)
            xs.append(x)
        before = fields(summary, x)
        again = solver.step()
        summary2 = sk.Solver.Summary()
        solver.finish(summary2)
        after = fields(summary2, params.toArray(n))
        out = dict(x=x, log=summary.iterations(), termination=TERMINATION[summary.terminationType()], message=summary.message(),
                   num_successful_steps=summary.numSuccessfulSteps(), num_unsuccessful_steps=summary.numUnsuccessfulSteps(),
                   final_cost=summary.finalCost(), stats=st, idempotent=bool(again) and before == after)
        if track_xs:
            out["xs"] = xs
        return out
    return run


def reference_runner(model, x0, base=None, long_double=False, schur=None, defect=None):
    """tests/failure_reference.py's loop as a runner."""
    def run(opts):
        r = fr.solve(model() if callable(model) else model, np.array(x0, dtype=np.float64), dict(base or {}, **opts), dtype=LD if long_double else np.float64,
                     schur=schur, defect=defect)
        xs = [np.array(x0, dtype=np.float64)]
        for e in r["log"][1:]:
            xs.append(np.array(e["candidate"]) if e["step_is_successful"] else xs[-1])
        return dict(r, xs=xs)
    return run


ORACLE_TERMINATION = {0: fr.CONVERGENCE, 1: fr.NO_CONVERGENCE, 2: fr.FAILURE}


def oracle_bal_runner(prob, base=None, cam_mask=None, pt_mask=None):
    """The compiled oracle's DENSE_SCHUR solve as a runner (no xs: the brackets fetch x_k by runs of k iterations)."""
    import oracle

    def run(opts):
        x, so = oracle.solve_bal(prob.num_cameras, prob.num_points, prob.camera_index, prob.point_index, prob.observations, prob.parameters.copy(),
                                 oracle.default_options(linear_solver_type=oracle.DENSE_SCHUR, num_threads=1, **dict(base or {}, **opts)),
                                 cam_mask=cam_mask, pt_mask=pt_mask)
        return dict(x=x, log=sc.log_of(so), termination=ORACLE_TERMINATION[so.termination_type], message=so.message.decode(),
                    num_successful_steps=so.num_successful_steps, num_unsuccessful_steps=so.num_unsuccessful_steps, final_cost=so.final_cost)
    return run


def oracle_blocks_runner(sizes, blocks, x0, solver="DENSE_QR"):
    import oracle

    def run(opts):
        x, so = oracle.solve(sizes, np.array(x0, dtype=np.float64), [b[:3] for b in blocks], oracle.default_options(linear_solver_type=getattr(oracle, solver), **opts))
        return dict(x=x, log=sc.log_of(so), termination=ORACLE_TERMINATION[so.termination_type], message=so.message.decode(),
                    num_successful_steps=so.num_successful_steps, num_unsuccessful_steps=so.num_unsuccessful_steps, final_cost=so.final_cost)
    return run


# ---------------------------------------------------------------------------------------------------------------------------
# DENSE_SCHUR on one process
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bal(shape, seed, perturb=None):
    from skeres_amd import bal
    return bal.generate(*shape, seed=seed, perturb=perturb) if perturb else bal.generate(*shape, seed=seed)


def _knobs(o, knobs):
    for k, v in knobs.items():
        getattr(o, k)(*v) if isinstance(v, tuple) else getattr(o, k)(v)
    return o


def _schur_options(knobs):
    def configure():
        import skeres_amd as sk
        o = sk.Solver.Options()
        o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
        return _knobs(o, knobs)
    return configure


def _schur_masks(prob, const_cams, const_pts, subset):
    if not (const_cams or const_pts or subset):
        return None, None
    cam_mask = np.full(prob.num_cameras, 0b111000000 if subset else 0, dtype=np.int32)
    cam_mask[list(const_cams)] = 0x1ff
    pt_mask = np.zeros(prob.num_points, dtype=np.int32)
    pt_mask[list(const_pts)] = 7
    return cam_mask, pt_mask


def _schur_case(name, shape, seed, perturb, K, knobs=None, plan=None, base=None, const_cams=(), const_pts=(), subset=False, reference=True, **kw):
    knobs = dict(knobs or {})

    def device():
        from test_gpu_step_check import _bal_builder
        build = _bal_builder(_bal(shape, seed, perturb), const_cams=const_cams, const_pts=const_pts, subset_intrinsics=subset)[0]
        return device_runner(build, _schur_options(knobs), stats=PLAN_STATS)
    more = {}
    if reference:
        def masks():
            return _schur_masks(_bal(shape, seed, perturb), const_cams, const_pts, subset)

        def ref(long_double=False, defect=None):
            prob = _bal(shape, seed, perturb)
            cam_mask, pt_mask = masks()
            return reference_runner(sc.BalModel(prob, cam_mask=cam_mask, pt_mask=pt_mask), prob.parameters, base, long_double,
                                    schur=(prob.num_cameras, prob.num_points), defect=defect)
        more = dict(reference=ref, oracle=lambda: oracle_bal_runner(_bal(shape, seed, perturb), base, *masks()))
    _case(name, n=9 * shape[0] + 3 * shape[1], K=K, device=device, plan=plan or {}, problem=lambda: _bal(shape, seed, perturb), **more, **kw)


SMALL = ((6, 40, 200), 1, (1e-2, 1e-1, 1e-1))
REJECTING_BASE = dict(min_relative_decrease=0.65, max_trust_region_radius=1e4)
REJECTING_KNOBS = {"setMinRelativeDecrease": 0.65, "setMaxTrustRegionRadius": 1e4}
PLANS = ((150, 3000, 14000), 5, None)
# 174 coordinates: less than one workgroup of the reduction over [cameras | points], its partial tail; as a replayed hipGraph and launch by launch
_schur_case("schur-small-replay", *SMALL, K=4, knobs={"setGraphReplay": True}, plan=dict(graph_replay=("eq", 1)))
_schur_case("schur-small-launches", *SMALL, K=4, knobs={"setGraphReplay": False}, plan=dict(graph_replay=("eq", 0)))
# the radius stays at its maximum, 1e4, until a rejected step halves it: the radius exit is bracketed behind a rejection
_schur_case("schur-rejecting", (16, 600, 2600), 4, (0.1, 1.0, 2.0), K=7, knobs=REJECTING_KNOBS, base=REJECTING_BASE, plan=dict(segments=("ge", 1)))
# held coordinates and pseudo-camera slots count as the ambient vector does: one constant camera, one constant point, subset intrinsics
_schur_case("schur-retained", *PLANS, K=4, knobs={"setRetainedPoints": ("on", 6)}, plan=dict(retained_points=("eq", 6)),
            const_cams=(7,), const_pts=(11,), subset=True, cpu="slow")
_schur_case("schur-dissected", *PLANS, K=4, knobs={"setCholeskyDissection": "on"}, plan=dict(dissected=("eq", 1)),
            const_cams=(7,), const_pts=(11,), subset=True, cpu="slow")


def _pinhole_device():
    """The (2; 6, 3) pinhole problem of tests/test_traced_functors.py: run padded to (2; 9, 3), three inert coordinates per camera."""
    from test_traced_functors import _pinhole_problem
    prob = _bal((16, 200, 900), 23)

    def build():
        problem, params, keep = _pinhole_problem(prob)
        return problem, params, 6 * prob.num_cameras + 3 * prob.num_points, keep
    return device_runner(build, _schur_options({}), stats=PLAN_STATS)


_case("schur-pinhole", n=6 * 16 + 3 * 200, K=4, device=_pinhole_device, plan=dict(tape_blocks=("eq", 900)))


# ---------------------------------------------------------------------------------------------------------------------------
# the dense Jacobian path, dense rows
# ---------------------------------------------------------------------------------------------------------------------------
def _dense_options(solver, knobs=None):
    def configure():
        import skeres_amd as sk
        o = sk.Solver.Options()
        o.setLinearSolverType(getattr(sk.LinearSolverType, solver))
        return _knobs(o, knobs or {})
    return configure


def _curve_device(solver):
    def device():
        import skeres_amd as sk
        from helpers import curve_fitting_data

        def build():
            x = sk.RichDoubleArray.fromArray(np.zeros(2))
            problem = sk.Problem()
            keep = []
            for xv, yv in curve_fitting_data():
                cf = sk.ExponentialResidual(xv, yv).toAutoDiffCostFunction()
                keep.append(cf)
                problem.addResidualBlock(cf, None, x, x.slice(1))
            return problem, x, 2, keep
        return device_runner(build, _dense_options(solver))
    return device


def _curve_reference(long_double=False, defect=None):
    import dogleg_cases as dc
    sizes, blocks, x0 = dc.dense_problem("curve-fitting")
    return reference_runner(sc.BlocksModel(sizes, blocks), x0, None, long_double, defect=defect)


def _curve_oracle(solver):
    def make():
        import dogleg_cases as dc
        sizes, blocks, x0 = dc.dense_problem("curve-fitting")
        return oracle_blocks_runner(sizes, blocks, x0, solver)
    return make


def _dense_bal_device(solver, subset):
    def device():
        from test_gpu_step_check import _bal_builder
        return device_runner(_bal_builder(_bal((2, 37, 74), 237), subset_intrinsics=subset)[0], _dense_options(solver))
    return device


def _dense_bal_reference(subset):
    def ref(long_double=False, defect=None):
        prob = _bal((2, 37, 74), 237)
        cam_mask, pt_mask = _schur_masks(prob, (), (), subset)
        return reference_runner(sc.BalModel(prob, cam_mask=cam_mask, pt_mask=pt_mask), prob.parameters, None, long_double, defect=defect)
    return ref


def _quaternion_fit():
    """The fit of tests/test_gpu_parity.py::test_quaternion_parameterization_solve_vs_oracle: ambient 4, tangent 3."""
    import oracle
    rng = np.random.default_rng(3)
    q_true = np.array([0.8, -0.3, 0.4, 0.33])
    q_true /= np.linalg.norm(q_true)
    pts = rng.normal(size=(3, 3))
    tgt = oracle.rotation_apply(9, np.concatenate([np.tile(q_true, (3, 1)), pts], axis=1)) + 0.01 * rng.normal(size=(3, 3))
    x0 = np.array([0.9, 0.1, -0.2, 0.3])
    return pts, tgt, x0 / np.linalg.norm(x0)


def _quaternion_device(solver):
    def device():
        import skeres_amd as sk
        pts, tgt, x0 = _quaternion_fit()

        def build():
            q = sk.RichDoubleArray.fromArray(x0)
            problem = sk.Problem()
            keep = [sk.QuaternionRotationError(p, t).toAutoDiffCostFunction() for p, t in zip(pts, tgt)]
            problem.addParameterBlock(q, 4, sk.PredefinedLocalParameterizations.quaternion())
            for cf in keep:
                problem.addResidualBlock(cf, None, q)
            return problem, q, 4, keep
        return device_runner(build, _dense_options(solver))
    return device


def _rows_device():
    import skeres_amd as sk
    from skeres_amd import dense_synth
    import oracle
    consts, _ = dense_synth.generate(10000, 129)

    def build():
        x = sk.RichDoubleArray.fromArray(np.zeros(129))
        problem = sk.Problem()
        problem.addDenseRows(oracle.SYNTH_TANH_ROW, consts, None, x, 129)
        return problem, x, 129, [consts]
    return device_runner(build, _dense_options("DENSE_NORMAL_CHOLESKY"))


for _solver in ("DENSE_QR", "DENSE_NORMAL_CHOLESKY"):
    # from (0, 0) the first steps are rejected: the radius exit behind rejections
    _case("curve-%s" % _solver, n=2, K=14, device=_curve_device(_solver), reference=_curve_reference, oracle=_curve_oracle(_solver))
    # n = 129 with the intrinsics held by a subset parameterization (the tangent-space form of the dense path) and without
    _case("dense-bal-%s" % _solver, n=129, K=4, device=_dense_bal_device(_solver, False), reference=_dense_bal_reference(False))
    _case("dense-bal-tangent-%s" % _solver, n=129, K=4, device=_dense_bal_device(_solver, True), reference=_dense_bal_reference(True))
    _case("quaternion-%s" % _solver, n=4, K=5, device=_quaternion_device(_solver))
_case("rows", n=129, K=5, device=_rows_device)


# ---------------------------------------------------------------------------------------------------------------------------
# CGNR, CGNR on the Schur complement, inner iterations
# ---------------------------------------------------------------------------------------------------------------------------
def _cgnr_device(name):
    def device():
        import cgnr_cases as cc
        return device_runner(lambda: cc.build_device(name), lambda: cc.device_options(name))
    return device


def _cgnr_schur_device():
    import cgnr_schur_cases as csc
    return device_runner(lambda: csc.build_device("bal-small"), lambda: csc.device_options("bal-small"))


def _inner_device():
    import inner_cases as ic
    return device_runner(lambda: ic.build_device("bal-small"), lambda: ic.device_options("bal-small"))


_case("cgnr-bal-small", n=174, K=5, device=_cgnr_device("bal-small"))
# n = 4200: the one-workgroup reduction loops 17 times.  Half of its steps are rejected, and the function quantity has its running minima
# (k = 2, 4, 6, 7, 12) where the step norm has none (k = 5, 8, 13): no k serves the run that holds the parameter test before the
# function test, which this case leaves to the others
_case("cgnr-chain", n=4200, K=12, device=_cgnr_device("chain"), parameter_before_function=False)
_case("cgnr-tape-quaternion", n=7, K=5, device=_cgnr_device("tape-quaternion"))     # the gradient's length 6 is not the ambient 7
_case("cgnr-schur-bal-small", n=174, K=5, device=_cgnr_schur_device)
_case("inner-bal-small", n=174, K=4, device=_inner_device)   # the step norm is the refined candidate's


# ---------------------------------------------------------------------------------------------------------------------------
# DOGLEG, bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _dogleg_schur_device():
    import dogleg_cases as dc
    from test_gpu_dogleg import _build, _options
    prob = dc.problem("small")

    def build():
        problem, params = _build(prob)
        return problem, params, prob.num_parameters
    return device_runner(build, lambda: _options(50))


def _dogleg_dense_device():
    from test_gpu_dogleg import _dense_sk_problem, _options
    import skeres_amd as sk

    def configure():
        o = _options(50)
        o.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
        return o
    return device_runner(lambda: _dense_sk_problem("curve-fitting"), configure)


def _bounds_device(name):
    def device():
        import bounds_cases as bc
        from test_gpu_bounds import _build, _options
        c, prob = bc.CASES[name], bc.problem(name)

        def build():
            problem, params = _build(prob, box=bc.box(name))
            return problem, params, prob.num_parameters
        return device_runner(build, lambda: _options(50, **c.get("options", {})), stats=("active_bounds", "bounded_coordinates"))
    return device


_case("dogleg-schur", n=174, K=5, device=_dogleg_schur_device)
_case("dogleg-dense", n=2, K=25, device=_dogleg_dense_device)
# Bounds: the gradient is the projected one and the step norm the line search's.  "active-intrinsics" keeps 15 to 17 bounds active and
# converges as projected steps do: its gradient max-norm falls by 7 % an iteration (535058, 326254, 301335, ... 175900 after ten, as
# the reference of tests/bounds_cases.py has it; "robust-subset", "contracting" and "plans-retained" likewise), so no k is a running
# minimum by a factor of two for the gradient exit, nor for the iteration-limit run that rides on it: it is there for the radius,
# function and parameter exits.  "small-infeasible-start" starts outside its box with seven bounds active after the projection and
# none from iteration 1 on: every exit.
_case("bounds-active", n=9 * 16 + 3 * 600, K=5, device=_bounds_device("active-intrinsics"), exits=("radius", "function", "parameter"))
_case("bounds-start", n=174, K=4, device=_bounds_device("small-infeasible-start"))


def check_plan(case, stats):
    for nm, (relation, value) in CASES[case].get("plan", {}).items():
        got = stats[nm]
        assert {"eq": got == value, "ge": got >= value, "gt": got > value}[relation], (case, nm, got, relation, value)
