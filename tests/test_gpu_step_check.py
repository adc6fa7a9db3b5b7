"""The device's accepted LM steps against the damped normal equations they solve (tests/step_check.py): for k = 1..3, x_k from a
solve with max_num_iterations = k, x_{k-1} from the solve one iteration shorter (its logged costs a bitwise prefix of run k's),
and eta <= max(TAU, 4 floor), the model cost change of the log to 1e-10, gradient_max_norm to 1e-11.  Every case asserts
through stat() that it ran the plan it names.  Backward errors are comparable across plans, elimination orders, retained-point
sets and slab counts, where the step vectors themselves are not (the reduced system's gauge directions are damped only by D^2).

With STEP_CHECK_LOG set, every checked step appends one JSON line (case, k, eta, floor, the oracle's eta where it runs) there."""
import json
import os

import numpy as np
import pytest

import oracle
import skeres_amd as sk
from skeres_amd import bal, dense_synth
from helpers import bal_problem_to_sk, bal_from_tracks, structural_edges_tracks, curve_fitting_data, sk_loss
import step_check as sc

pytestmark = pytest.mark.gpu

BAL_STATS = ("retained_points", "dissected", "border_cameras", "cholesky_columns_resident", "segments", "envelope_fill", "graph_replay",
             "pair_segments_short", "pair_segments_long", "host_callback_blocks", "tape_blocks")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _record(case, k, e, oracle_eta=None):
    path = os.environ.get("STEP_CHECK_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "k": k, "eta": e["eta"], "floor": e["floor"], "eta_cameras": e["eta_cameras"],
                                "eta_points": e["eta_points"], "eta_retained": e["eta_retained"], "oracle_eta": oracle_eta}) + "\n")


def _stats(solver, names):
    out = {}
    for nm in names:
        try:
            out[nm] = solver.stat(nm)
        except sk.SkeresError:
            pass
    return out


def _device_steps(build, kmax, configure, names=BAL_STATS):
    """build() -> (problem, params, n); configure(options).  Returns x_0..x_kmax, the logs of the runs, the plan's stats and the
    summaries; the logged costs of run k - 1 are asserted to be a bitwise prefix of run k's."""
    xs, logs, stats, sums = [], [None], None, [None]
    for k in range(1, kmax + 1):
        problem, params, n = build()
        if k == 1:
            xs.append(params.toArray(n))
        options = sk.Solver.Options()
        configure(options)
        options.setMaxNumIterations(k)
        solver = sk.StepSolver(options, problem)
        st = _stats(solver, names)
        assert stats is None or st == stats
        stats = st
        while not solver.step():
            pass
        summary = sk.Solver.Summary()
        solver.finish(summary)
        xs.append(params.toArray(n))
        logs.append(summary.iterations())
        sums.append(summary)
        if k > 1:
            assert [it["cost"] for it in logs[k][:k]] == [it["cost"] for it in logs[k - 1][:k]], k
    return xs, logs, stats, sums


def _check_steps(case, model, xs, logs, kmax, jacobi_scaling=True, oracle_xs=None, oracle_logs=None, min_lm_diagonal=1e-6):
    """Checks every accepted step of the runs; returns the number checked and the most columns the LM diagonal clamped."""
    s = sc.jacobi_scale(model, xs[0], jacobi_scaling)
    checked = clamped = 0
    for k in range(1, kmax + 1):
        log = logs[k]
        if len(log) <= k:
            break
        if not log[k]["step_is_successful"]:
            assert np.array_equal(xs[k], xs[k - 1])
            continue
        e = sc.check(model, xs[0], xs[k - 1], xs[k], log, k, jacobi_scaling=jacobi_scaling, scale=s, min_lm_diagonal=min_lm_diagonal)
        oe = None
        if oracle_xs is not None and len(oracle_logs[k]) > k and oracle_logs[k][k]["step_is_successful"]:
            oe = sc.backward_error(model, xs[0], oracle_xs[k - 1], oracle_xs[k], oracle_logs[k], k, jacobi_scaling=jacobi_scaling, scale=s,
                                   min_lm_diagonal=min_lm_diagonal)["eta"]
        _record(case, k, e, oe)
        checked += 1
        clamped = max(clamped, e["clamped"])
    assert checked >= 1
    return checked, clamped


def _bal_builder(prob, loss=None, losses=None, const_cams=(), const_pts=(), subset_intrinsics=False):
    """A builder of the sk problem of `prob`: one loss, or a loss spec per observation (losses; blocks added in one bulk call per
    spec), constant cameras / points, intrinsics held by a subset parameterization."""
    C = prob.num_cameras

    def build():
        if losses is None:
            problem, params, _ = bal_problem_to_sk(prob, loss=sk_loss(loss) if loss else None)
        else:
            params = sk.RichDoubleArray.fromArray(prob.parameters)
            problem = sk.Problem()
            offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
            keys = [repr(l) for l in losses]
            for key in sorted(set(keys)):
                sel = np.array([kk == key for kk in keys])
                spec = losses[int(np.flatnonzero(sel)[0])]
                problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations[sel],
                                          sk_loss(spec) if spec else sk.PredefinedLossFunctions.trivialLoss(), params, offs[sel])
        if subset_intrinsics:
            fixed = sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8])
            for i in range(C):
                if i not in const_cams:
                    problem.setParameterization(params.slice(9 * i), fixed)
        for i in const_cams:
            problem.setParameterBlockConstant(params.slice(9 * i))
        for q in const_pts:
            problem.setParameterBlockConstant(params.slice(9 * C + 3 * q))
        return problem, params, prob.num_parameters
    cam_mask = pt_mask = None
    if const_cams or const_pts or subset_intrinsics:
        cam_mask = np.full(C, 0b111000000 if subset_intrinsics else 0, dtype=np.int32)
        cam_mask[list(const_cams)] = 0x1ff
        pt_mask = np.zeros(prob.num_points, dtype=np.int32)
        pt_mask[list(const_pts)] = 7
    return build, cam_mask, pt_mask


def _dense_schur(**knobs):
    def configure(o):
        o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
        for k, v in knobs.items():
            getattr(o, k)(*v) if isinstance(v, tuple) else getattr(o, k)(v)
    return configure


def _bal_case(case, prob, kmax=3, knobs=None, loss=None, losses=None, const_cams=(), const_pts=(), with_oracle=False,
              jacobi_scaling=True, min_relative_decrease=None, min_lm_diagonal=None):
    knobs = dict(knobs or {})
    if min_lm_diagonal:
        knobs["setMinLmDiagonal"] = min_lm_diagonal
    if not jacobi_scaling:
        knobs["setJacobiScaling"] = False
    if min_relative_decrease:
        knobs["setMinRelativeDecrease"] = min_relative_decrease
    build, cam_mask, pt_mask = _bal_builder(prob, loss=loss, losses=losses, const_cams=const_cams, const_pts=const_pts)
    xs, logs, stats, sums = _device_steps(build, kmax, _dense_schur(**knobs))
    assert sums[1].linearSolverTypeUsed() == sk.LinearSolverType.DENSE_SCHUR
    retained = None
    if stats.get("retained_points", 0) > 0:
        problem, _, _ = build()
        rp = problem.retainedPlan("on" if "setRetainedPoints" in knobs else "auto",
                                  knobs["setRetainedPoints"][1] if isinstance(knobs.get("setRetainedPoints"), tuple) else 0)
        if rp["retained_points"] == stats["retained_points"]:
            retained = np.unique(prob.point_index[rp["retained_of_block"] == 1])
    model = sc.BalModel(prob, loss=losses if losses is not None else loss, cam_mask=cam_mask, pt_mask=pt_mask, retained=retained)
    oxs = ologs = None
    if with_oracle:
        oxs, ologs = [prob.parameters.copy()], [None]
        extra = {"min_relative_decrease": min_relative_decrease} if min_relative_decrease else {}
        if min_lm_diagonal:
            extra["min_lm_diagonal"] = min_lm_diagonal
        for k in range(1, kmax + 1):
            x, so = oracle.solve_bal(prob.num_cameras, prob.num_points, prob.camera_index, prob.point_index, prob.observations, prob.parameters,
                                     oracle.default_options(linear_solver_type=oracle.DENSE_SCHUR, max_num_iterations=k, num_threads=4,
                                                            jacobi_scaling=int(jacobi_scaling), **extra),
                                     loss=loss, cam_mask=cam_mask, pt_mask=pt_mask)
            oxs.append(x)
            ologs.append(sc.log_of(so))
    _, clamped = _check_steps(case, model, xs, logs, kmax, jacobi_scaling=jacobi_scaling, oracle_xs=oxs, oracle_logs=ologs,
                              min_lm_diagonal=min_lm_diagonal or 1e-6)
    return stats, logs, clamped


def _plan(prob, **knobs):
    """The plan's stats of a solver of `prob` under DENSE_SCHUR and `knobs`, created and not stepped."""
    problem, _, _ = bal_problem_to_sk(prob)
    options = sk.Solver.Options()
    _dense_schur(**knobs)(options)
    return _stats(sk.StepSolver(options, problem), BAL_STATS)


# ---------------------------------------------------------------------------
# plans on generated problems
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,P,N,seed", [(6, 40, 200, 1), (16, 600, 2600, 11), (150, 3000, 14000, 5), (400, 30000, 140000, 77)])
def test_auto_plan_steps(C, P, N, seed):
    prob = bal.generate(C, P, N, seed=seed)
    stats, _, _ = _bal_case("auto-%d" % C, prob, kmax=3 if C <= 150 else 2, with_oracle=C <= 150)
    assert stats["segments"] >= 1


def test_bal49_with_graph_replay_steps():
    prob = bal.generate(49, 7776, 31843, seed=49)
    stats, _, _ = _bal_case("bal49-graph-replay", prob, knobs={"setGraphReplay": True}, kmax=2, with_oracle=True)
    assert stats["graph_replay"] == 1
    assert stats["retained_points"] == 0 and stats["dissected"] == 0   # (a launch-bound problem under replay retains nothing)


@pytest.mark.parametrize("npts", [4, 7])
def test_retained_points_forced_steps(npts):
    """Asked for 4 and 7 points the plan retains 3 and 6: a pseudo-camera holds three points, and the plan fills every one."""
    prob = bal.generate(150, 3000, 14000, seed=5)
    stats, _, _ = _bal_case("retained-%d" % npts, prob, knobs={"setRetainedPoints": ("on", npts), "setGraphReplay": False}, kmax=2)
    assert stats["retained_points"] == npts - npts % 3


@pytest.mark.parametrize("resident", [True, False])
def test_dissection_forced_steps(resident):
    """Two-way dissection; without resident kernels the only path that launches border_add2_kernel."""
    prob = bal.generate(400, 30000, 140000, seed=77) if not resident else bal.generate(150, 3000, 14000, seed=5)
    knobs = {"setCholeskyDissection": "on"}
    if not resident:
        knobs["setResidentKernels"] = False
    stats, _, _ = _bal_case("dissection-resident-%s" % ("on" if resident else "off"), prob, knobs=knobs, kmax=2)
    assert stats["dissected"] == 1
    if not resident:
        assert stats.get("cholesky_columns_resident", 0) == 0


def test_envelope_off_steps():
    prob = bal.generate(150, 3000, 14000, seed=5)
    stats, _, _ = _bal_case("envelope-off", prob, knobs={"setCholeskyEnvelope": False}, kmax=2)
    assert stats["envelope_fill"] >= 0.99


def test_jacobi_scaling_off_steps():
    prob = bal.generate(150, 3000, 14000, seed=5)
    stats, _, _ = _bal_case("jacobi-off", prob, kmax=2, jacobi_scaling=False, with_oracle=True)
    assert stats == _plan(prob)   # (the plan AUTO makes with Jacobi scaling on)


def test_border_of_loop_closure_cameras_steps():
    prob = bal.generate(600, 6000, 26000, seed=9, revisits=[(60, 350, 12, 40), (200, 520, 12, 40)])
    stats, _, _ = _bal_case("border-revisits", prob, knobs={"setCholeskyBorder": "on", "setRetainedPoints": "off"}, kmax=2)
    assert stats["border_cameras"] >= 1 and stats["retained_points"] == 0


def test_rejected_step_then_accepted_steps():
    """Step 3 is rejected (relative decrease 0.61 under min_relative_decrease 0.65; chosen with the oracle), step 4 solves the same J
    with a new D (0.66).  (A near-undamped first step, radius 1e14, is no such case: its gauge directions are rounding noise
    amplified 1e14-fold, and whether it decreases the cost differs between two correct solves.)"""
    prob = bal.generate(16, 600, 2600, seed=4, perturb=(0.1, 1.0, 2.0))
    stats, logs, _ = _bal_case("rejected-step", prob, kmax=4, min_relative_decrease=0.65, with_oracle=True)
    assert stats["graph_replay"] == 1 and stats["retained_points"] == 0 and stats["dissected"] == 0
    assert [bool(logs[k][k]["step_is_successful"]) for k in range(1, 5)] == [True, True, False, True]


def test_tolerant_loss_and_constant_blocks_steps():
    prob = bal.generate(150, 3000, 14000, seed=6)
    stats, _, _ = _bal_case("tolerant+constant", prob, kmax=2, loss=("tolerant", 4.0, 1.0), const_cams=(0, 75), const_pts=(5, 6), with_oracle=True)
    assert stats["graph_replay"] == 0 and stats["segments"] >= 1


@pytest.mark.parametrize("variant", ["auto", "retained", "dense"])
def test_clamped_lm_diagonal_steps(variant):
    """With the default min_lm_diagonal (1e-6) no column is clamped on these problems (||J_s,j||^2 >= 0.24: the Jacobi-scaled norm
    ||J_j|| / (1 + ||J_j||) is far from 0), so min_lm_diagonal = 0.5 here: D^2 = clamp(||J_s,j||^2, 0.5, max) / radius clamps some
    columns and not others, and a clamp of the unscaled norm, or of the wrong side, would show."""
    if variant == "dense":
        prob = bal.generate(2, 37, 74, seed=237)
        build, cam_mask, pt_mask = _bal_builder(prob)

        def configure(o):
            o.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
            o.setMinLmDiagonal(0.5)
        xs, logs, _, sums = _device_steps(build, 3, configure, names=())
        assert sums[1].linearSolverTypeUsed() == sk.LinearSolverType.DENSE_QR
        _, clamped = _check_steps("clamped-DENSE_QR-n129", sc.BalModel(prob), xs, logs, 3, min_lm_diagonal=0.5)
        free = prob.num_parameters
    else:
        prob = bal.generate(150, 3000, 14000, seed=5)
        knobs = {"setRetainedPoints": ("on", 6), "setGraphReplay": False} if variant == "retained" else {}
        stats, _, clamped = _bal_case("clamped-" + variant, prob, kmax=2, knobs=knobs, min_lm_diagonal=0.5, with_oracle=variant == "auto")
        assert stats["retained_points"] == (6 if variant == "retained" else stats["retained_points"])
        free = prob.num_parameters
    assert 0 < clamped < free


# ---------------------------------------------------------------------------
# structural edges of the Schur assembly
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges_problem():
    C, tracks = structural_edges_tracks()
    prob = bal_from_tracks(C, tracks)
    assert prob.num_points % 64 and prob.num_observations % 64
    return prob


@pytest.mark.parametrize("variant", ["auto", "retained", "mixed-loss", "constant"])
def test_structural_edges_steps(edges_problem, variant):
    """The pair segments: 7 long ones (32 .. 38 shared points) and a number of short ones that is not a multiple of the seven lane
    groups of a wave (535 without the 260-camera track, 33713 with it; tests/helpers.py structural_edges_tracks)."""
    prob = edges_problem
    kw = {}
    if variant == "retained":
        kw["knobs"] = {"setRetainedPoints": ("on", 3), "setGraphReplay": False}
    elif variant == "mixed-loss":
        specs = [("tolerant", 4.0, 1.0), ("cauchy", 2.0), None]
        kw["losses"] = [specs[o % 3] for o in range(prob.num_observations)]
    elif variant == "constant":
        kw["const_cams"] = (21,)
        kw["const_pts"] = (int(prob.point_index[0]),)
    stats, _, _ = _bal_case("edges-" + variant, prob, kmax=2, **kw)
    if variant == "retained":
        assert stats["retained_points"] == 3
    else:
        assert stats["pair_segments_long"] == 7, stats
        assert stats["pair_segments_short"] in (535, 33713), stats
        assert stats["host_callback_blocks"] == 0 and stats["tape_blocks"] == 0


def _host_snavely():
    from test_gpu_parity import _host_snavely_functor
    return _host_snavely_functor()


@pytest.mark.parametrize("path", ["director", "tape"])
def test_structural_edges_through_the_host_director_and_the_tape(edges_problem, path):
    """The same problem with a quarter of its blocks evaluated by host code (the director path: rows uploaded into the Schur
    assembly), and all of them through a recorded functor (the tape)."""
    prob = edges_problem
    C = prob.num_cameras
    HostSnavely = _host_snavely() if path == "director" else None
    keep = []

    def build():
        params = sk.RichDoubleArray.fromArray(prob.parameters)
        problem = sk.Problem()
        if path == "tape":
            from skeres_amd.examples.traced_functors import TracedSnavelyReprojectionError
            offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
            f = TracedSnavelyReprojectionError(0.0, 0.0)
            keep.append(f)
            problem.addResidualBlocksTraced(f, prob.observations, None, params, offs)
        else:
            loss = sk.PredefinedLossFunctions.trivialLoss()
            for i in range(prob.num_observations):
                ox, oy = prob.observations[i]
                cf = HostSnavely(ox, oy).toAutoDiffCostFunction() if i % 4 == 0 else sk.SnavelyReprojectionError(ox, oy).toAutoDiffCostFunction()
                keep.append(cf)
                problem.addResidualBlock(cf, loss, params.slice(9 * int(prob.camera_index[i])), params.slice(9 * C + 3 * int(prob.point_index[i])))
        return problem, params, prob.num_parameters
    xs, logs, stats, sums = _device_steps(build, 2, _dense_schur())
    assert sums[1].linearSolverTypeUsed() == sk.LinearSolverType.DENSE_SCHUR
    if path == "director":
        assert stats["host_callback_blocks"] == (prob.num_observations + 3) // 4 and stats["tape_blocks"] == 0
    else:
        assert stats["tape_blocks"] == prob.num_observations and stats["host_callback_blocks"] == 0
    assert stats["graph_replay"] == 0
    _check_steps("edges-" + path, sc.BalModel(prob), xs, logs, 2)


# ---------------------------------------------------------------------------
# ranks: a world of two over gloo sharing one GPU (tests/dist_gpu_worker2.py saves rank 0's x after k iterations)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape,segments", [("sharded", "600,6000,26000,9,kept", None), ("segmented", "600,6000,26000,9,kept2", 2)])
def test_world_of_two_ranks_steps(tmp_path, mode, shape, segments):
    """One run sharded (twelve retained points, whichever rank owns one writes its rows), one segmented in two with the retained
    points' pseudo-cameras in the separator."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    save = str(tmp_path / "steps.json")
    port = 29700 + (os.getpid() % 97)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "dist_gpu_worker2.py"), mode, shape] + ([str(segments)] if segments else [])
    out = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="1", STEP_CHECK_SAVE=save, STEP_CHECK_K="2"), cwd=root,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_GPU2_OK world=2" in out.stdout
    saved = json.load(open(save))
    fields = shape.split(",")
    prob = bal.generate(int(fields[0]), int(fields[1]), int(fields[2]), seed=int(fields[3]))
    for run in saved["runs"]:
        plan = run["plan"]
        assert plan["distribution"] == mode and plan["retained_points"] == 12
        if mode == "segmented":
            assert plan["dissected"] == 1 and plan["segments"] == 2
    xs = [prob.parameters.copy()] + [np.array(r["x"]) for r in saved["runs"]]
    logs = [None] + [r["log"] for r in saved["runs"]]
    assert [it["cost"] for it in logs[2][:2]] == [it["cost"] for it in logs[1][:2]]
    _check_steps("world2-" + mode, sc.BalModel(prob), xs, logs, 2)


# ---------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------
def test_ladybug_1723_steps_at_full_size():
    """The default plan: retained points, lock-step dissection, resident chain; step 2 is the first to factor an S that the
    janitor workgroups cleaned."""
    prob = bal.generate_named("ladybug-1723-156502", seed=1723, perturb=(1e-2, 1e-1, 1e-1))
    stats, _, _ = _bal_case("ladybug-1723", prob, kmax=3)
    assert stats["retained_points"] >= 3 and stats["dissected"] >= 1 and stats["cholesky_columns_resident"] > 0


# ---------------------------------------------------------------------------
# dense paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["DENSE_QR", "DENSE_NORMAL_CHOLESKY"])
@pytest.mark.parametrize("C,P,subset", [(2, 36, False), (2, 37, False), (5, 70, False), (5, 71, False), (5, 71, True)])
def test_dense_solvers_on_bal_steps(solver, C, P, subset):
    """n = 9C + 3P = 126, 129, 255, 258 on both sides of 128 and 256; once with the intrinsics held by a subset parameterization."""
    N = 2 * P if C == 2 else 3 * P
    prob = bal.generate(C, P, N, seed=C * 100 + P)
    build, cam_mask, pt_mask = _bal_builder(prob, subset_intrinsics=subset)
    lst = getattr(sk.LinearSolverType, solver)
    xs, logs, _, sums = _device_steps(build, 3, lambda o: o.setLinearSolverType(lst), names=())
    assert sums[1].linearSolverTypeUsed() == lst
    _check_steps("%s-n%d%s" % (solver, 9 * C + 3 * P, "-subset" if subset else ""), sc.BalModel(prob, cam_mask=cam_mask, pt_mask=pt_mask), xs, logs, 3)


@pytest.mark.parametrize("solver", ["DENSE_QR", "DENSE_NORMAL_CHOLESKY"])
def test_curve_fitting_steps(solver):
    data = curve_fitting_data()
    lst = getattr(sk.LinearSolverType, solver)

    def build():
        x = sk.DoubleArray(2)
        x.copyFrom(np.zeros(2))
        problem = sk.Problem()
        for xv, yv in data:
            problem.addResidualBlock(sk.ExponentialResidual(xv, yv).toAutoDiffCostFunction(), None, x, x.slice(1))
        return problem, x, 2
    # (from m = c = 0 the first steps of EX/CurveFitting.scala are rejected: eight iterations hold accepted ones)
    xs, logs, _, sums = _device_steps(build, 8, lambda o: o.setLinearSolverType(lst), names=())
    assert sums[1].linearSolverTypeUsed() == lst
    blocks = [(oracle.EXPONENTIAL, [xv, yv], [0, 1], None) for xv, yv in data]
    assert _check_steps("curve-fitting-" + solver, sc.BlocksModel([1, 1], blocks), xs, logs, 8)[0] >= 2


# ---------------------------------------------------------------------------
# dense rows (config 5): the slab count of the Gram kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,slabs,loss", [(10000, 1, 2, None), (10000, 127, 2, None), (10000, 1025, 2, None), (40000, 129, 8, None),
                                            (70000, 128, 16, None), (9000, 1024, 2, None), (100, 300, 1, None), (10000, 129, 2, ("cauchy", 0.1))])
def test_dense_rows_steps(m, n, slabs, loss):
    consts, _ = dense_synth.generate(m, n, seed=m + n)

    def build():
        x = sk.DoubleArray(n)
        x.copyFrom(np.zeros(n))
        problem = sk.Problem()
        problem.addDenseRows(oracle.SYNTH_TANH_ROW, consts, sk_loss(loss), x, n)
        return problem, x, n

    def configure(o):
        o.setLinearSolverType(sk.LinearSolverType.DENSE_NORMAL_CHOLESKY)
    kmax = 2
    xs, logs, stats, sums = _device_steps(build, kmax, configure, names=("gram_slabs",))
    assert stats["gram_slabs"] == slabs
    _check_steps("dense-rows-%dx%d%s" % (m, n, "-cauchy" if loss else ""), sc.DenseRowsModel(consts, n, loss=loss), xs, logs, kmax)


def test_dense_rows_with_every_column_clamped_steps():
    """min_lm_diagonal = 2 above every ||J_s,j||^2 (< 1 with Jacobi scaling): D^2 = 2 / radius on every column (launch_lm_diagonal of
    the dense-rows solver)."""
    m, n = 10000, 129
    consts, _ = dense_synth.generate(m, n, seed=m + n)

    def build():
        x = sk.DoubleArray(n)
        x.copyFrom(np.zeros(n))
        problem = sk.Problem()
        problem.addDenseRows(oracle.SYNTH_TANH_ROW, consts, None, x, n)
        return problem, x, n

    def configure(o):
        o.setLinearSolverType(sk.LinearSolverType.DENSE_NORMAL_CHOLESKY)
        o.setMinLmDiagonal(2.0)
    xs, logs, stats, sums = _device_steps(build, 2, configure, names=("gram_slabs",))
    assert stats["gram_slabs"] == 2
    _, clamped = _check_steps("dense-rows-clamped-%dx%d" % (m, n), sc.DenseRowsModel(consts, n), xs, logs, 2, min_lm_diagonal=2.0)
    assert clamped == n
