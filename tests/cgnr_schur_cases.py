"""The cases of the tests of CGNR with the Schur elimination (tests/test_cgnr_schur_cpu.py, tests/test_gpu_cgnr_schur.py) and their
reference trajectories (tests/cgnr_schur_reference.py), computed once per process.  Each is the smallest shape that reaches a path:

    bal-small, bal-identity, bal-limit   cgnr_cases' (6, 40, 200): E the points, F four cameras; every list a single part
    bal-reset        eta = 1e-8: a solve of more than ten iterations (the residual reset) and of two batches
    bal-robust       (16, 600, 2600), Huber, subset intrinsics, a constant point: a camera's 160-odd pairs are three parts of the
                     kernel of S's block diagonal
    bal-duplicate    bal-small with one observation repeated: two residual blocks on one (g, e) pair
    landmark         covariance_schur_cases' bal-landmark: an e-block seen by 68 moving cameras, the long e-block path
    quaternion       cgnr_cases' recorded functor with 70 blocks: E is the parameterized block (tangent size 3, 70 slots: two parts)
    chain            cgnr_cases.chain_case(4400, 320): about half the blocks stay in F, so the reduced columns cross a 4096 dot chunk
                     and the F blocks the 256 of an update workgroup; the hub is an F block of many parts; every fifth pair reversed
    all-eliminated   three unrelated one-block residuals: F is empty

Seeds and the iterations compared (kmax) were chosen with the reference alone by cgnr_cases' rule: double and long double take the
same number of CG iterations in every solve, zeta stays ZETA_MARGIN away from eta at the stopping iteration and the one before,
and the two logs agree ten times inside the device tolerances.  tests/test_cgnr_schur_cpu.py asserts all three."""
import functools

import numpy as np

import oracle
from skeres_amd import bal
import step_check as sc
import dogleg_reference as dr
import dogleg_cases as dc
import cgnr_reference as cr
import cgnr_cases as cc
import cgnr_schur_reference as csr
import evaluate_cases as ec

LD = np.longdouble
TOL, ZETA_MARGIN = cc.TOL, cc.ZETA_MARGIN

_SMALL = dict(kind="bal", base="bal-small")
CASES = {
    "bal-small": dict(_SMALL, kmax=4),
    "bal-identity": dict(_SMALL, kmax=1, options=dict(preconditioner="identity")),
    "bal-limit": dict(_SMALL, kmax=4, options=dict(max_linear_solver_iterations=3)),
    "bal-reset": dict(_SMALL, kmax=3, options=dict(eta=1e-8)),
    "bal-robust": dict(kind="bal", base="bal-robust", kmax=4, loss=("huber", 1.0), subset=True, const_pts=(5,)),
    "bal-duplicate": dict(kind="bal", base="duplicate", kmax=4),
    "landmark": dict(kind="bal", base="landmark", kmax=3),
    "quaternion": dict(kind="quaternion", kmax=4),
    "chain": dict(kind="chain", kmax=3),
    "all-eliminated": dict(kind="separate", kmax=2),
}
CHAIN_BLOCKS, CHAIN_HUB_BLOCKS = 4400, 320


# ---- the problems ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bal_problem(name):
    base = CASES[name]["base"]
    if base == "duplicate":
        import covariance_cases as vc
        small = cc.bal_problem("bal-small")
        i, c, p = vc.duplicate_observation()
        obs = np.concatenate([small.observations, [small.observations[i] + np.array([0.25, -0.5])]])
        return bal.BalProblem(small.num_cameras, small.num_points, np.append(small.camera_index, c).astype(np.int32),
                              np.append(small.point_index, p).astype(np.int32), np.ascontiguousarray(obs), small.parameters.copy())
    if base == "landmark":      # covariance_schur_cases._bal_landmark's problem
        import covariance_schur_cases as scs
        C, P = scs.LANDMARK_CAMERAS, scs.LANDMARK_POINTS
        return scs._hand_bal(C, [[(37 * p + j) % C for j in range(4 + p % 3)] for p in range(P)] + [list(range(C))], seed=5)
    return cc.bal_problem(base)


def bal_masks(name):
    c, prob = CASES[name], bal_problem(name)
    cam_mask = np.full(prob.num_cameras, 0b111000000 if c.get("subset") else 0, dtype=np.int32)
    cam_mask[list(dc.CONST_CAMS)] = 0x1ff
    pt_mask = np.zeros(prob.num_points, dtype=np.int32)
    pt_mask[list(c.get("const_pts", ()))] = 7
    return cam_mask, pt_mask


@functools.lru_cache(maxsize=None)
def _chain():
    return cc.chain_case(num_blocks=CHAIN_BLOCKS, hub_blocks=CHAIN_HUB_BLOCKS)


@functools.lru_cache(maxsize=None)
def _separate():
    """r = 10 - x on each of three blocks of size 1."""
    return ec.Case("all-eliminated", [1.0, -2.0, 4.0], [1, 1, 1], [(oracle.HELLO_WORLD, [], [b], None, "dev") for b in range(3)])


def _blocks_case(name):
    return _chain() if CASES[name]["kind"] == "chain" else _separate()


def x0(name):
    kind = CASES[name]["kind"]
    if kind == "bal":
        return bal_problem(name).parameters
    if kind == "quaternion":
        return cc.quaternion_setup()[2]
    return np.asarray(_blocks_case(name).x, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def model(name):
    c = CASES[name]
    if c["kind"] == "bal":
        cam_mask, pt_mask = bal_masks(name)
        return sc.BalModel(bal_problem(name), loss=c.get("loss"), cam_mask=cam_mask, pt_mask=pt_mask)
    if c["kind"] == "quaternion":
        return cc.model("tape-quaternion")
    case = _blocks_case(name)
    return sc.BlocksModel(case.sizes, [blk[:4] for blk in case.blocks])


def cost(name):
    c = CASES[name]
    if c["kind"] == "bal":
        return dr.bal_cost(bal_problem(name), c.get("loss"))
    if c["kind"] == "quaternion":
        return cr.tape_cost(model(name).inner)
    return dr.blocks_cost(model(name))


def column_blocks(name):
    """[(first column, size)] of the parameter blocks in the model's column space."""
    c = CASES[name]
    if c["kind"] == "bal":
        prob = bal_problem(name)
        C = prob.num_cameras
        return [(9 * i, 9) for i in range(C)] + [(9 * C + 3 * p, 3) for p in range(prob.num_points)]
    if c["kind"] == "quaternion":
        return [(0, 3), (3, 3)]
    m = model(name)
    return [(int(m.off[b]), int(m.sizes[b])) for b in range(len(m.sizes))]


def block_offsets(name):
    """Per parameter block its first entry in the parameter array of the device problem."""
    if CASES[name]["kind"] == "quaternion":
        return [0, 4]
    return [start for start, _ in column_blocks(name)]


# ---- the device side -------------------------------------------------------------------------------------------------------------
def build_device(name):
    """The case as a skeres_amd problem: (problem, params DoubleArray, number of parameters, things to keep alive)."""
    import skeres_amd as sk
    from helpers import sk_loss
    c = CASES[name]
    if c["kind"] == "quaternion":
        return cc.build_device("tape-quaternion")
    if c["kind"] != "bal":
        problem, _, params, keep = _blocks_case(name).build()
        return problem, params, len(_blocks_case(name).x), keep
    prob = bal_problem(name)
    C = prob.num_cameras
    params = sk.RichDoubleArray.fromArray(prob.parameters)
    problem = sk.Problem()
    offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
    loss = sk_loss(c["loss"]) if c.get("loss") else sk.PredefinedLossFunctions.trivialLoss()
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    keep = [loss]
    if c.get("subset"):
        fixed = sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8])
        keep.append(fixed)
        for i in range(C):
            if i not in dc.CONST_CAMS:
                problem.setParameterization(params.slice(9 * i), fixed)
    for i in dc.CONST_CAMS:
        problem.setParameterBlockConstant(params.slice(9 * i))
    for q in c.get("const_pts", ()):
        problem.setParameterBlockConstant(params.slice(9 * C + 3 * q))
    return problem, params, prob.num_parameters, keep


@functools.lru_cache(maxsize=None)
def problem_order(name):
    """Per block of the case its index in the device problem's own order (first mention): the tie-break of the greedy visit."""
    problem, params, _, keep = build_device(name)
    order = [problem.parameterBlockIndex(params.slice(int(o))) for o in block_offsets(name)]
    assert sorted(order) == list(range(len(order)))
    return tuple(order)


def device_options(name, schur=True, **override):
    import skeres_amd as sk
    c = CASES[name]
    opt = dict(c.get("options", {}))
    opt["max_num_iterations"] = c["kmax"]
    opt.update(override)
    o = sk.Solver.Options()
    o.setLinearSolverType(opt.pop("linear_solver_type", sk.LinearSolverType.CGNR))
    o.setMaxNumIterations(opt.pop("max_num_iterations"))
    if schur is not None:
        o.setSchurElimination(schur)
    if "preconditioner" in opt:
        o.setPreconditionerType({"identity": sk.PreconditionerType.IDENTITY, "jacobi": sk.PreconditionerType.JACOBI}[opt.pop("preconditioner")])
    if "eta" in opt:
        o.setEta(opt.pop("eta"))
    if "max_linear_solver_iterations" in opt:
        o.setMaxLinearSolverIterations(opt.pop("max_linear_solver_iterations"))
    assert not opt, opt
    return o


# ---- the references --------------------------------------------------------------------------------------------------------------
def _options(name, override):
    o = dict(CASES[name].get("options", {}))
    o["max_num_iterations"] = CASES[name]["kmax"]
    o.update(override)
    return o


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, defect=None, **override):
    """(x, log) of the Schur reference on case `name`; shared by the tests, not to be modified."""
    return csr.solve(model(name), cost(name), x0(name), _options(name, override), dtype=LD if long_double else np.float64,
                     blocks=column_blocks(name), order=problem_order(name), defect=defect)


@functools.lru_cache(maxsize=None)
def full_reference(name, **override):
    """(x, log) of cgnr_reference (no elimination) on the same case, or with exact=True of the exact step."""
    o = _options(name, override)
    exact = o.pop("exact", False)
    return cr.solve(model(name), cost(name), x0(name), o, blocks=column_blocks(name), exact=exact)


@functools.lru_cache(maxsize=None)
def plan(name):
    return csr.plan(model(name), x0(name), column_blocks(name), problem_order(name))


@functools.lru_cache(maxsize=None)
def final_cost_gap(name="bal-small"):
    """Relative gap between the reference's Schur-CG final cost and its exact-step final cost, both solved to convergence (the
    default tolerances): what a comparison with a factorisation solver may be held to, as cgnr_cases.chain_final_cost_gap."""
    a = reference(name, max_num_iterations=50)[1][-1]["cost"]
    b = full_reference(name, max_num_iterations=50, exact=True)[1][-1]["cost"]
    gap = abs(a - b) / abs(b)
    print("%s: final cost Schur CG %.17g exact steps %.17g relative gap %.3e" % (name, a, b, gap), flush=True)
    return gap
