"""The cases of the CGNR tests and their reference trajectories (tests/cgnr_reference.py), computed once per process.  Each case
is the smallest shape that can break a particular kernel path:

    bal-small        (6, 40, 200) of tests/dogleg_cases.py, cameras 0 and 1 constant, JACOBI, default eta: tangent sizes 9 and 3,
                     partial workgroups, every column block a single part
    bal-identity     the same with IDENTITY
    bal-robust       (16, 600, 2600), Huber, subset intrinsics, a constant point: a camera's 160-odd slots are three parts
    bal-reset        bal-small with eta = 1e-8: some solve takes >= 11 CG iterations, so the residual reset at iteration 10 runs and
                     one solve spans two batches
    bal-limit        max_linear_solver_iterations = 3: status 1, the step still used
    chain            2100 blocks of size 2 (n = 4200: the dot products cross a 4096 reduction chunk, the fused update has nine
                     workgroups) joined by BINARY_VECTOR3 residuals between neighbours, every fifth listed in reverse column order;
                     a hub block in 320 more residual blocks (five full parts and a partial one); the two ends with a single slot
    at-optimum       HelloWorld at x = 10: zero gradient
    tape-quaternion  a recorded functor over a 4-block with the quaternion parameterization and a 3-block.  step_check.TapeModel gives the
                     ambient Jacobian; cgnr_reference.QuaternionTangentModel multiplies it by dPlus/ddelta and steps through Plus,
                     so the case IS held to the reference, field by field, like the others.

Seeds, perturbations and the iterations compared (kmax) were chosen with the reference alone, in double and in long double, so that
the two take the same number of CG iterations in every solve, zeta stays away from eta at the stopping iteration and the one before,
and the logs agree ten times inside the tolerances of the device comparison; tests/test_cgnr_cpu.py asserts that."""
import functools

import numpy as np

import oracle
from skeres_amd import bal
import step_check as sc
import dogleg_reference as dr
import dogleg_cases as dc
import cgnr_reference as cr
import evaluate_cases as ec

LD = np.longdouble
TOL = dc.TOL   # the project's tolerances for oracle comparisons: cost 1e-10, the other fields 1e-8 (relative, per iteration)
ZETA_MARGIN = 1e-3

_SMALL = dict(kind="bal", shape=(6, 40, 200), seed=1, perturb=dc.DEFAULT_PERTURB)
CASES = {
    "bal-small": dict(_SMALL, kmax=4),
    "bal-identity": dict(_SMALL, kmax=1, options=dict(preconditioner="identity")),
    "bal-robust": dict(kind="bal", shape=(16, 600, 2600), seed=11, perturb=dc.DEFAULT_PERTURB, kmax=4, loss=("huber", 1.0), subset=True, const_pts=(5,)),
    "bal-reset": dict(_SMALL, kmax=3, options=dict(eta=1e-8)),
    "bal-limit": dict(_SMALL, kmax=4, options=dict(max_linear_solver_iterations=3)),
    "chain": dict(kind="chain", kmax=3),
    "at-optimum": dict(kind="hello", kmax=2),
    "tape-quaternion": dict(kind="quaternion", kmax=4),
}

CHAIN_BLOCKS, CHAIN_HUB, CHAIN_HUB_BLOCKS = 2100, 7, 320


# ---- the problems ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bal_problem(name):
    c = CASES[name]
    return bal.generate(*c["shape"], seed=c["seed"], perturb=c["perturb"])


def bal_masks(name):
    c, prob = CASES[name], bal_problem(name)
    cam_mask = np.full(prob.num_cameras, 0b111000000 if c.get("subset") else 0, dtype=np.int32)
    cam_mask[list(dc.CONST_CAMS)] = 0x1ff
    pt_mask = np.zeros(prob.num_points, dtype=np.int32)
    pt_mask[list(c.get("const_pts", ()))] = 7
    return cam_mask, pt_mask


def chain_case(num_blocks=CHAIN_BLOCKS, hub_blocks=CHAIN_HUB_BLOCKS, seed=3):
    """The chain as an evaluate_cases.Case (one bulk addResidualBlocks call).  BINARY_VECTOR3's three residuals between blocks
    (x0, x1) and (y0, y1) vanish together only where x0 y0 = 0, x1 y1 = c and x0 x1 + y0 y1 = -10 c: the hidden truth has even
    blocks (0, V) and odd blocks (-10 V, w_k), so every pair (even, odd) — the neighbours, and the odd hub with its even partners
    — is consistent with c = V w_k.  c carries noise (a small-residual problem: Gauss-Newton steps converge fast to a cost that
    is not zero); the start is the truth perturbed."""
    assert CHAIN_HUB % 2 == 1
    rng = np.random.default_rng(seed)
    V = 0.2
    truth = np.zeros((num_blocks, 2))
    truth[0::2, 1] = V
    truth[1::2, 0] = -10 * V
    truth[1::2, 1] = rng.uniform(0.5, 1.5, len(truth[1::2]))
    pairs = [((i + 1, i) if i % 5 == 0 else (i, i + 1)) for i in range(num_blocks - 1)]
    stride = 2 * max(1, (num_blocks - 40) // (2 * hub_blocks))
    for k in range(hub_blocks):
        j = 20 + stride * k
        pairs.append((CHAIN_HUB, j) if k % 2 == 0 else (j, CHAIN_HUB))
    blocks = [(ec.BINARY_VECTOR3, [float(truth[a, 1] * truth[b, 1]) + float(rng.normal(0, 0.01))], [a, b], None, "bulk") for a, b in pairs]
    x0 = (truth + rng.uniform(-0.02, 0.02, truth.shape)).ravel()
    return ec.Case("chain", x0, [2] * num_blocks, blocks)


@functools.lru_cache(maxsize=None)
def _chain():
    return chain_case()


def hello_case():
    return ec.Case("at-optimum", [10.0], [1], [(oracle.HELLO_WORLD, [], [0], None, "dev")])


def _quaternion_functor():
    import skeres_amd as sk
    from skeres_amd import tape as T

    class TracedQuaternionPose(sk.TracedCostFunctor):
        """r = R(q) p + u - t for q = (w, x, y, z), normalised first, and a translation block u; p and t captured
        (QuaternionRotationError with a second block, written generically)."""

        def __init__(self, *captured):
            super().__init__(3, 4, 3, captured=captured or (0.0,) * 6)

        def apply(self, q, u):
            c = self.captured_values()
            scale = 1.0 / T.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
            a, b, cc, d = q[0] * scale, q[1] * scale, q[2] * scale, q[3] * scale
            t2, t3, t4, t5, t6, t7, t8, t9, t1 = a * b, a * cc, a * d, -(b * b), b * cc, b * d, -(cc * cc), cc * d, -(d * d)
            return [((2.0 * (((t8 + t1) * c[0] + (t6 - t4) * c[1]) + (t3 + t7) * c[2]) + c[0]) + u[0]) - c[3],
                    ((2.0 * (((t4 + t6) * c[0] + (t5 + t1) * c[1]) + (t9 - t2) * c[2]) + c[1]) + u[1]) - c[4],
                    ((2.0 * (((t7 - t3) * c[0] + (t2 + t9) * c[1]) + (t5 + t8) * c[2]) + c[2]) + u[2]) - c[5]]
    return TracedQuaternionPose()


@functools.lru_cache(maxsize=None)
def quaternion_setup(num_blocks=70, seed=2):
    """(functor, captured [nb, 6], x0 = (q, u)): points rotated by a hidden unit quaternion and shifted, plus noise; the start is
    another pose."""
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    u = rng.normal(0, 1, 3)
    p = rng.normal(0, 1, (num_blocks, 3)) + np.array([2.0, -1.0, 0.5])
    w, v = q[0], q[1:]
    t = p + 2 * np.cross(v, np.cross(v, p) + w * p) + u + rng.normal(0, 0.05, p.shape)
    q0 = q + rng.normal(0, 0.2, 4)
    q0 /= np.linalg.norm(q0)
    return _quaternion_functor(), np.concatenate([p, t], axis=1), np.concatenate([q0, u + rng.normal(0, 0.3, 3)])


def x0(name):
    kind = CASES[name]["kind"]
    if kind == "bal":
        return bal_problem(name).parameters
    if kind == "chain":
        return _chain().x
    if kind == "hello":
        return np.array([10.0])
    return quaternion_setup()[2]


@functools.lru_cache(maxsize=None)
def model(name):
    c = CASES[name]
    if c["kind"] == "bal":
        cam_mask, pt_mask = bal_masks(name)
        return sc.BalModel(bal_problem(name), loss=c.get("loss"), cam_mask=cam_mask, pt_mask=pt_mask)
    if c["kind"] in ("chain", "hello"):
        case = _chain() if c["kind"] == "chain" else hello_case()
        return sc.BlocksModel(case.sizes, [blk[:4] for blk in case.blocks])
    f, cap, _ = quaternion_setup()
    offs = np.tile(np.array([[0, 4]], dtype=np.int64), (cap.shape[0], 1))
    return cr.QuaternionTangentModel(sc.TapeModel(7, [(f.tape(), (4, 3), cap, offs, None)]))


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


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, **override):
    """(x, log) of the reference on case `name`; shared by the tests, not to be modified."""
    c = CASES[name]
    o = dict(c.get("options", {}))
    o["max_num_iterations"] = c["kmax"]
    o.update(override)
    exact = o.pop("exact", False)
    return cr.solve(model(name), cost(name), x0(name), o, dtype=LD if long_double else np.float64, blocks=column_blocks(name), exact=exact)


@functools.lru_cache(maxsize=None)
def chain_final_cost_gap():
    """Relative gap between the reference's CGNR final cost and its exact-step final cost on `chain`, both solved to convergence
    (the default tolerances): what a comparison of CGNR with a factorisation solver may be held to, at the level of the minimiser."""
    a = reference("chain", max_num_iterations=50)[1][-1]["cost"]
    b = reference("chain", max_num_iterations=50, exact=True)[1][-1]["cost"]
    gap = abs(a - b) / abs(b)
    print("chain: final cost CGNR %.17g exact steps %.17g relative gap %.3e" % (a, b, gap), flush=True)
    return gap


# ---- the device side -------------------------------------------------------------------------------------------------------------
def build_device(name):
    """The case as a skeres_amd problem: (problem, params DoubleArray, number of parameters, things to keep alive)."""
    import skeres_amd as sk
    from helpers import sk_loss
    c = CASES[name]
    if c["kind"] == "bal":
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
    if c["kind"] in ("chain", "hello"):
        case = _chain() if c["kind"] == "chain" else hello_case()
        problem, _, params, keep = case.build()
        return problem, params, len(case.x), keep
    f, cap, q0 = quaternion_setup()
    params = sk.RichDoubleArray.fromArray(q0)
    problem = sk.Problem()
    problem.addResidualBlocksTraced(f, cap, None, params, np.tile(np.array([[0, 4]], dtype=np.int64), (cap.shape[0], 1)))
    pz = sk.PredefinedLocalParameterizations.quaternion()
    problem.setParameterization(params.slice(0), pz)
    return problem, params, 7, [f, pz]


def device_options(name, **override):
    import skeres_amd as sk
    c = CASES[name]
    opt = dict(c.get("options", {}))
    opt["max_num_iterations"] = c["kmax"]
    opt.update(override)
    o = sk.Solver.Options()
    o.setLinearSolverType(opt.pop("linear_solver_type", sk.LinearSolverType.CGNR))
    o.setMaxNumIterations(opt.pop("max_num_iterations"))
    if "preconditioner" in opt:
        o.setPreconditionerType({"identity": sk.PreconditionerType.IDENTITY, "jacobi": sk.PreconditionerType.JACOBI}[opt.pop("preconditioner")])
    if "eta" in opt:
        o.setEta(opt.pop("eta"))
    if "max_linear_solver_iterations" in opt:
        o.setMaxLinearSolverIterations(opt.pop("max_linear_solver_iterations"))
    if "min_linear_solver_iterations" in opt:
        o.setMinLinearSolverIterations(opt.pop("min_linear_solver_iterations"))
    assert not opt, opt
    return o


def close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def compare_logs(log, ref, kmax, tol=TOL, factor=1.0, show=None):
    """Asserts the accepted / rejected pattern, the CG iteration count and every compared field of iterations 0..kmax; prints each
    figure first when asked to."""
    assert len(log) == len(ref) == kmax + 1, (len(log), len(ref))
    for k in range(kmax + 1):
        if show:
            print("%s k=%d cg %d / %d" % (show, k, log[k]["linear_solver_iterations"], ref[k]["linear_solver_iterations"]),
                  " ".join("%s %.17g / %.17g" % (f, log[k][f], ref[k][f]) for f in tol), flush=True)
    for k in range(kmax + 1):
        assert bool(log[k]["step_is_valid"]) == bool(ref[k]["step_is_valid"]), k
        assert bool(log[k]["step_is_successful"]) == bool(ref[k]["step_is_successful"]), k
        assert int(log[k]["linear_solver_iterations"]) == int(ref[k]["linear_solver_iterations"]), k
        for f, t in tol.items():
            assert close(log[k][f], ref[k][f], t * factor), (k, f, log[k][f], ref[k][f])


def deviation(a, b, fields=TOL):
    """The largest relative deviation per field between two logs of equal length."""
    out = {f: 0.0 for f in fields}
    for ea, eb in zip(a, b):
        for f in fields:
            if eb[f] != 0:
                out[f] = max(out[f], abs(ea[f] - eb[f]) / abs(eb[f]))
            elif ea[f] != 0:
                out[f] = float("inf")
    return out
