"""The cases of the covariance tests (tests/test_covariance_cpu.py, tests/test_gpu_covariance.py) and their references
(tests/covariance_reference.py), computed once per process.  Each case is the smallest shape that reaches a path; the generators
are those of tests/cgnr_cases.py and tests/evaluate_cases.py, imported unchanged.

    curve            ExponentialResidual on the 67 samples of tests/golden/curve_fitting_data.txt: N = 2 (the functor's two blocks
                     of size 1), also held to the closed form of a 2 x 2 inverse
    bal-small        (6, 40, 200), seed 1, cameras 0 and 1 constant: N = 156, H spans two 128-blocks, the border a third
    bal-robust       (16, 600, 2600), seed 11, Huber(1), subset intrinsics, point 5 constant: N = 1881, a camera's diagonal pair is
                     three parts; compute_blocks over the 14 moving cameras and points 0..20 (20 that move: k = 84 + 60 = 144, two
                     border block rows; point 5, constant, gives zero blocks); loss on and off
    bal-duplicate    bal-small with a second residual block on an existing (camera, point) pair: a two-term off-diagonal pair
    chain            cgnr_cases.chain_case(num_blocks=700, hub_blocks=320), block 3 constant.  (The hub's partners are the even blocks
                     20, 22, ..., 658, so 320 of them need 660 blocks or more: the generator indexes past a chain of 400.  The hub's
                     diagonal pair has 320 + 2 terms: five full parts and a partial one; every fifth neighbour pair is listed in
                     reverse column order.  The chain's normal matrix has one eigenvalue that is exactly zero — a gauge freedom of its
                     products, which the damped solvers never notice —, so block 3 is held constant as cameras 0 and 1 are in the
                     bundle-adjustment cases: N = 1398, kappa_2 of the scaled normal matrix 8.9e5, found with the reference alone.)
    tape-quaternion  the recorded functor of cgnr_cases over a 4-block with the quaternion parameterization and a 3-block
    callback         curve with host-callback blocks

Gauge-free bundle adjustment (no camera held) is not a case: its normal matrix is singular in exact arithmetic, and whether the
floating-point pivots of an exactly singular matrix fall below min_reciprocal_condition_number is not a contract."""
import functools

import numpy as np

from skeres_amd import bal
import step_check as sc
import dogleg_cases as dc
import cgnr_cases as cc
import evaluate_cases as ec
import covariance_reference as cv

LD = np.longdouble
U = cv.U
CHAIN_BLOCKS, CHAIN_HUB_BLOCKS, CHAIN_HELD = 700, 320, 3


class CovCase:
    """blocks: cv.Block per parameter block; offsets: of the blocks in x; model(loss): the step_check model; pairs: requested block
    index pairs (all_of: blocks for compute_blocks instead); build(loss): the device problem."""

    def __init__(self, name, x, blocks, offsets, model, pairs=None, all_of=None, build=None, has_loss=False):
        self.name, self.x, self.blocks, self.offsets = name, np.asarray(x, dtype=np.float64), blocks, list(offsets)
        self.model, self.all_of, self.build, self.has_loss = model, all_of, build, has_loss
        self.pairs = pairs if pairs is not None else [(a, b) for i, a in enumerate(all_of) for b in all_of[i:]]


def _bal_case(name, prob, loss=None, subset=False, const_pts=(), pairs=None, all_of=None):
    C, P = prob.num_cameras, prob.num_points
    cam_mask = np.full(C, 0b111000000 if subset else 0, dtype=np.int32)
    cam_mask[list(dc.CONST_CAMS)] = 0x1ff
    pt_mask = np.zeros(P, dtype=np.int32)
    pt_mask[list(const_pts)] = 7
    blocks, offsets = [], []
    for i in range(C):
        const = i in dc.CONST_CAMS
        held = [6, 7, 8] if subset and not const else []
        free = [9 * i + j for j in range(9) if j not in held]
        blocks.append(cv.Block(9, len(free), free, const, ("subset", held) if held else None))
        offsets.append(9 * i)
    for p in range(P):
        blocks.append(cv.Block(3, 3, [9 * C + 3 * p + j for j in range(3)], p in const_pts, None))
        offsets.append(9 * C + 3 * p)

    def model(with_loss=True):
        return sc.BalModel(prob, loss=loss if with_loss else None, cam_mask=cam_mask, pt_mask=pt_mask)

    def build(with_loss=True):
        import skeres_amd as sk
        from helpers import sk_loss
        params = sk.RichDoubleArray.fromArray(prob.parameters)
        problem = sk.Problem()
        offs = np.stack([9 * prob.camera_index.astype(np.int64), 9 * C + 3 * prob.point_index.astype(np.int64)], axis=1)
        lf = sk_loss(loss) if loss and with_loss else sk.PredefinedLossFunctions.trivialLoss()
        problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, lf, params, offs)
        keep = [lf]
        if subset:
            fixed = sk.PredefinedLocalParameterizations.subset(9, [6, 7, 8])
            keep.append(fixed)
            for i in range(C):
                if i not in dc.CONST_CAMS:
                    problem.setParameterization(params.slice(9 * i), fixed)
        for i in dc.CONST_CAMS:
            problem.setParameterBlockConstant(params.slice(9 * i))
        for q in const_pts:
            problem.setParameterBlockConstant(params.slice(9 * C + 3 * q))
        return problem, params, keep

    return CovCase(name, prob.parameters, blocks, offsets, model, pairs, all_of, build, has_loss=loss is not None)


def _bal_small_pairs(C):
    cam, pt = (lambda i: i), (lambda p: C + p)
    return [(cam(2), cam(2)), (cam(2), cam(3)), (cam(3), pt(5)), (pt(5), pt(5)), (pt(7), pt(5)), (cam(0), cam(2)), (cam(0), cam(0))]


def _bal_small():
    prob = cc.bal_problem("bal-small")
    return _bal_case("bal-small", prob, pairs=_bal_small_pairs(prob.num_cameras))


def _bal_robust():
    prob = cc.bal_problem("bal-robust")
    C = prob.num_cameras
    moving = [i for i in range(C) if i not in dc.CONST_CAMS] + [C + p for p in range(21)]   # (point 5 is constant: 20 points move)
    return _bal_case("bal-robust", prob, loss=("huber", 1.0), subset=True, const_pts=(5,), all_of=moving)


def duplicate_observation():
    """(index of the observation that bal-duplicate repeats, its camera, its point): the first one on a moving camera."""
    prob = cc.bal_problem("bal-small")
    i = int(np.flatnonzero(prob.camera_index >= 2)[0])
    return i, int(prob.camera_index[i]), int(prob.point_index[i])


def _bal_duplicate():
    base = cc.bal_problem("bal-small")
    i, c, p = duplicate_observation()
    obs = np.concatenate([base.observations, [base.observations[i] + np.array([0.25, -0.5])]])
    prob = bal.BalProblem(base.num_cameras, base.num_points, np.append(base.camera_index, c).astype(np.int32),
                          np.append(base.point_index, p).astype(np.int32), np.ascontiguousarray(obs), base.parameters.copy())
    C = prob.num_cameras
    return _bal_case("bal-duplicate", prob, pairs=_bal_small_pairs(C) + [(c, C + p), (C + p, C + p), (c, c)])


def _blocks_case(name, case, pairs):
    """An evaluate_cases.Case without parameterizations (constant blocks: case.constant) as a CovCase."""
    blocks = [cv.Block(s, s, list(range(int(o), int(o) + s)), b in case.constant, None) for b, (s, o) in enumerate(zip(case.sizes, case.off))]

    def model(with_loss=True):
        return sc.BlocksModel(case.sizes, [blk[:4] for blk in case.blocks], [("constant",) if b in case.constant else None for b in range(len(case.sizes))])

    def build(with_loss=True):
        problem, _, params, keep = case.build()
        return problem, params, keep

    return CovCase(name, case.x, blocks, case.off[:-1], model, pairs, None, build)


def _curve(kind="dev", name="curve"):
    from helpers import curve_fitting_data
    blocks = [(ec.EXPONENTIAL, [float(x), float(y)], [0, 1], None, kind) for x, y in curve_fitting_data()]
    return _blocks_case(name, ec.Case(name, [0.3, 0.1], [1, 1], blocks), [(0, 0), (0, 1), (1, 1)])


def _chain():
    case = cc.chain_case(num_blocks=CHAIN_BLOCKS, hub_blocks=CHAIN_HUB_BLOCKS)
    case.constant = {CHAIN_HELD}
    hub = cc.CHAIN_HUB
    return _blocks_case("chain", case, [(hub, 0), (hub, CHAIN_BLOCKS - 1), (6, 5), (hub, hub)])


def _quaternion():
    f, cap, x0 = cc.quaternion_setup()
    blocks = [cv.Block(4, 3, [0, 1, 2], False, ("quaternion",)), cv.Block(3, 3, [3, 4, 5], False, None)]

    def build(with_loss=True):
        problem, params, _, keep = cc.build_device("tape-quaternion")
        return problem, params, keep

    return CovCase("tape-quaternion", x0, blocks, [0, 4], lambda with_loss=True: cc.model("tape-quaternion"), [(0, 0), (0, 1), (1, 1)], None, build)


CASES = {"curve": _curve, "bal-small": _bal_small, "bal-robust": _bal_robust, "bal-duplicate": _bal_duplicate, "chain": _chain,
         "tape-quaternion": _quaternion, "callback": lambda: _curve("host", "callback")}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def normal_matrix(name, long_double=False, with_loss=True):
    """(H, number of normal-matrix pairs) of the reference; shared, not to be modified."""
    c = case(name)
    return cv.normal_matrix(c.model(with_loss), c.x, c.blocks, LD if long_double else np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, with_loss=True):
    """The reference's covariance blocks of the case's pairs (covariance_reference.covariance); shared, not to be modified."""
    c = case(name)
    H, npairs = normal_matrix(name, long_double, with_loss)
    out = cv.covariance(H, c.blocks, c.x, c.offsets, c.pairs, LD if long_double else np.float64)
    out["normal_matrix_pairs"] = npairs
    return out


@functools.lru_cache(maxsize=None)
def self_deviation(name, with_loss=True):
    """D: the float64 restatement against the long-double one, in the metric."""
    c = case(name)
    return cv.deviation(reference(name, False, with_loss), reference(name, True, with_loss), c.pairs)


def tolerance(name, with_loss=True):
    """The bound of the inversion test: max(16 D, 64 u)."""
    return max(16 * self_deviation(name, with_loss), 64 * U)


# ---- the device side -------------------------------------------------------------------------------------------------------------
def handles(c, params):
    return [params.slice(int(o)) for o in c.offsets]


def compute(c, with_loss=True, apply_loss=True, options=None):
    """(Covariance, ok, problem, params, block handles, keep) of one compute of the case's pairs on the device."""
    import skeres_amd as sk
    problem, params, keep = c.build(with_loss)
    h = handles(c, params)
    if options is None:
        options = sk.Covariance.Options()
    options.applyLossFunction(apply_loss)
    cov = sk.Covariance(options)
    if c.all_of is not None:
        ok = cov.compute([h[b] for b in c.all_of], problem)
    else:
        ok = cov.compute([(h[a], h[b]) for a, b in c.pairs], problem)
    return cov, ok, problem, params, h, keep


def device_blocks(c, cov, h):
    """What the getters return for the case's pairs and the diagonal blocks of every named block, as covariance() lays it out."""
    out = {"tangent": {}, "ambient": {}}
    named = sorted({q for ab in c.pairs for q in ab})
    for a, b in list(c.pairs) + [(q, q) for q in named if (q, q) not in c.pairs]:
        try:
            out["tangent"][(a, b)] = cov.getCovarianceBlockInTangentSpace(h[a], h[b])
            out["ambient"][(a, b)] = cov.getCovarianceBlock(h[a], h[b])
        except ValueError:
            if (a, b) in c.pairs:
                raise
    return out


def device_jacobian(c, problem, h, apply_loss=True):
    """The CRSMatrix sk_problem_evaluate returns at the same point, its columns the blocks in the case's order."""
    import skeres_amd as sk
    o = sk.Problem.EvaluateOptions()
    o.setApplyLossFunction(apply_loss)
    o.setParameterBlocks(h)
    return problem.evaluate(o, cost=False, residuals=False, gradient=False, jacobian=True)["jacobian"]
