"""The cases of Problem::Evaluate (tests/test_evaluate_cpu.py, tests/test_gpu_evaluate.py): the smallest problems at which each
part of sk_problem_evaluate can go wrong, as data that both the numpy reference (tests/evaluate_reference.py) and the product
(build()) read.

A Case holds one flat parameter vector cut into parameter blocks, and residual blocks
    (functor id, captured constants, [parameter block indices], loss spec or None, kind)
kind: "dev" a registered device functor, "tape" the recorded Snavely functor, "host" a host callback answering from oracle.evaluate,
"bulk" the whole list added in one addResidualBlocks call.  Loss specs and parameterizations are the oracle's tuples."""
import numpy as np

import oracle

SNAVELY, EXPONENTIAL, F1, F2, F3, F4, BINARY_SCALAR, BINARY_VECTOR3, TEN_PARAMETER, QUATERNION_ROTATION = 1, 2, 3, 4, 5, 6, 7, 8, 9, 12


class Case:
    def __init__(self, name, x, sizes, blocks, snavely=False, parameterizations=None, constant=(), registered=(), apply_loss=True,
                 residual_blocks=None, parameter_blocks=None, bal_shape=None):
        self.name = name
        self.x = np.asarray(x, dtype=np.float64)
        self.sizes = list(sizes)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        assert self.off[-1] == len(self.x)
        self.blocks = blocks
        self.snavely = snavely                      # residuals in pixels: atol 1e-9 (else 1e-12)
        self.parameterizations = parameterizations or {}   # parameter block -> oracle parameterization tuple
        self.constant = set(constant)               # parameter blocks set constant
        self.registered = list(registered)          # parameter blocks added up front (addParameterBlock), in this order
        self.apply_loss = apply_loss
        self.residual_blocks = residual_blocks      # None: all
        self.parameter_blocks = parameter_blocks    # None: all
        self.bal_shape = bal_shape                  # (cameras, points) when x is a BAL vector and block c / C + p its camera / point

    def first_seen(self):
        order, seen = [], set()
        for b in self.registered + [q for blk in self.blocks for q in blk[2]]:
            if b not in seen:
                seen.add(b)
                order.append(b)
        return order

    def build(self):
        """The case as a skeres_amd Problem: (problem, EvaluateOptions or None, params DoubleArray, things to keep alive)."""
        import skeres_amd as sk
        from helpers import sk_loss
        params = sk.RichDoubleArray.fromArray(self.x)
        block = lambda b: params.slice(int(self.off[b]))
        problem, keep, losses = sk.Problem(), [], {}

        def loss_of(spec):
            if spec is None:
                return None
            if repr(spec) not in losses:
                losses[repr(spec)] = sk_loss(spec)
            return losses[repr(spec)]

        def parameterization(b):
            p = self.parameterizations.get(b)
            if p is None:
                return None
            P = sk.PredefinedLocalParameterizations
            made = {"quaternion": P.quaternion, "homogeneous": lambda: P.homogeneousVector(self.sizes[b]),
                    "subset": lambda: P.subset(self.sizes[b], list(p[1])), "identity": lambda: P.identity(self.sizes[b])}[p[0]]()
            keep.append(made)
            return made
        for b in self.registered:
            problem.addParameterBlock(block(b), self.sizes[b], parameterization(b))
        if self.blocks and self.blocks[0][4] == "bulk":
            fid, loss = self.blocks[0][0], self.blocks[0][3]
            offs = np.array([[self.off[q] for q in blk[2]] for blk in self.blocks], dtype=np.int64)
            problem.addResidualBlocks(fid, np.array([blk[1] for blk in self.blocks]), loss_of(loss), params, offs)
        else:
            recorded = None
            for fid, consts, pbs, loss, kind in self.blocks:
                if kind == "dev":
                    nres, sizes, _ = oracle.functor_info(fid)
                    functor = sk.AutoDiffCostFunctor(nres, *sizes, consts=consts)
                    functor.FUNCTOR_ID = fid
                    cost = functor.toAutoDiffCostFunction()
                elif kind == "tape":
                    from skeres_amd.examples.traced_functors import TracedSnavelyReprojectionError
                    recorded = recorded or TracedSnavelyReprojectionError(0.0, 0.0)
                    cost = recorded.withCaptured(*consts).toAutoDiffCostFunction()
                else:
                    cost = _OracleCallback(fid, consts, fail=(kind == "host_fails"))
                keep.append(cost)
                problem.addResidualBlock(cost, loss_of(loss), *[block(q) for q in pbs])
        for b, p in self.parameterizations.items():
            if b not in self.registered:
                problem.setParameterization(block(b), parameterization(b))
        for b in sorted(self.constant):
            problem.setParameterBlockConstant(block(b))
        options = None
        if not self.apply_loss or self.residual_blocks is not None or self.parameter_blocks is not None:
            options = sk.Problem.EvaluateOptions()
            options.setApplyLossFunction(self.apply_loss)
            if self.residual_blocks is not None:
                options.setResidualBlocks(self.residual_blocks)
            if self.parameter_blocks is not None:
                options.setParameterBlocks([block(b) for b in self.parameter_blocks])
        return problem, options, params, keep


def _OracleCallback(fid, consts, fail=False):
    """A host cost function (the director path) that answers from oracle.evaluate."""
    import skeres_amd as sk
    nres, sizes, _ = oracle.functor_info(fid)

    class Callback(sk.SizedCostFunction):
        def __init__(self):
            super().__init__(nres, *sizes)

        def evaluate(self, parameters, residuals, jacobians):
            if fail:
                return False
            ok, r, jac = oracle.evaluate(fid, consts, parameters)
            residuals[:] = r
            if jacobians is not None:
                for q, j in enumerate(jacobians):
                    if j is not None:
                        j[:] = jac[q]
            return ok
    return Callback()


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def powell():
    # functors added F3, F1, F4, F2: rows follow the order added across four functor groups; first sighting orders the columns
    # x2, x3, x1, x4, so F1 (x1, x2) has its second block in the lower column
    blocks = [(F3, [], [1, 2], None, "dev"), (F1, [], [0, 1], None, "dev"), (F4, [], [0, 3], None, "dev"), (F2, [], [2, 3], None, "dev")]
    return Case("powell", [3.0, -1.0, 0.0, 1.0], [1, 1, 1, 1], blocks)


def curve_robust(apply_loss=True):
    from helpers import robust_curve_fitting_data
    blocks = [(EXPONENTIAL, [x, y], [0, 1], ("cauchy", 0.5), "dev") for x, y in robust_curve_fitting_data()]
    return Case("curve_robust" if apply_loss else "curve_robust_noloss", [0.1, 0.2], [1, 1], blocks, apply_loss=apply_loss)


def mixed_sizes():
    rng = np.random.default_rng(5)
    sizes = [2] * 5 + [1] * 12          # blocks 0..4 of size 2, 5..16 of size 1
    ones = list(range(5, 17))
    blocks = [(BINARY_VECTOR3, [0.7], [0, 1], None, "dev"),
              (TEN_PARAMETER, [], ones[:10], None, "dev"),
              (BINARY_SCALAR, [1.3], [2, 3], ("huber", 0.3), "dev"),
              (BINARY_VECTOR3, [-0.4], [1, 0], None, "dev"),             # second block in the lower column
              (TEN_PARAMETER, [], ones[2:][::-1], ("cauchy", 1.0), "dev"),   # ten blocks in descending column order
              (BINARY_SCALAR, [0.2], [4, 2], None, "dev"),
              (BINARY_VECTOR3, [2.0], [3, 4], ("huber", 0.5), "dev"),
              (TEN_PARAMETER, [], [ones[i] for i in (11, 0, 10, 1, 9, 2, 8, 3, 7, 4)], None, "dev"),
              (BINARY_SCALAR, [-1.1], [1, 4], None, "dev")]
    return Case("mixed_sizes", rng.normal(0, 1, sum(sizes)), sizes, blocks)


def manifolds():
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, 20)
    x[0:4] /= np.linalg.norm(x[0:4])     # the quaternion block is a unit quaternion
    blocks = []
    for i in range(20):
        c = np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 1, 3)])
        blocks.append((QUATERNION_ROTATION, list(c), [i % 5], ("huber", 0.7) if i % 2 == 0 else None, "dev"))
    pz = {0: ("quaternion",), 1: ("homogeneous",), 2: ("subset", [0])}
    return Case("manifolds", x, [4] * 5, blocks, parameterizations=pz, constant=[3], registered=[0, 1, 2, 3, 4])


_BAL_SMALL = None


def _bal_small_problem():
    global _BAL_SMALL
    if _BAL_SMALL is None:
        from skeres_amd import bal
        _BAL_SMALL = bal.generate(6, 40, 170, seed=3)
    return _BAL_SMALL


def _bal_blocks(prob, kind, order, loss_of):
    C = prob.num_cameras
    return [(SNAVELY, list(prob.observations[i]), [int(prob.camera_index[i]), C + int(prob.point_index[i])], loss_of(k), kind)
            for k, i in enumerate(order)]


def bal_small(kind="dev", name="bal_small", **kw):
    prob = _bal_small_problem()
    C, P = prob.num_cameras, prob.num_points
    order = list(np.random.default_rng(21).permutation(prob.num_observations))   # residual blocks added in a shuffled order
    blocks = _bal_blocks(prob, kind, order, lambda k: ("huber", 1.0) if k % 2 == 0 else None)
    fid, consts, pbs, _, _ = blocks[7]
    blocks.append((fid, [consts[0] + 0.25, consts[1] - 0.5], pbs, ("huber", 1.0), kind))   # one (camera, point) pair observed twice
    return Case(name, prob.parameters, [9] * C + [3] * P, blocks, snavely=True, parameterizations={1: ("subset", [6, 7, 8])},
                constant=[0, C + 0], bal_shape=(C, P), **kw)


def bal_tape():
    return bal_small("tape", "bal_tape")


def bal_host(failing=False):
    prob = _bal_small_problem()
    C, P = prob.num_cameras, prob.num_points
    blocks = _bal_blocks(prob, "dev", range(30), lambda k: None)
    for i in (3, 9, 15, 21, 27):
        blocks[i] = blocks[i][:4] + ("host_fails" if failing and i == 15 else "host",)
    return Case("bal_host", prob.parameters, [9] * C + [3] * P, blocks, snavely=True, bal_shape=(C, P))


def wide_column():
    from helpers import bal_from_tracks
    prob = bal_from_tracks(3, [[0, 1, 2]] * 200, seed=4)     # every point seen by every camera: 600 blocks, a camera's column block has 200 of them (400 rows)
    blocks = _bal_blocks(prob, "dev", range(prob.num_observations), lambda k: None)
    return Case("wide_column", prob.parameters, [9] * 3 + [3] * 200, blocks, snavely=True, bal_shape=(3, 200))


def subsets():
    base = bal_small()
    C, P = base.bal_shape
    ids = list(range(len(base.blocks)))[::3][::-1]           # every third id, descending
    pbs = [C + p for p in range(P)][::-1] + [2, 0]            # the points in reverse, then cameras 2 and 0
    return bal_small(name="subsets", residual_blocks=ids, parameter_blocks=pbs)


def medium():
    from skeres_amd import bal
    prob = bal.generate(50, 4000, 18000)
    blocks = _bal_blocks(prob, "bulk", range(prob.num_observations), lambda k: ("huber", 1.0))
    return Case("medium", prob.parameters, [9] * 50 + [3] * 4000, blocks, snavely=True, bal_shape=(50, 4000))


CASES = {"powell": powell, "curve_robust": curve_robust, "curve_robust_noloss": lambda: curve_robust(False), "mixed_sizes": mixed_sizes,
         "manifolds": manifolds, "bal_small": bal_small, "bal_tape": bal_tape, "bal_host": bal_host, "wide_column": wide_column,
         "subsets": subsets, "medium": medium}
_MADE = {}


def case(name):
    if name not in _MADE:
        _MADE[name] = CASES[name]()
    return _MADE[name]
