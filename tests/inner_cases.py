"""The cases of the inner-iteration tests (tests/test_inner_cpu.py, tests/test_gpu_inner.py) and their reference trajectories
(tests/inner_reference.py), computed once per process.  Each is the smallest shape that reaches a path, built from the case
builders of tests/cgnr_cases.py and tests/cgnr_schur_cases.py:

    bal-small        (6, 40, 200): two groups (the points, then the four moving cameras), every list a single part
    bal-small-schur  the same with the Schur elimination
    bal-identity     the same with preconditioner = identity
    bal-robust       (16, 600, 2600), Huber, subset intrinsics, a constant point: a camera's 160-odd slots are three parts, the busiest camera's 228 four
    quaternion       the recorded functor with 70 blocks: Plus on a manifold inside the inner solve, each block's list two parts
    chain            cgnr_cases.chain_case(CHAIN_BLOCKS, CHAIN_HUB_BLOCKS): a path needs two groups and the hub a third one; the hub
                     is a long block (its slot list is two parts)
    all-eliminated   three unrelated one-block residual blocks (with the Schur elimination: no CG iteration): one group takes all
                     of them and nothing is left for a second.  Not cgnr_schur_cases' r = 10 - x: its minimum is a cost of zero,
                     which the inner solves reach to rounding, and a cost of 1e-23 cannot be held to 1e-10.  Here each block is a
                     4-vector q in r = R(q) p - t with |t| != |p|, so the cost at the minimum is (|p| - |t|)^2 / 2 > 0.
    bal-points       bal-small with the caller's ordering: the points alone, in group 3 (compressed to 0)
    bal-tolerance    bal-small with inner_iteration_tolerance = 0.5: the refinement switches off after its first use
    bal-useful       bal-small from a start perturbed by N(0, 0.5) (seed 8): at iteration 2 the trust-region step raises the cost, the
                     refinement brings it below the current cost, and `useful` accepts a step whose rho (7.5e-5) is below
                     min_relative_decrease.  Found with the reference alone, over 40 seeds, three perturbations and three initial
                     radii: 60 such iterations, this one at the default radius with the largest rho.

Seeds and the iterations compared (kmax) were chosen with the reference alone by the rule of tests/test_inner_cpu.py."""
import functools

import numpy as np

from skeres_amd import bal
import step_check as sc
import dogleg_reference as dr
import cgnr_reference as cr
import cgnr_cases as cc
import cgnr_schur_cases as csc
import inner_reference as ir
import evaluate_cases as ec

LD = np.longdouble
TOL = cc.TOL

CHAIN_BLOCKS, CHAIN_HUB_BLOCKS = 145, 63

CASES = {
    "bal-small": dict(base="bal-small", kmax=3),
    "bal-small-schur": dict(base="bal-small", kmax=3, schur=True),
    "bal-identity": dict(base="bal-identity", kmax=1),      # (as in cgnr_cases: a later solve takes 28 unpreconditioned CG iterations)
    "bal-robust": dict(base="bal-robust", kmax=2),
    "quaternion": dict(base="quaternion", kmax=3),
    "chain": dict(base=None, own="chain", seed=2, kmax=2),
    "all-eliminated": dict(base=None, own="separate", seed=4, kmax=1, schur=True),
    "bal-points": dict(base="bal-small", kmax=3, ordering="points"),
    "bal-tolerance": dict(base="bal-small", kmax=3, tolerance=0.5),
    "bal-useful": dict(base="bal-small", kmax=2, perturb=(8, 0.5)),
}


@functools.lru_cache(maxsize=None)
def _chain(seed):
    return cc.chain_case(num_blocks=CHAIN_BLOCKS, hub_blocks=CHAIN_HUB_BLOCKS, seed=seed)


@functools.lru_cache(maxsize=None)
def _separate(seed):
    rng = np.random.default_rng(seed)
    x, blocks = [], []
    for b in range(3):
        q = rng.normal(0, 1, 4)
        x.extend(q / np.linalg.norm(q))
        p = rng.normal(0, 1, 3)
        t = rng.normal(0, 1, 3)
        t *= (1.2 + 0.1 * b) * np.linalg.norm(p) / np.linalg.norm(t)
        blocks.append((ec.QUATERNION_ROTATION, list(np.concatenate([p, t])), [b], None, "dev"))
    return ec.Case("all-eliminated", x, [4, 4, 4], blocks)


def _own(name):
    return {"chain": _chain, "separate": _separate}[CASES[name]["own"]](CASES[name]["seed"])


def kind(name):
    base = CASES[name]["base"]
    return "blocks" if base is None else csc.CASES[base]["kind"]


@functools.lru_cache(maxsize=None)
def _x0(name):
    base = CASES[name]["base"]
    x = np.asarray(_own(name).x, dtype=np.float64) if base is None else csc.x0(base)
    if "perturb" in CASES[name]:
        seed, scale = CASES[name]["perturb"]
        x = x + model(name).free * np.random.default_rng(seed).normal(0, scale, x.shape)
    return x


def x0(name):
    return _x0(name).copy()


@functools.lru_cache(maxsize=None)
def model(name):
    base = CASES[name]["base"]
    if base is None:
        case = _own(name)
        return sc.BlocksModel(case.sizes, [blk[:4] for blk in case.blocks])
    return csc.model(base)


def cost(name):
    base = CASES[name]["base"]
    return dr.blocks_cost(model(name)) if base is None else csc.cost(base)


def column_blocks(name):
    base = CASES[name]["base"]
    if base is None:
        m = model(name)
        return [(int(m.off[b]), int(m.sizes[b])) for b in range(len(m.sizes))]
    return csc.column_blocks(base)


def block_offsets(name):
    base = CASES[name]["base"]
    return [start for start, _ in column_blocks(name)] if base is None else csc.block_offsets(base)


def ambient(name, b):
    """The slice of block b in the parameter array."""
    if kind(name) == "quaternion":
        return slice(0, 4) if b == 0 else slice(4, 7)
    start, size = column_blocks(name)[b]
    return slice(start, start + size)


def options(name):
    base = CASES[name]["base"]
    o = {} if base is None else dict(csc.CASES[base].get("options", {}))
    o["max_num_iterations"] = CASES[name]["kmax"]
    return o


# ---- a block's own residual blocks ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def local(name, b):
    """What inner_reference.block_solve takes for block b: a model and a cost over the block's residual blocks alone."""
    k, m = kind(name), model(name)
    start, size = column_blocks(name)[b]
    cols = [c for c in range(start, start + size) if m.free[c]]
    out = dict(cols=cols, start=start, ambient=ambient(name, b))
    if k == "bal":
        base = CASES[name]["base"]
        prob, c = csc.bal_problem(base), csc.CASES[base]
        C = prob.num_cameras
        sel = np.flatnonzero(prob.camera_index == b) if b < C else np.flatnonzero(prob.point_index == b - C)
        sub = bal.BalProblem(prob.num_cameras, prob.num_points, prob.camera_index[sel].astype(np.int32), prob.point_index[sel].astype(np.int32),
                             np.ascontiguousarray(prob.observations[sel]), prob.parameters.copy())
        cam_mask, pt_mask = csc.bal_masks(base)
        out.update(model=sc.BalModel(sub, loss=c.get("loss"), cam_mask=cam_mask, pt_mask=pt_mask), cost=dr.bal_cost(sub, c.get("loss")))
    elif k == "quaternion":     # both blocks are in every residual block
        out.update(model=m, cost=cost(name))
    else:
        sub = sc.BlocksModel(m.sizes, [blk for blk in m.blocks if b in blk[2]])
        out.update(model=sub, cost=dr.blocks_cost(sub))
    return out


# ---- the device side -------------------------------------------------------------------------------------------------------------
def build_device(name):
    """The case as a skeres_amd problem: (problem, params DoubleArray, number of parameters, things to keep alive)."""
    base = CASES[name]["base"]
    if base is None:
        problem, _, params, keep = _own(name).build()
        return problem, params, len(_own(name).x), keep
    problem, params, n, keep = csc.build_device(base)
    if "perturb" in CASES[name]:
        params.copyFrom(x0(name))
    return problem, params, n, keep


@functools.lru_cache(maxsize=None)
def problem_order(name):
    """Per block of the case its index in the device problem's own order (first mention): the tie-break of the greedy visit."""
    problem, params, _, keep = build_device(name)
    order = [problem.parameterBlockIndex(params.slice(int(o))) for o in block_offsets(name)]
    assert sorted(order) == list(range(len(order)))
    return tuple(order)


def caller_groups(name):
    """The caller's ordering of a case as {group id: blocks}, or None."""
    if CASES[name].get("ordering") == "points":
        C = csc.bal_problem("bal-small").num_cameras
        return {3: list(range(C, len(column_blocks(name))))}
    return None


@functools.lru_cache(maxsize=None)
def groups(name):
    """The reference's groups of the case: a tuple of tuples of moving blocks."""
    m = model(name)
    given = caller_groups(name)
    if given is not None:
        moving = lambda b: any(m.free[c] for c in range(column_blocks(name)[b][0], sum(column_blocks(name)[b])))
        return tuple(tuple(b for b in given[g] if moving(b)) for g in sorted(given))
    return tuple(tuple(g) for g in ir.ordering(m, x0(name), column_blocks(name), problem_order(name)))


def device_options(name, inner=True, schur=None, **override):
    import skeres_amd as sk
    c = CASES[name]
    base = c["base"] if c["base"] is not None else "chain"      # (cgnr_schur_cases' entry without options of its own)
    o = csc.device_options(base, c.get("schur", False) if schur is None else schur, max_num_iterations=c["kmax"], **override)
    if inner is not None:
        o.setUseInnerIterations(inner)
    if "tolerance" in c:
        o.setInnerIterationTolerance(c["tolerance"])
    return o


def set_caller_ordering(name, o, params):
    """Hands the case's ordering to the options (the points of bal-small as group 3)."""
    given = caller_groups(name)
    if given is not None:
        offs = block_offsets(name)
        o.setInnerIterationOrdering({g: [params.slice(int(offs[b])) for b in blks] for g, blks in given.items()})


# ---- the references --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, defect=None, trace=False, **override):
    """(x, log[, trace]) of the reference on case `name`; shared by the tests, not to be modified."""
    c = CASES[name]
    o = options(name)
    o.update(override)
    tr = [] if trace else None
    x, log = ir.solve(model(name), cost(name), x0(name), o, dtype=LD if long_double else np.float64, blocks=column_blocks(name),
                      order=problem_order(name), schur=c.get("schur", False), groups=[list(g) for g in groups(name)],
                      local_of=lambda b: local(name, b), inner_iteration_tolerance=c.get("tolerance", ir.INNER_ITERATION_TOLERANCE),
                      defect=defect, trace=tr)
    return (x, log, tr) if trace else (x, log)


# ---- the case rule (tests/test_inner_cpu.py) -------------------------------------------------------------------------------------
# A decision compares a quantity v with a threshold t; it can only change when q = v / t crosses 1.  The difference of a decision
# between the double and the long-double reference is measured on q: |q_double - q_long| / max(|q_long|, 1) — the relative
# difference where the quantity lies above its threshold, the absolute one (in units of the threshold) below it.  Taken relative to
# v alone the figure is meaningless: a block that has converged ends on a cost change of a few ulps of its cost, twelve orders
# below the function tolerance, and those ulps differ by a quarter between the two precisions (0.24 on bal-small) although the
# decision is nowhere near changing.
#
# The margin |q - 1| that a decision keeps is a thousand times the largest difference of a decision OF ITS KIND over all cases, since
# the device differs from double by rounding of the same order.  The kinds are the tests of the inner loop (gradient, parameter,
# function, rho) and of the outer loop (parameter, function, rho, useful, enabled).  One margin for all kinds cannot be held by any
# seed: the largest difference is a block's gradient max-norm next to its minimum (a sum of terms that cancel, 4.7e-6 on
# bal-robust, orders of magnitude above its threshold of 1e-10), which would ask for a margin of 4.7e-3, and bal-robust alone takes
# 23 000 decisions, of which the closest function-tolerance test lies 1.3e-3 from its threshold (four perturbed starts of that
# case: 5.5e-5 to 7.8e-4); that test's own difference between the precisions is 4.2e-7.  A decision of one kind changes only when a quantity of that kind
# moves, so each kind is held to its own figure.  profiles/inner_iterations_error.txt records all of them (python
# tests/inner_cases.py prints that file).
MEASURED_DECISION_DEVIATION = {"inner function": 4.160e-07, "inner gradient": 4.741e-06, "inner parameter": 3.046e-07, "inner rho": 1.933e-07,
                               "outer enabled": 1.667e-12, "outer function": 6.563e-13, "outer parameter": 4.442e-11, "outer rho": 6.993e-13, "outer useful": 1.391e-13}
DECISION_MARGIN = {dk: 1000 * v for dk, v in MEASURED_DECISION_DEVIATION.items()}


def _kind(what):
    return ("inner " + what.split()[-1]) if what.startswith("block ") else ("outer " + what)


def decisions(name):
    """{kind: (deviation, closest, where, count)}: the largest difference of a decision of that kind between the double and the
    long-double trace (on q = value / threshold, see above), the smallest margin |q - 1| of one (in either precision) and where."""
    a, b = reference(name, False, trace=True)[2], reference(name, True, trace=True)[2]
    assert [w for w, _, _ in a] == [w for w, _, _ in b], name
    out = {}
    for (what, va, ta), (_, vb, tb) in zip(a, b):
        if ta == 0 or tb == 0:      # (a threshold of zero: function_tolerance * cost at a cost of zero; no case has one)
            assert va != 0 and vb != 0, (name, what)
            continue
        qa, qb = va / ta, vb / tb
        d, c, w, n = out.get(_kind(what), (0.0, float("inf"), None, 0))
        m = min(abs(qa - 1), abs(qb - 1))
        out[_kind(what)] = (max(d, abs(qa - qb) / max(abs(qb), 1.0)), min(c, m), what if m < c else w, n + 1)
    return out


if __name__ == "__main__":
    worst = {}
    print("Decision quantities of the inner-iteration cases (tests/inner_cases.py), double against long double, reference alone.")
    print("Per case and kind of decision, each as q = value / threshold: how many, the largest |q_double - q_long| / max(|q_long|, 1),")
    print("and the smallest margin |q - 1| of one in either precision.")
    for nm in sorted(CASES):
        for dk, (d, c, w, n) in sorted(decisions(nm).items()):
            worst[dk] = max(worst.get(dk, 0.0), d)
            print("%-16s %-16s %6d decisions  difference %.3e  closest %.3e (%s)" % (nm, dk, n, d, c, w))
    print("largest difference per kind, and the margin (a thousand times that):")
    for dk in sorted(worst):
        print("    %-16s %.3e  %.3e" % (dk, worst[dk], 1000 * worst[dk]))
    print("MEASURED_DECISION_DEVIATION = {%s}" % ", ".join('"%s": %.3e' % (dk, worst[dk] * 1.001) for dk in sorted(worst)))
