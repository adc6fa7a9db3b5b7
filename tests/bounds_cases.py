"""The cases of the parameter-bounds tests and their reference trajectories (tests/bounds_reference.py), computed once per process.

Bundle-adjustment cases hold cameras 0 and 1 constant, as tests/dogleg_cases.py does, at the shapes the existing suites use as
their smallest: (6, 40, 200) one partial workgroup, (16, 600, 2600) the middle shape, (150, 3000, 14000) several workgroups and
the smallest size at which plans are forced.  Boxes, seeds, perturbations and the iterations compared (kmax) were chosen with the
reference alone, in double and in long double; tests/test_bounds_cpu.py asserts the conditions they were chosen under and what
every case is there to exercise.

A box is written relative to the case's own start x0 (bal.generate leaves the focal lengths at their true values and perturbs
poses and points): box(prob) -> (lo, hi) over [cameras | points]."""
import functools

import numpy as np

from skeres_amd import bal
import step_check as sc
import dogleg_reference as dr
import dogleg_cases as dc
import bounds_reference as br

LD = np.longdouble
TOL = dc.TOL
CONST_CAMS = dc.CONST_CAMS
INF = np.inf


def _empty(prob):
    n = prob.num_parameters
    return np.full(n, -INF), np.full(n, INF)


def box_wide(prob, width=1e7):
    """Finite bounds on every coordinate, far from anything the solve visits — the points x - g of the gradient test included
    (gradients reach 7e4 here)."""
    x0 = prob.parameters
    w = width * (1.0 + np.abs(x0))
    return x0 - w, x0 + w


def box_loose(prob):
    """The same a thousand times the size of every coordinate: a long step of the hard start reaches it."""
    return box_wide(prob, 1e3)


def box_infeasible_start(prob):
    """Cameras 2 and 3 (the translation's z) and points 0..4 (x): a bound halfway between the start and where the unbounded solve of
    the same reference code ends, so that the start lies outside the box and the way to the optimum inside it; a far finite bound
    on another coordinate of each of those blocks."""
    lo, hi = _empty(prob)
    x0, C = prob.parameters, prob.num_cameras
    cam_mask = np.zeros(C, dtype=np.int32)
    cam_mask[list(CONST_CAMS)] = 0x1ff
    free = sc.BalModel(prob, cam_mask=cam_mask, pt_mask=np.zeros(prob.num_points, dtype=np.int32))
    xs, _ = br.solve(free, dr.bal_cost(prob), x0, lo, hi, dict(max_num_iterations=8), schur=(C, prob.num_points))
    for j in [9 * i + 5 for i in (2, 3)] + [9 * C + 3 * q for q in range(5)]:
        mid = x0[j] + 0.5 * (xs[j] - x0[j])
        if xs[j] > x0[j]:
            lo[j] = mid
        else:
            hi[j] = mid
        lo[j + 1 if j >= 9 * C else j - 2] = x0[j + 1 if j >= 9 * C else j - 2] - 10.0
    return lo, hi


def box_intrinsics(prob, every=3, factor=0.9):
    """f <= 0.9 of its start (the true value: the unconstrained optimum lies above the bound) for a third of the cameras, k1 >= 0 for
    every free one (a constant camera with a negative k1 would make the problem infeasible)."""
    lo, hi = _empty(prob)
    x0, C = prob.parameters, prob.num_cameras
    for i in range(C):
        if i % every == 2:
            hi[9 * i + 6] = factor * x0[9 * i + 6]
        if i not in CONST_CAMS:
            lo[9 * i + 7] = 0.0
    return lo, hi


def widest_tracks(prob, k):
    """The k points seen by most cameras (ties: the lower index): the retained-points plan takes its points from these."""
    count = np.bincount(prob.point_index, minlength=prob.num_points)
    return [int(q) for q in np.argsort(-count, kind="stable")[:k]]


def box_plans(prob, factor=0.99):
    """The four widest tracks (forced to 4, the plan retains three of them) and point 7 (eliminated) inside a box of half-width 2e-3
    around their start; an active focal bound on every third camera, no bound on k1."""
    lo, hi = box_intrinsics(prob, factor=factor)
    lo[9 * np.arange(prob.num_cameras) + 7] = -INF
    x0, C = prob.parameters, prob.num_cameras
    pts = widest_tracks(prob, 4)
    assert 7 not in pts
    for q in pts + [7]:
        sl = slice(9 * C + 3 * q, 9 * C + 3 * q + 3)
        lo[sl], hi[sl] = x0[sl] - 2e-3, x0[sl] + 2e-3
    return lo, hi


def box_robust(prob):
    """Bounds on free coordinates only (the intrinsics are held by the subset, point 5 is constant): every third camera's
    translation within 0.02 of its start, points 10..19 within 0.01."""
    lo, hi = _empty(prob)
    x0, C = prob.parameters, prob.num_cameras
    for i in range(2, C, 3):
        sl = slice(9 * i + 3, 9 * i + 6)
        lo[sl], hi[sl] = x0[sl] - 0.02, x0[sl] + 0.02
    for q in range(10, 20):
        sl = slice(9 * C + 3 * q, 9 * C + 3 * q + 3)
        lo[sl], hi[sl] = x0[sl] - 0.01, x0[sl] + 0.01
    return lo, hi


CASES = {
    "small-inactive": dict(shape=(6, 40, 200), seed=1, perturb=dc.DEFAULT_PERTURB, kmax=3, box=box_wide),
    "small-infeasible-start": dict(shape=(6, 40, 200), seed=1, perturb=dc.DEFAULT_PERTURB, kmax=3, box=box_infeasible_start),
    "active-intrinsics": dict(shape=(16, 600, 2600), seed=11, perturb=dc.DEFAULT_PERTURB, kmax=2, box=box_intrinsics),
    # a hard start from a radius of 1e10: four accepted full steps, then two iterations whose full step sends the cost up by many orders
    # of magnitude; the quadratic's minimiser lies far below the contraction's lower limit and alpha = 1e-3 is accepted
    "contracting": dict(shape=(16, 600, 2600), seed=6, perturb=(0.1, 1.0, 2.0), kmax=6, box=box_loose, options=dict(initial_trust_region_radius=1e10)),
    "plans-retained": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=3, box=box_plans,
                           knobs={"setRetainedPoints": ("on", 4)}),
    "plans-jacobi-off": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=1, box=box_plans,
                             knobs={"setRetainedPoints": ("on", 4)}, options=dict(jacobi_scaling=False)),
    "robust-subset": dict(shape=(16, 600, 2600), seed=11, perturb=dc.DEFAULT_PERTURB, kmax=4, loss=("huber", 1.0), subset=True, const_pts=(5,),
                          box=box_robust),
    "tape": dict(shape=(6, 40, 200), seed=1, perturb=dc.DEFAULT_PERTURB, kmax=3, box=box_infeasible_start, tape=True),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    return bal.generate(*c["shape"], seed=c["seed"], perturb=c["perturb"])


@functools.lru_cache(maxsize=None)
def box(name):
    lo, hi = CASES[name]["box"](problem(name))
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def masks(name):
    c, prob = CASES[name], problem(name)
    cam_mask = np.full(prob.num_cameras, 0b111000000 if c.get("subset") else 0, dtype=np.int32)
    cam_mask[list(CONST_CAMS)] = 0x1ff
    pt_mask = np.zeros(prob.num_points, dtype=np.int32)
    pt_mask[list(c.get("const_pts", ()))] = 7
    return cam_mask, pt_mask


def model(name):
    cam_mask, pt_mask = masks(name)
    return sc.BalModel(problem(name), loss=CASES[name].get("loss"), cam_mask=cam_mask, pt_mask=pt_mask)


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, unbounded=False, kmax=None):
    """(x, log) of the reference on case `name`; shared by the tests, not to be modified.  unbounded: the same code with no box."""
    c, prob = CASES[name], problem(name)
    o = dict(c.get("options", {}))
    o["max_num_iterations"] = c["kmax"] if kmax is None else kmax
    lo, hi = _empty(prob) if unbounded else box(name)
    return br.solve(model(name), dr.bal_cost(prob, c.get("loss")), prob.parameters, lo, hi, o, dtype=LD if long_double else np.float64,
                    schur=(prob.num_cameras, prob.num_points))


# ---- the dense Jacobian path -----------------------------------------------------------------------------------------------
# powell: EX/Powell.scala with a box that excludes the origin (its unconstrained minimiser); curve-fitting: EX/CurveFitting.scala
# with c >= 0.3 (its optimum is c = 0.13; the start (0, 0) is infeasible); hello-world: r = 10 - x with x <= 7; dense-tangent:
# the small bundle-adjustment shape through DENSE_QR, every free camera's intrinsics held by a subset parameterization (the
# tangent-space form of the dense path), with the box of "small-infeasible-start".
DENSE_CASES = {"powell": dict(kmax=3), "curve-fitting": dict(kmax=8), "curve-fitting-overflow": dict(kmax=4), "hello-world": dict(kmax=1),
               "dense-tangent": dict(kmax=3)}


@functools.lru_cache(maxsize=None)
def dense_problem(name):
    """(block sizes, [(functor, consts, parameter blocks, loss)], x0, lo, hi, parameterizations)."""
    import oracle
    if name == "powell":
        sizes, blocks, x0 = dc.dense_problem("powell")
        return sizes, blocks, x0, np.array([0.5, -INF, -INF, 0.25]), np.array([INF, -0.1, INF, INF]), None
    if name in ("curve-fitting", "curve-fitting-overflow"):
        sizes, blocks, _ = dc.dense_problem("curve-fitting")
        x0 = np.array([1.0, 0.0]) if name == "curve-fitting" else np.array([-100.0, 0.0])
        return sizes, blocks, x0, np.array([-INF, 0.3]), np.array([INF, 2.0]), None
    if name == "hello-world":
        return [1], [(oracle.HELLO_WORLD, [], [0], None)], np.array([0.5]), np.array([-INF]), np.array([7.0]), None
    prob = problem("small-infeasible-start")
    C, P = prob.num_cameras, prob.num_points
    sizes = [9] * C + [3] * P
    blocks = [(oracle.SNAVELY, [float(prob.observations[o, 0]), float(prob.observations[o, 1])], [int(prob.camera_index[o]), C + int(prob.point_index[o])], None)
              for o in range(prob.num_observations)]
    pz = [("constant",) if i in CONST_CAMS else ("subset", [6, 7, 8]) for i in range(C)] + [None] * P
    lo, hi = box("small-infeasible-start")
    return sizes, blocks, prob.parameters, lo, hi, pz


@functools.lru_cache(maxsize=None)
def dense_model(name):
    sizes, blocks, x0, lo, hi, pz = dense_problem(name)
    return sc.BlocksModel(sizes, blocks, pz)


@functools.lru_cache(maxsize=None)
def dense_reference(name, long_double=False):
    sizes, blocks, x0, lo, hi, pz = dense_problem(name)
    m = dense_model(name)
    cost = dr.blocks_cost(m)

    def quiet_cost(x):   # (an overflowing exp is a cost that is not finite, not a warning)
        with np.errstate(all="ignore"):
            return cost(x)
    return br.solve(m, quiet_cost, x0, lo, hi, dict(max_num_iterations=DENSE_CASES[name]["kmax"]), dtype=LD if long_double else np.float64)


ALL = sorted(CASES) + sorted(DENSE_CASES)


def any_reference(name, long_double=False):
    return reference(name, long_double) if name in CASES else dense_reference(name, long_double)


def kmax_of(name):
    return (CASES[name] if name in CASES else DENSE_CASES[name])["kmax"]


def violations(name):
    """The conditions a case was chosen under, checked on the reference alone; returns what is violated (nothing: [])."""
    kmax = kmax_of(name)
    a, b = any_reference(name)[1], any_reference(name, True)[1]
    out = []
    if not (len(a) == len(b) == kmax + 1):
        return ["%d / %d logged iterations for kmax %d" % (len(a), len(b), kmax)]
    for k in range(kmax + 1):
        for f in ("step_is_valid", "step_is_successful", "step_size", "line_search_evaluations", "active_bounds"):
            if a[k][f] != b[k][f]:
                out.append("k=%d %s: %r in double, %r in long double" % (k, f, a[k][f], b[k][f]))
        if [(t[0], bool(np.isfinite(t[1]))) for t in a[k]["trials"]] != [(t[0], bool(np.isfinite(t[1]))) for t in b[k]["trials"]]:
            out.append("k=%d: the trials differ" % k)
        for f, t in TOL.items():
            if not dc.close(a[k][f], b[k][f], t / 10):
                out.append("k=%d %s: %.17g / %.17g" % (k, f, a[k][f], b[k][f]))
        for log in (a, b):
            if any(m < 1e-6 for m in log[k]["margins"]):
                out.append("k=%d: an Armijo test within %.1e of its bound" % (k, min(log[k]["margins"])))
            # An alpha that comes out of the interpolation unclamped depends on the last bits of phi: no two summation orders give
            # the same one.  The cases keep to alphas that have the same bits whatever the rounding: 1, the lower limit of the
            # contraction (the quadratic's minimiser below 0.9e-3 alpha) and the bisection after a cost that is not finite.
            if any(u > 0.9e-3 for u in log[k]["unclamped"]):
                out.append("k=%d: an interpolated alpha inside its limits (%.3g of the last one)" % (k, max(log[k]["unclamped"])))
    return out


EXACT = ("step_is_valid", "step_is_successful", "step_size", "line_search_evaluations")


def compare_logs(log, ref, kmax, tol=TOL, factor=1.0, show=None):
    """dogleg_cases.compare_logs, and exactly equal: the line search's alpha and the number of candidate costs of every iteration."""
    dc.compare_logs(log, ref, kmax, tol=tol, factor=factor, show=show)
    for k in range(kmax + 1):
        if show:
            print("%s k=%d alpha %r / %r evaluations %r / %r" % (show, k, log[k]["step_size"], ref[k]["step_size"], log[k]["line_search_evaluations"],
                                                                 ref[k]["line_search_evaluations"]), flush=True)
    for k in range(kmax + 1):
        assert log[k]["step_size"] == ref[k]["step_size"], (k, log[k]["step_size"], ref[k]["step_size"])
        assert int(log[k]["line_search_evaluations"]) == int(ref[k]["line_search_evaluations"]), k
