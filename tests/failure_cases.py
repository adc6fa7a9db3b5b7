"""The cases of the failure-path tests (tests/test_failure_cpu.py, tests/test_gpu_failure.py), their models for
tests/failure_reference.py, their problems for the device, and the comparison of a device run with the reference.

Every case names the branches of the loop it is there to reach (`reach`: names of failure_reference.BRANCHES); the CPU test
asserts that the reference went through them, in double and in long double alike, and that no decision is borderline (margins()).

What the device returns where the contract leaves it open — the evaluation after an accepted step fails (case e): the accepted
candidate is written back (as oracle/lm.cpp:634-636) and final_cost is the cost of the last point whose evaluation succeeded
(SolverBase keeps cost_ until an evaluation has come back finite; with host-callback blocks the failure is known before anything
of the new point is reduced).  The tests pin the point, the termination and the log, not that cost beyond its being finite.

Case g (a Jacobian entry that is not finite beside finite residuals at x0) is held to two levels (G_LEVEL): "exact" — immediate
FAILURE with "Initial residual and Jacobian evaluation failed.", nothing logged — where the maximum the evaluation reduces anyway
can carry the NaN (DENSE_QR / DENSE_NORMAL_CHOLESKY: dense_gmax_kernel; DENSE_SCHUR: grad_max_xnorm_kernel and the final
reductions), and "invariants" where it cannot.  Every backend is held to "exact", for a NaN entry (sqrt(u u) at u = 0, a director
block that writes one) and for an infinite one (sqrt(u) at u = 0, with Jacobi scaling — the column's scale is 1 / (1 + inf) = 0 and
its gradient entry inf * 0 — and without).

Margins.  Dense cases: a candidate meant to fail overshoots its barrier by at least 10 % of the step's length |x_new - x|, one
meant to pass clears it by as much.  DENSE_SCHUR cases: by 10 % of the barrier coordinate's own displacement — the step of a
bundle-adjustment problem whose one focal length is far off is dominated by the pose and the points of that camera moving to
compensate (|step| 40 .. 100 against a displacement of the focal coordinate of 5 .. 15), so no barrier on one coordinate can be
overshot by a tenth of the whole step; the displacement along the barrier's normal is what decides the side a candidate lands on.

Case i (linear solves that are not valid followed by valid ones, several times in one solve): its construction, and why its zero
columns are points' and none of its coordinates is inert, stands above its cases.  Its decisions are those of a quotient that rounds
to 0 or does not: exact wherever the radius was reached by powers of two and by x 3, and held 5 % away from 2^-1075 elsewhere
(tests/test_failure_cpu.py).  margins() does not apply to kind i: it measures a candidate's distance from a barrier coordinate, and
these cases have no barrier — no candidate fails; what stands in its place is the quotient's margin above and the margin of every
deciding relative decrease from min_relative_decrease, asserted in the same CPU test.

Dense rows and case f: dense_synth's rows are r_i = tanh(a_i . x / sqrt(n)) - y_i with |a_ij| < 3.5, so no Jacobian entry exceeds
3.5 / sqrt(n): the overflow of J^T J cannot be produced, and dense rows have no case f."""
import functools

import numpy as np

import skeres_amd as sk
from skeres_amd import bal, dense_synth
from skeres_amd import tape as T
from skeres_amd.examples.traced_functors import angle_axis_rotate_point

import step_check as sc
import failure_reference as fr
import dogleg_reference as dr
from dogleg_cases import TOL
from helpers import curve_fitting_data, sk_loss

LD = np.longdouble
# The radius sequence: 1e-14 relative wherever the reference's own radius is exact — the initial radius divided by powers of two (every
# invalid, failed or rejected step) and multiplied by 3 (an accepted step with rho >= 0.94).  An accepted step with a smaller rho sets
# radius / (1 - (2 rho - 1)^3): from there on the radius carries the rounding of rho = cost_change / model_cost_change, the reference's
# own double and long-double runs differ by up to 6.4e-14 there, and the tolerance is TOL_RADIUS_ROUNDED = 1e-12: sixteen times that
# spread of the reference itself (tests/test_failure_cpu.py holds the two precisions to a tenth of it).  The reference marks every
# entry (radius_exact).
TOL_RADIUS = 1e-14
TOL_RADIUS_ROUNDED = 1e-12
# x is x0 plus the accepted steps, each of them held to TOL["step_norm"] of its own length; the returned point is held to the same
# figure relative to the largest coordinate
TOL_X = TOL["step_norm"]
G_LEVEL = {"DENSE_QR": "exact", "DENSE_NORMAL_CHOLESKY": "exact", "DENSE_SCHUR": "exact"}
BAL_SHAPE, BAL_SEED = (6, 40, 200), 1
BIG = 1e160
BARRIER_CAMERA = 3


# ---------------------------------------------------------------------------------------------------------------------------
# functors: recorded (device) and the same arithmetic as host callbacks
# ---------------------------------------------------------------------------------------------------------------------------
class LogFit(sk.TracedCostFunctor):
    """r = a t + log(b) - y: the Gauss-Newton step from b = 5 towards b = 1/2 lands at b = -6.6."""

    def __init__(self, t=0.0, y=0.0):
        super().__init__(1, 1, 1, captured=(t, y))

    def apply(self, a, b):
        t, y = self.captured_values()
        return [a[0] * t + T.log(b[0]) - y]


class AbsFit(sk.TracedCostFunctor):
    """r = a t + sqrt(b b) - y: at b = 0 the residual is finite and d/db sqrt(b b) = 0 / 0."""

    def __init__(self, t=0.0, y=0.0):
        super().__init__(1, 1, 1, captured=(t, y))

    def apply(self, a, b):
        t, y = self.captured_values()
        return [a[0] * t + T.sqrt(b[0] * b[0]) - y]


class SqrtFit(sk.TracedCostFunctor):
    """r = a t + sqrt(b) - y: at b = 0 the residual is finite and d/db sqrt(b) = +inf (the Jacobi scale of that column is 1 / (1 + inf) = 0)."""

    def __init__(self, t=0.0, y=0.0):
        super().__init__(1, 1, 1, captured=(t, y))

    def apply(self, a, b):
        t, y = self.captured_values()
        return [a[0] * t + T.sqrt(b[0]) - y]


class Stiff(sk.TracedCostFunctor):
    """r = ka (xa - ca) + kb (xb - cb).  ka = 1, kb = 1e160 at xa = ca, xb = cb: a zero residual whose 2 x 2 block of J^T J
    is [[1, 1e160], [1e160, inf]] — the second pivot of its Cholesky factorisation is inf - inf."""

    def __init__(self):
        super().__init__(1, 1, 1, captured=(0.0, 0.0, 0.0, 0.0))

    def apply(self, xa, xb):
        ka, ca, kb, cb = self.captured_values()
        return [ka * (xa[0] - ca) + kb * (xb[0] - cb)]


class LogFocalSnavely(sk.TracedCostFunctor):
    """Snavely's reprojection error whose focal length is sel * camera[6] + F (1 + log(camera[6])): sel = 1, F = 0 is the plain
    camera; sel = 0 a camera whose seventh parameter is 1 at the focal length F and must stay positive."""

    def __init__(self, captured=(0.0, 0.0, 1.0, 0.0)):
        super().__init__(2, 9, 3, captured=captured)

    def focal(self, camera, sel, F):
        return sel * camera[6] + F * (1.0 + T.log(camera[6]))

    def apply(self, camera, point):
        ox, oy, sel, F = self.captured_values()
        p = angle_axis_rotate_point(camera[0:3], point)
        p = [p[0] + camera[3], p[1] + camera[4], p[2] + camera[5]]
        xp, yp = (-p[0]) / p[2], (-p[1]) / p[2]
        r2 = xp * xp + yp * yp
        fd = self.focal(camera, sel, F) * (1.0 + r2 * (camera[7] + camera[8] * r2))
        return [fd * xp - ox, fd * yp - oy]


class AbsFocalSnavely(LogFocalSnavely):
    """... whose focal length is sel * camera[6] + F sqrt(camera[7] camera[7]): finite at camera[7] = 0, its derivative 0 / 0."""

    def focal(self, camera, sel, F):
        return sel * camera[6] + F * T.sqrt(camera[7] * camera[7])


class SqrtFocalSnavely(LogFocalSnavely):
    """... whose focal length is sel * camera[6] + F sqrt(camera[7] + sel): 0 at camera[7] = 0 for sel = 0, its derivative +inf (a plain
    camera, sel = 1 and F = 0, takes the root of 1 + k1)."""

    def focal(self, camera, sel, F):
        return sel * camera[6] + F * T.sqrt(camera[7] + sel)


class StiffSnavely(LogFocalSnavely):
    """... plus, in the first residual, sel (camera[3] - c3) + F (camera[4] - c4) with c3, c4 this functor's literals: the camera's
    9 x 9 block of J^T J gets [[1, F], [F, F^2]] in its translation rows (sel = 1, F = 1e160: an inf - inf pivot)."""

    def __init__(self, c3, c4):
        self.c3, self.c4 = float(c3), float(c4)
        super().__init__(captured=(0.0, 0.0, 0.0, 0.0))

    def apply(self, camera, point):
        ox, oy, sel, F = self.captured_values()
        p = angle_axis_rotate_point(camera[0:3], point)
        p = [p[0] + camera[3], p[1] + camera[4], p[2] + camera[5]]
        xp, yp = (-p[0]) / p[2], (-p[1]) / p[2]
        r2 = xp * xp + yp * yp
        fd = camera[6] * (1.0 + r2 * (camera[7] + camera[8] * r2))
        return [fd * xp - ox + sel * (camera[3] - self.c3) + F * (camera[4] - self.c4), fd * yp - oy]


def _logfit_host(t, y, fail=None):
    """LogFit as a host callback f(params, jac) -> (ok, r, [J]); fail(a, b, jac) -> True where the block reports failure."""
    def f(p, jac):
        a, b = float(p[0][0]), float(p[1][0])
        ok = fail is None or not fail(a, b, jac)
        with np.errstate(all="ignore"):
            return ok, [a * t + np.log(b) - y], [np.array([[t]]), np.array([[1.0 / b]])]
    return f


def _exponential_host(xv, yv):
    """EX/CurveFitting.scala:92-98 as a host callback."""
    def f(p, jac):
        with np.errstate(all="ignore"):
            e = np.exp(float(p[0][0]) * xv + float(p[1][0]))
        return True, [yv - e], [np.array([[-xv * e]]), np.array([[-e]])]
    return f


class _FirstCallFails:
    """A block that reports failure on its first call and never again (fresh per run)."""

    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, p, jac):
        self.calls += 1
        ok, r, J = self.f(p, jac)
        return ok and self.calls != 1, r, J


def _nan_jacobian_at(f, b0):
    """f, but at b == b0 the Jacobian with respect to b is NaN (the residual stays what it is)."""
    def g(p, jac):
        ok, r, J = f(p, jac)
        if ok and float(p[1][0]) == b0:
            J = [J[0], np.full_like(J[1], np.nan)]
        return ok, r, J
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# the problems
# ---------------------------------------------------------------------------------------------------------------------------
def _logfit_data():
    rng = np.random.default_rng(3)
    t = np.linspace(0.0, 2.0, 20)
    return t, 1.5 * t + np.log(0.5) + 0.05 * rng.normal(size=20)


def _stiff_problem(n):
    """n scalar unknowns; blocks over the pairs (j, j + 1 mod n) with ka = kb = 1 and a residual of 1, and one stiff block over
    (n - 2, n - 1): the inf - inf pivot is the LAST one (n = 129: index 128, the first row of the second 128-block)."""
    x0 = np.linspace(-1.0, 1.0, n)
    offs = [[j, (j + 1) % n] for j in range(n)] + [[n - 2, n - 1]]
    cap = [[1.0, x0[a] - 0.5, 1.0, x0[b] - 0.5] for a, b in offs[:-1]] + [[1.0, x0[n - 2], BIG, x0[n - 1]]]
    return x0, np.array(offs, dtype=np.int64), np.array(cap)


@functools.lru_cache(maxsize=None)
def _bal(shape=BAL_SHAPE, seed=BAL_SEED, perturb=(1e-4, 1e-3, 1e-3), revisits=()):
    return bal.generate(*shape, seed=seed, perturb=perturb, revisits=list(revisits))


def _bal_offsets(prob):
    return np.stack([9 * prob.camera_index.astype(np.int64), 9 * prob.num_cameras + 3 * prob.point_index.astype(np.int64)], axis=1)


def _bal_kind(prob):
    kind = np.zeros(prob.num_parameters, dtype=np.int8)
    kind[9 * prob.num_cameras:] = 1
    return kind


U = 9 * BARRIER_CAMERA + 6   # the barrier coordinate of the DENSE_SCHUR cases: the seventh parameter of camera 3


def _log_focal_problem(prob, start):
    """x0 and the captured doubles of LogFocalSnavely: camera 3 through the logarithm, its seventh parameter started at `start`
    (1 is its focal length as generated); None: every camera plain."""
    x0 = prob.parameters.copy()
    special = (prob.camera_index == BARRIER_CAMERA) if start is not None else np.zeros(prob.num_observations, dtype=bool)
    cap = np.concatenate([prob.observations, np.where(special, 0.0, 1.0)[:, None], np.where(special, x0[U], 0.0)[:, None]], axis=1)
    if start is not None:
        x0[U] = start
    return x0, cap


HELD_CAMERAS = (0, 1)   # the gauge, as tests/dogleg_cases.py holds it


def _held_columns():
    return [9 * c + k for c in HELD_CAMERAS for k in range(9)]


# name: kind (the issue's letter), backend, what the reference must reach, options, and how to build model / device problem
CASES = {}


def _case(name, **kw):
    CASES[name] = dict(kw, name=name)


for _solver in ("DENSE_QR", "DENSE_NORMAL_CHOLESKY"):
    for _bad in ("nan", "inf"):
        _case("a-%s-%s" % (_solver, _bad), kind="a", backend=_solver, family="curve", bad=_bad, reach={"initial-evaluation-failed"})
    _case("c-%s" % _solver, kind="c", backend=_solver, family="logfit", host=False, x0=(1.0, 5.0), options=dict(initial_trust_region_radius=10.0),
          reach={"candidate-failed", "accepted"}, barrier=(1, 0.0), failed_candidates=2, converges=True)
    _case("f-%s-n3" % _solver, kind="f", backend=_solver, family="stiff", n=3, options=dict(jacobi_scaling=False),
          reach={"invalid-step", "too-many-invalid-steps"})
for _bad in ("nan", "inf"):
    _case("a-DENSE_SCHUR-%s" % _bad, kind="a", backend="DENSE_SCHUR", family="bal", bad=_bad, reach={"initial-evaluation-failed"})
    _case("a-rows-%s" % _bad, kind="a", backend="ROWS", family="rows", bad=_bad,
          reach={"initial-evaluation-failed"} if _bad == "nan" else set())   # (tanh(inf) = 1 and its derivative 0: the evaluation SUCCEEDS, the gradient is zero)
_case("b-DENSE_QR", kind="b", backend="DENSE_QR", family="curve-host", reach={"initial-evaluation-failed"})
_case("b-DENSE_SCHUR", kind="b", backend="DENSE_SCHUR", family="bal-host-first-call", reach={"initial-evaluation-failed"})
# (One DENSE_SCHUR case, the replay option left on: a recorded functor, like a director block, switches the hipGraph replay of the
# iteration off in BalSolver::setup whatever the option says, and the compiled Snavely functor has no barrier.  Invalid solves inside a
# replayed graph: case i-graph below.  OPEN: no failed CANDIDATE runs inside a replayed graph, so the zeroing of the failure flag after one,
# inside the captured sequence, is not exercised by any test.)
_case("c-DENSE_SCHUR", kind="c", backend="DENSE_SCHUR", family="log-focal", start=8.0, replay=True,
          reach={"candidate-failed", "accepted"}, barrier=(U, 0.0), failed_candidates=4, converges=True)
_case("d-DENSE_QR", kind="d", backend="DENSE_QR", family="logfit", host=True, x0=(1.0, 5.0), options=dict(initial_trust_region_radius=10.0),
      fail_beyond=0.0, reach={"candidate-failed", "accepted"}, barrier=(1, 0.0), failed_candidates=2, converges=True)
_case("d-DENSE_SCHUR", kind="d", backend="DENSE_SCHUR", family="log-focal-host", start=8.0, fail_beyond=0.0,
      reach={"candidate-failed", "accepted"}, barrier=(U, 0.0), failed_candidates=4, converges=True)
_case("e-DENSE_QR", kind="e", backend="DENSE_QR", family="logfit", host=True, x0=(1.0, 2.0), options=dict(initial_trust_region_radius=0.1),
      reach={"accepted", "evaluation-after-accept-failed"}, barrier=(1, None))
_case("e-DENSE_SCHUR", kind="e", backend="DENSE_SCHUR", family="log-focal-host", start=0.5,
      reach={"accepted", "evaluation-after-accept-failed"}, barrier=(U, None))
_case("f-DENSE_QR-n3-two-invalid", kind="f", backend="DENSE_QR", family="stiff", n=3, options=dict(jacobi_scaling=False, max_num_consecutive_invalid_steps=2),
      reach={"invalid-step", "too-many-invalid-steps"})
_case("f-DENSE_NORMAL_CHOLESKY-n129", kind="f", backend="DENSE_NORMAL_CHOLESKY", family="stiff", n=129, options=dict(jacobi_scaling=False),
      reach={"invalid-step", "too-many-invalid-steps"})
_case("f-DENSE_SCHUR", kind="f", backend="DENSE_SCHUR", family="stiff-snavely", options=dict(jacobi_scaling=False), resident=False,
      reach={"invalid-step", "too-many-invalid-steps"})
_case("f-DENSE_SCHUR-two-invalid", kind="f", backend="DENSE_SCHUR", family="stiff-snavely", resident=False,
      options=dict(jacobi_scaling=False, max_num_consecutive_invalid_steps=2), reach={"invalid-step", "too-many-invalid-steps"})
for _solver in ("DENSE_QR", "DENSE_SCHUR"):
    _case("g-%s-recorded" % _solver, kind="g", backend=_solver, family="abs-fit" if _solver == "DENSE_QR" else "abs-focal", reach={"initial-evaluation-failed"})
    # the issue's own example, d/du sqrt(u) at u = 0: +inf, not NaN — under Jacobi scaling the column's scale is 1 / (1 + inf) = 0
    _case("g-%s-recorded-inf" % _solver, kind="g", backend=_solver, family="sqrt-fit" if _solver == "DENSE_QR" else "sqrt-focal", reach={"initial-evaluation-failed"})
    _case("g-%s-recorded-inf-unscaled" % _solver, kind="g", backend=_solver, family="sqrt-fit" if _solver == "DENSE_QR" else "sqrt-focal",
          options=dict(jacobi_scaling=False), reach={"initial-evaluation-failed"})
    _case("g-%s-host" % _solver, kind="g", backend=_solver, family="logfit-nan-jacobian" if _solver == "DENSE_QR" else "bal-host-nan-jacobian",
          reach={"initial-evaluation-failed"})
# case h: the barrier of case c on (150, 3000, 14000) under the two forced plans of tests/test_gpu_step_check.py
H_SHAPE, H_SEED = (150, 3000, 14000), 5
for _plan, _knobs in (("retained", {"setRetainedPoints": ("on", 3)}), ("dissected", {"setCholeskyDissection": "on"})):
    _case("h-%s" % _plan, kind="h", backend="DENSE_SCHUR", family="log-focal", start=12.0, shape=H_SHAPE, seed=H_SEED, knobs=_knobs,
          options=dict(max_num_iterations=8), reach={"candidate-failed", "accepted"}, barrier=(U, 0.0), failed_candidates=4, reference_of="h-retained")


# case i: linear solves that are not valid FOLLOWED by valid ones, several times, on every plan of the reduced system.  Only the
# radius changes between an invalid solve and the next (x stays), so validity must hang on the radius alone, and without any rounding
# that device and reference could do differently: a FREE column of the Jacobian that is exactly zero has the LM diagonal
# min_lm_diagonal / radius, and with min_lm_diagonal = 2^-1075 R* (R* a power of two) that quotient rounds to 0 in IEEE double exactly
# where radius >= R* — a zero pivot — and to a positive subnormal below.  Ceres does the same with such a column; no held coordinate
# and no parameterization takes part.
#   The zero column is a POINT's, never a camera's: bal_point_block_kernel factors its 3 x 3 block with sqrt and /, correctly rounded
# down to the subnormals, where wave_potrf32 takes __builtin_amdgcn_rcp of the pivot, which overflows for a subnormal one — a camera
# column with a subnormal diagonal is never valid on the device (open list).  So every camera column of these
# problems is non-zero, and none of their coordinates is inert (held, padded or constant).
#   The silent co-axial component (_with_silent_component): cameras A and B with zero angle-axis on the z axis, k1 = k2 = 0, focal
# lengths 512 and 1024, A at the origin, B at t_z = -4.  ON_AXIS points are seen by A and B alone at observation (0, 0): their
# z-column is exactly 0 (the derivative along the axis vanishes) and so are their residuals.  OFF_AXIS points are seen by A and B
# alone too, with coordinates that make every operation of the projection exact, so their residuals are exactly 0 as well; they keep
# the cameras' t_z, f, k1 and k2 columns non-zero.  The component's gradient is exactly 0: it never moves, the zero columns persist
# through every accepted step, and the episodes recur whenever the radius has grown past R* again.  max_trust_region_radius = 2^16
# keeps the component's gauge directions damped far above rounding.  ("once": the two cameras also see generic points, so they move
# with the first accepted step and the one episode is that of iteration 1.)
R_STAR = 2.0 ** 12
I_MIN_LM_DIAGONAL = 2.0 ** (12 - 1075)
I_OPTIONS = dict(min_lm_diagonal=I_MIN_LM_DIAGONAL, initial_trust_region_radius=4 * R_STAR, max_trust_region_radius=2.0 ** 16)
ON_AXIS = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -4.0], [0.0, 0.0, -8.0]])
OFF_AXIS = np.array([[1.0, 2.0, -4.0], [-2.0, 1.0, -4.0], [2.0, -1.0, -4.0], [-1.0, -3.0, -4.0], [3.0, 1.0, -4.0]])
SILENT_CAMERAS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 512.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, -4.0, 1024.0, 0.0, 0.0]])


def _with_silent_component(prob, place, generic=0):
    """prob with the silent component appended: its two cameras in the middle of the camera list ("middle") or behind it ("end"), its
    points behind the points.  generic > 0: that many of prob's points seen by exactly two cameras have those two observations moved
    to A and B, as A and B project the point as it stands (the variant with one episode).  Returns (problem, dict(cameras, on_axis,
    off_axis: indices in the new problem))."""
    C, P = prob.num_cameras, prob.num_points
    a = C // 2 if place == "middle" else C
    cam = np.where(prob.camera_index >= a, prob.camera_index + 2, prob.camera_index).astype(np.int32)
    pt, obs = prob.point_index.copy(), prob.observations.copy()
    pts = np.concatenate([prob.points(), ON_AXIS, OFF_AXIS])
    if generic:
        count = np.bincount(prob.point_index, minlength=P)
        moved = 0
        for q in np.flatnonzero(count == 2):
            # (a point of the slab in front of both cameras, near the axis)
            o = np.flatnonzero(prob.point_index == q)
            pts[q] = [0.25 * (moved + 1), -0.125 * (moved + 1), -6.0 - moved]
            proj, depth = bal.snavely_project(SILENT_CAMERAS, np.stack([pts[q], pts[q]]))
            assert (depth < 0).all()
            cam[o] = [a, a + 1]
            obs[o] = proj + 0.25 * np.array([[1.0, -1.0], [-1.0, 1.0]])
            moved += 1
            if moved == generic:
                break
        assert moved == generic
    extra = np.concatenate([ON_AXIS, OFF_AXIS])
    proj, depth = bal.snavely_project(np.repeat(SILENT_CAMERAS, len(extra), axis=0), np.tile(extra, (2, 1)))
    assert (depth < 0).all()
    cam = np.concatenate([cam, np.repeat([a, a + 1], len(extra)).astype(np.int32)])
    pt = np.concatenate([pt, np.tile(P + np.arange(len(extra)), 2).astype(np.int32)])
    obs = np.concatenate([obs, proj])
    cams = np.concatenate([prob.cameras()[:a], SILENT_CAMERAS, prob.cameras()[a:]])
    out = bal.BalProblem(C + 2, P + len(extra), cam, pt, np.ascontiguousarray(obs), np.concatenate([cams.ravel(), pts.ravel()]))
    return out, dict(cameras=(a, a + 1), on_axis=tuple(range(P, P + len(ON_AXIS))), off_axis=tuple(range(P + len(ON_AXIS), P + len(extra))))


I_SHAPE, I_SEED = H_SHAPE, H_SEED
I_REACH = {"invalid-step", "accepted"}


def _case_i(name, reference_of=None, **kw):
    kw.setdefault("shape", I_SHAPE)
    kw.setdefault("seed", I_SEED)
    kw.setdefault("place", "middle")
    kw.setdefault("perturb", (1e-2, 1e-1, 1e-1))
    kw.setdefault("kmax", 9)
    kw.setdefault("episodes", 3)
    kw["options"] = dict(I_OPTIONS, max_num_iterations=kw["kmax"], **kw.get("options", {}))
    _case(name, kind="i", backend="DENSE_SCHUR", family="silent", reach=I_REACH, reference_options=dict(zero_columns_in_ieee_double=True),
          reference_of=reference_of or name, **kw)


_case_i("i-resident", knobs={"setGraphReplay": False}, plan=dict(cholesky_columns_resident=("gt", 0)))
_case_i("i-launch-by-launch", reference_of="i-resident", knobs={"setGraphReplay": False}, resident=False, plan=dict(cholesky_columns_resident=("eq", 0)))
_case_i("i-dissected", reference_of="i-resident", knobs={"setCholeskyDissection": "on", "setGraphReplay": False}, plan=dict(dissected=("eq", 1)))
_case_i("i-retained", reference_of="i-resident", knobs={"setRetainedPoints": ("on", 3), "setGraphReplay": False}, plan=dict(retained_points=("eq", 3)))
_case_i("i-huber", loss=("huber", 1.0), knobs={"setGraphReplay": False}, plan=dict(cholesky_columns_resident=("gt", 0)))
_case_i("i-graph", shape=(49, 7776, 31843), seed=49, place="end", replay=True, plan=dict(graph_replay=("eq", 1)))
# (the revisiting shape of tests/test_gpu_step_check.py::test_border_of_loop_closure_cameras_steps, its knobs; kmax = 8 holds the three
# episodes and the accepted step behind the last — the reference of this one takes 14 s in double and 75 s in long double)
_case_i("i-border", shape=(600, 6000, 26000), seed=9, revisits=((60, 350, 12, 40), (200, 520, 12, 40)), kmax=8,
        knobs={"setCholeskyBorder": "on", "setRetainedPoints": "off", "setGraphReplay": False}, plan=dict(border_cameras=("gt", 0), retained_points=("eq", 0)))
# (once the two cameras have moved, the on-axis points' depth is a nearly undetermined direction and what follows the first accepted step
# is rejected: one rejected step is kept, whose rho = -0.29 is far from any threshold and leaves the radius in the exact sequence)
_case_i("i-once", shape=(6, 40, 110), seed=BAL_SEED, perturb=(1e-4, 1e-3, 1e-3), place="end", generic=4, episodes=1, kmax=4, knobs={"setGraphReplay": False})


def names(kind=None, backend=None):
    return sorted(n for n, c in CASES.items() if (kind is None or c["kind"] in kind) and (backend is None or c["backend"] == backend))


def _bad_value(c):
    return np.nan if c["bad"] == "nan" else np.inf


def _e_threshold(name):
    """Case e: (the threshold the second accepted point crosses, half-way between the first and the second accepted point's barrier
    coordinate; +1 / -1: the side of it on which Jacobians can be evaluated), found with the reference on the problem without the
    failing block, in double."""
    c = CASES[name]
    plain = dict(c, fail_with_jacobians_beyond=(0.0, 0.0))
    run = fr.solve(_model(plain), start(name), options(name), schur=schur(name))
    acc = [e for e in run["log"][1:] if e["step_is_successful"]]
    j = c["barrier"][0]
    x1, x2 = acc[0]["candidate"][j], acc[1]["candidate"][j]
    return 0.5 * (x1 + x2), float(np.sign(x1 - x2))


@functools.lru_cache(maxsize=None)
def barrier(name):
    """(coordinate, value, side): the candidate can be evaluated where side * (x[coordinate] - value) > 0."""
    c = CASES[name]
    if c["kind"] == "e":
        return (c["barrier"][0],) + _e_threshold(name)
    return c["barrier"][0], c["barrier"][1], 1.0


def _beyond(c, name):
    """Case e's predicate on the barrier coordinate: past the threshold."""
    given = c.get("fail_with_jacobians_beyond")
    _, thr, side = (None,) + given if given is not None else barrier(name)
    return lambda v: side * (v - thr) < 0


def _prob(c):
    if c["family"] == "silent":
        return _silent(c["shape"], c["seed"], c["perturb"], c["place"], c.get("generic", 0), c.get("revisits", ()))[0]
    return _bal(c.get("shape", BAL_SHAPE), c.get("seed", BAL_SEED))


@functools.lru_cache(maxsize=None)
def _silent(shape, seed, perturb, place, generic, revisits=()):
    return _with_silent_component(_bal(shape, seed, perturb, revisits), place, generic)


def component(name):
    """Case i: the silent component of the case's problem — cameras, on_axis and off_axis points (indices), zero_columns (the
    on-axis points' z coordinates in x) and columns (every coordinate of the component in x)."""
    c = CASES[name]
    prob, comp = _silent(c["shape"], c["seed"], c["perturb"], c["place"], c.get("generic", 0), c.get("revisits", ()))
    nc = 9 * prob.num_cameras
    cols = [9 * a + k for a in comp["cameras"] for k in range(9)] + [nc + 3 * q + k for q in comp["on_axis"] + comp["off_axis"] for k in range(3)]
    return dict(comp, zero_columns=[nc + 3 * q + 2 for q in comp["on_axis"]], columns=cols)


def start(name):
    """x0 of a case (a fresh array)."""
    c = CASES[name]
    fam = c["family"]
    if fam in ("curve", "curve-host"):
        x0 = np.zeros(2)
        if "bad" in c:
            x0[0] = _bad_value(c)
        return x0
    if fam in ("logfit", "logfit-nan-jacobian"):
        return np.array(c.get("x0", (1.0, 5.0)))
    if fam in ("abs-fit", "sqrt-fit"):
        return np.array([1.0, 0.0])
    if fam == "stiff":
        return _stiff_problem(c["n"])[0]
    if fam == "rows":
        x0 = np.zeros(3)
        x0[1] = _bad_value(c)
        return x0
    prob = _prob(c)
    if fam in ("log-focal", "log-focal-host"):
        return _log_focal_problem(prob, c["start"])[0]
    x0 = prob.parameters.copy()
    if fam == "bal":
        x0[9 * 2 + 4] = _bad_value(c)
    if fam in ("abs-focal", "sqrt-focal"):
        x0[U + 1] = 0.0
    return x0


def options(name):
    return dict(CASES[name].get("options", {}))


def schur(name):
    c = CASES[name]
    if c["backend"] != "DENSE_SCHUR":
        return None
    prob = _prob(c)
    return prob.num_cameras, prob.num_points


def host_blocks(name):
    """DENSE_SCHUR cases with director blocks: the observations evaluated on the host (every fourth)."""
    return np.arange(0, _prob(CASES[name]).num_observations, 4)


def _bal_fails(c, name):
    """failed(x, jac) of the DENSE_SCHUR cases whose host blocks report failure."""
    fam = c["family"]
    if fam == "bal-host-first-call":
        state = {"calls": 0}

        def failed(x, jac):
            state["calls"] += 1
            return state["calls"] == 1
        return failed
    if fam == "log-focal-host":
        if c["kind"] == "d":
            return lambda x, jac: bool(x[U] <= c["fail_beyond"])
        beyond = _beyond(c, name)
        return lambda x, jac: bool(jac and beyond(x[U]))
    return None


class _WithFailure(sc._Model):
    """A model whose blocks also report failure where failed(x, jac) says so."""

    def __init__(self, model, failed):
        self.model, self.failed = model, failed
        self.n, self.free, self.kind = model.n, model.free, model.kind

    def chunks(self, x):
        return self.model.chunks(x)


class _NanColumn(sc._Model):
    """A model whose Jacobian column `col` is NaN at x[col] == at (a host callback that writes one)."""

    def __init__(self, model, col, at):
        self.model, self.col, self.at = model, col, at
        self.n, self.free, self.kind = model.n, model.free, model.kind

    def chunks(self, x):
        for r, terms in self.model.chunks(x):
            if x[self.col] == self.at:
                for J, first in terms:
                    hit = (first[:, None] + np.arange(J.shape[2])) == self.col
                    J[np.broadcast_to(hit[:, None, :], J.shape)] = np.nan
            yield r, terms


def _model(c):
    fam, name = c["family"], c["name"]
    if fam in ("curve", "curve-host"):
        blocks = [_exponential_host(xv, yv) for xv, yv in curve_fitting_data()]
        if fam == "curve-host":
            blocks[0] = _FirstCallFails(blocks[0])
        return fr.CallableModel(2, [(f, [0, 1], [1, 1]) for f in blocks])
    if fam in ("logfit", "logfit-nan-jacobian"):
        t, y = _logfit_data()
        if not c.get("host", True):
            return sc.TapeModel(2, [(LogFit().tape(), (1, 1), np.stack([t, y], axis=1), np.tile([0, 1], (len(t), 1)), None)])
        fail = None
        if c["kind"] == "d":
            fail = lambda a, b, jac: b <= c["fail_beyond"]
        if c["kind"] == "e":
            beyond = _beyond(c, name)
            fail = lambda a, b, jac: jac and beyond(b)
        blocks = [_logfit_host(ti, yi, fail) for ti, yi in zip(t, y)]
        if fam == "logfit-nan-jacobian":
            blocks[5] = _nan_jacobian_at(blocks[5], start(name)[1])
        return fr.CallableModel(2, [(f, [0, 1], [1, 1]) for f in blocks])
    if fam in ("abs-fit", "sqrt-fit"):
        t, y = _logfit_data()
        return sc.TapeModel(2, [((AbsFit() if fam == "abs-fit" else SqrtFit()).tape(), (1, 1), np.stack([t, y], axis=1), np.tile([0, 1], (len(t), 1)), None)])
    if fam == "stiff":
        x0, offs, cap = _stiff_problem(c["n"])
        return sc.TapeModel(c["n"], [(Stiff().tape(), (1, 1), cap, offs, None)])
    if fam == "rows":
        consts, _ = dense_synth.generate(100, 3, seed=3)
        return sc.DenseRowsModel(consts, 3)
    prob = _prob(c)
    if fam == "silent":   # (the oracle's Jacobian in double, as the step check has it)
        return sc.BalModel(prob, loss=c.get("loss"))
    offs, kind, n = _bal_offsets(prob), _bal_kind(prob), prob.num_parameters
    plain_cap = _log_focal_problem(prob, None)[1]
    if fam in ("bal", "bal-host-first-call", "bal-host-nan-jacobian"):
        m = sc.TapeModel(n, [(LogFocalSnavely().tape(), (9, 3), plain_cap, offs, None)], kind=kind)
        if fam == "bal-host-nan-jacobian":
            return _NanColumn(m, U, start(name)[U])
        failed = _bal_fails(c, name)
        return m if failed is None else _WithFailure(m, failed)
    if fam in ("log-focal", "log-focal-host"):
        m = sc.TapeModel(n, [(LogFocalSnavely().tape(), (9, 3), _log_focal_problem(prob, c["start"])[1], offs, None)], kind=kind, held=_held_columns())
        failed = _bal_fails(c, name)
        return m if failed is None else _WithFailure(m, failed)
    if fam in ("abs-focal", "sqrt-focal"):
        x0, cap = _log_focal_problem(prob, 1.0)   # camera 3: focal length F sqrt(k1 k1) or F sqrt(k1), k1 = 0 at x0
        return sc.TapeModel(n, [((AbsFocalSnavely() if fam == "abs-focal" else SqrtFocalSnavely()).tape(), (9, 3), cap, offs, None)], kind=kind)
    if fam == "stiff-snavely":
        return sc.TapeModel(n, [_stiff_snavely_group(prob)], kind=kind)
    raise KeyError(fam)


def _stiff_snavely_group(prob):
    x0 = prob.parameters
    first = int(np.flatnonzero(prob.camera_index == BARRIER_CAMERA)[0])
    cap = np.concatenate([prob.observations, np.zeros((prob.num_observations, 2))], axis=1)
    cap[first, 2:] = (1.0, BIG)
    f = StiffSnavely(x0[9 * BARRIER_CAMERA + 3], x0[9 * BARRIER_CAMERA + 4])
    return (f.tape(), (9, 3), cap, _bal_offsets(prob), None)


def model(name):
    """A fresh model of the case (blocks that count their calls start from zero)."""
    return _model(CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False):
    """The reference's run of a case; shared by the tests, not to be modified.  (The two plans of case h are one problem.)"""
    if CASES[name].get("reference_of", name) != name:
        return reference(CASES[name]["reference_of"], long_double)
    c = CASES[name]
    cost_of = dr.bal_cost(_prob(c), c["loss"]) if c["family"] == "silent" and c.get("loss") else None   # (1/2 sum rho, the oracle's residuals in double)
    return fr.solve(model(name), start(name), dict(options(name), **c.get("reference_options", {})), dtype=LD if long_double else np.float64,
                    schur=schur(name), cost_of=cost_of)


def margins(name, run=None):
    """[(iteration, signed distance of the candidate's barrier coordinate from the barrier / length, failed)] of the candidates of
    a barrier case; length: |x_new - x| (dense) or the coordinate's own displacement (DENSE_SCHUR: the module's docstring).  For case
    e the barrier is the threshold, "failed" the evaluation with Jacobians at the accepted point."""
    c = CASES[name]
    run = reference(name) if run is None else run
    j, b, side = barrier(name)
    out = []
    for k, e in enumerate(run["log"][1:], 1):
        if "candidate" not in e:
            continue
        length = abs(e["candidate"][j] - e["previous"][j]) if c["backend"] == "DENSE_SCHUR" else e["step_norm"]
        out.append((k, side * (e["candidate"][j] - b) / length, bool(e["candidate_failed"])))
    if c["kind"] == "e":   # the accepted candidate whose evaluation failed is not logged: it is the run's x
        prev = [e for e in run["log"] if e["step_is_successful"]][-1]
        x_prev = prev["candidate"] if "candidate" in prev else start(name)
        length = abs(run["x"][j] - x_prev[j]) if c["backend"] == "DENSE_SCHUR" else float(np.linalg.norm(run["x"] - x_prev))
        out.append((len(run["log"]), side * (run["x"][j] - b) / length, True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _close(a, b, tol, scale=None):
    return abs(a - b) <= tol * (abs(b) if scale is None else scale)


def compare(run, ref, x0, show=None, worst=None, tol_radius_rounded=None):
    """A device run (device_run's dict) against the reference's, entry by entry; the invariants first.  worst: a dict that
    collects the largest relative deviation per field.  tol_radius_rounded: the radius tolerance on entries behind an unclamped update
    (default TOL_RADIUS_ROUNDED, what every device case is held to)."""
    x0 = np.asarray(x0, dtype=np.float64)
    tol_radius_rounded = TOL_RADIUS_ROUNDED if tol_radius_rounded is None else tol_radius_rounded
    # invariants, whatever else differs
    if ref["termination"] == fr.FAILURE:
        assert run["termination"] == fr.FAILURE, (run["termination"], run["message"])
    assert not np.any(np.isfinite(x0) & ~np.isfinite(run["x"])), "a non-finite value was written to a parameter that was finite"
    if ref["final_cost"] is not None:   # (None: the contract does not pin it)
        assert np.isfinite(run["final_cost"]), run["final_cost"]
        assert _close(run["final_cost"], ref["final_cost"], TOL["cost"]), (run["final_cost"], ref["final_cost"])
    # the discrete fields
    d, dr_ = fr.discrete(run), fr.discrete(ref)
    if show:
        print(show, d, flush=True)
    for f in dr_:
        assert d[f] == dr_[f], (f, d[f], dr_[f])
    # the log
    for k, (e, r) in enumerate(zip(run["log"], ref["log"])):
        scale_cc = max(abs(r["cost_change"]), abs(r["cost"]))
        dev = dict(trust_region_radius=abs(e["trust_region_radius"] - r["trust_region_radius"]) / abs(r["trust_region_radius"]),
                   cost=abs(e["cost"] - r["cost"]) / abs(r["cost"]), cost_change=abs(e["cost_change"] - r["cost_change"]) / scale_cc,
                   gradient_max_norm=abs(e["gradient_max_norm"] - r["gradient_max_norm"]) / max(abs(r["gradient_max_norm"]), 1e-300),
                   step_norm=abs(e["step_norm"] - r["step_norm"]) / max(abs(r["step_norm"]), 1e-300))
        if show:
            print(show, "k=%d" % k, " ".join("%s %.17g / %.17g" % (f, e[f], r[f]) for f in dev), flush=True)
        if worst is not None:
            for f, v in dev.items():
                worst[f] = max(worst.get(f, 0.0), float(v))
        assert dev["trust_region_radius"] <= (TOL_RADIUS if r.get("radius_exact", True) else tol_radius_rounded), (k, e["trust_region_radius"], r["trust_region_radius"])
        assert dev["cost"] <= TOL["cost"], (k, e["cost"], r["cost"])
        assert dev["cost_change"] <= TOL["cost"], (k, e["cost_change"], r["cost_change"])
        assert dev["gradient_max_norm"] <= TOL["gradient_max_norm"], (k, e["gradient_max_norm"], r["gradient_max_norm"])
        assert dev["step_norm"] <= TOL["step_norm"], (k, e["step_norm"], r["step_norm"])
    # the returned point: bitwise where nothing was accepted (NaN by its bits), else to TOL_X of the largest coordinate
    if ref["num_successful_steps"] == 0 and "evaluation-after-accept-failed" not in ref["reached"]:
        assert np.array_equal(bits(run["x"]), bits(x0)), "x0 was to come back untouched"
    else:
        dx = float(np.max(np.abs(run["x"] - ref["x"])) / np.max(np.abs(ref["x"])))
        if show:
            print(show, "x: max deviation / max |x| = %.3g" % dx, flush=True)
        if worst is not None:
            worst["x"] = max(worst.get("x", 0.0), dx)
        assert dx <= TOL_X, dx
    # a rejected or invalid step leaves the point where it was, bitwise
    for k in range(1, min(len(run.get("xs", [])), len(run["log"]))):
        if not run["log"][k]["step_is_successful"]:
            assert np.array_equal(bits(run["xs"][k]), bits(run["xs"][k - 1])), k


# ---------------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------------
TERMINATION = {sk.TerminationType.CONVERGENCE: fr.CONVERGENCE, sk.TerminationType.NO_CONVERGENCE: fr.NO_CONVERGENCE, sk.TerminationType.FAILURE: fr.FAILURE}


class _HostBlock(sk.SizedCostFunction):
    """A director cost function around f(params, jac) -> (ok, r, [J])."""

    def __init__(self, f, nres, *sizes):
        super().__init__(nres, *sizes)
        self.f = f

    def evaluate(self, parameters, residuals, jacobians):
        ok, r, J = self.f(parameters, jacobians is not None)
        if not ok:
            return False
        residuals[:] = r
        if jacobians is not None:
            for q, Jq in enumerate(J):
                if jacobians[q] is not None:
                    jacobians[q][:] = Jq
        return True


def _host_of_functor(functor, failed=None, nan_column=None):
    """f(params, jac) of a TracedCostFunctor's body evaluated on the host (its director path: doubles and Jets), reporting failure
    where failed(params, jac) says so, or writing NaN into column nan_column of the first block's Jacobian."""
    inner = functor.toHostAutoDiffCostFunction()
    nres, sizes = functor.kNumResiduals, functor.N

    def f(p, jac):
        if failed is not None and failed(p, jac):
            return False, None, None
        r = np.zeros(nres)
        J = [np.zeros((nres, s)) for s in sizes] if jac else None
        if not inner.evaluate([np.asarray(q, dtype=np.float64) for q in p], r, J):
            return False, None, None
        if jac and nan_column is not None:
            J[0][:, nan_column] = np.nan
        return True, r, J
    return f


def device_problem(name):
    """(problem, parameters, n, what must stay alive) of a case on the device."""
    c = CASES[name]
    fam = c["family"]
    x0 = start(name)
    params = sk.RichDoubleArray.fromArray(x0)
    problem = sk.Problem()
    keep = [params]
    trivial = sk.PredefinedLossFunctions.trivialLoss()

    def add_host(f, nres, sizes, offs):
        cf = _HostBlock(f, nres, *sizes)
        keep.append(cf)
        problem.addResidualBlock(cf, trivial, *[params.slice(int(o)) for o in offs])

    def add_traced(functor, cap, offs):
        keep.append(functor)
        problem.addResidualBlocksTraced(functor, np.ascontiguousarray(cap), None, params, np.ascontiguousarray(offs, dtype=np.int64))

    if fam == "curve":
        for xv, yv in curve_fitting_data():
            cf = sk.ExponentialResidual(xv, yv).toAutoDiffCostFunction()
            keep.append(cf)
            problem.addResidualBlock(cf, None, params, params.slice(1))
    elif fam in ("curve-host", "logfit-nan-jacobian") or (fam == "logfit" and c.get("host", True)):
        for f, offs, sizes in model(name).blocks:
            add_host(f, 1, sizes, offs)
    elif fam in ("logfit", "abs-fit", "sqrt-fit"):
        t, y = _logfit_data()
        add_traced({"logfit": LogFit, "abs-fit": AbsFit, "sqrt-fit": SqrtFit}[fam](), np.stack([t, y], axis=1), np.tile([0, 1], (len(t), 1)))
    elif fam == "stiff":
        _, offs, cap = _stiff_problem(c["n"])
        add_traced(Stiff(), cap, offs)
    elif fam == "rows":
        consts, _ = dense_synth.generate(100, 3, seed=3)
        import oracle
        problem.addDenseRows(oracle.SYNTH_TANH_ROW, consts, None, params, 3)
    else:
        prob = _prob(c)
        offs = _bal_offsets(prob)
        if fam in ("bal", "silent"):
            loss = sk_loss(c["loss"]) if c.get("loss") else trivial
            keep.append(loss)
            problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
        elif fam in ("log-focal", "abs-focal", "sqrt-focal", "stiff-snavely"):
            if fam == "stiff-snavely":
                tape, _, cap, _, _ = _stiff_snavely_group(prob)
                functor = StiffSnavely(x0[9 * BARRIER_CAMERA + 3], x0[9 * BARRIER_CAMERA + 4])
            else:
                cap = _log_focal_problem(prob, c["start"] if fam == "log-focal" else 1.0)[1]
                functor = {"log-focal": LogFocalSnavely, "abs-focal": AbsFocalSnavely, "sqrt-focal": SqrtFocalSnavely}[fam]()
            add_traced(functor, cap, offs)
        else:   # every fourth block through the director path, the others recorded
            cap = _log_focal_problem(prob, c.get("start"))[1]
            device = LogFocalSnavely()
            hosted = set(host_blocks(name).tolist())
            failed = None
            if fam == "bal-host-first-call":
                state = {"calls": 0}

                def failed(p, jac):
                    state["calls"] += 1
                    return state["calls"] == 1
            elif fam == "log-focal-host":
                ref_fail = _bal_fails(c, name)
                xfull = np.zeros(prob.num_parameters)

                def failed(p, jac):   # (a block sees its own camera: the reference's predicate on the barrier coordinate of camera 3)
                    xfull[U] = p[0][6]
                    return ref_fail(xfull, jac)
            for i in range(prob.num_observations):
                on_barrier_camera = int(prob.camera_index[i]) == BARRIER_CAMERA
                if i in hosted:
                    f = _host_of_functor(LogFocalSnavely(captured=tuple(cap[i])),
                                         failed=failed if (fam == "bal-host-first-call" or on_barrier_camera) else None,
                                         nan_column=6 if (fam == "bal-host-nan-jacobian" and on_barrier_camera) else None)
                    add_host(f, 2, (9, 3), offs[i])
                else:
                    cf = device.withCaptured(*cap[i]).toAutoDiffCostFunction()
                    keep.append(cf)
                    problem.addResidualBlock(cf, trivial, params.slice(int(offs[i, 0])), params.slice(int(offs[i, 1])))
        if fam in ("log-focal", "log-focal-host"):
            for cam in HELD_CAMERAS:
                problem.setParameterBlockConstant(params.slice(9 * cam))
    return problem, params, len(x0), keep


def device_options(name, override=None):
    """The case's options on the device; override: option values that replace the case's (the fresh-start twin of case i)."""
    c = CASES[name]
    o = sk.Solver.Options()
    o.setLinearSolverType(sk.LinearSolverType.DENSE_NORMAL_CHOLESKY if c["backend"] == "ROWS" else getattr(sk.LinearSolverType, c["backend"]))
    setters = dict(initial_trust_region_radius="setInitialTrustRegionRadius", jacobi_scaling="setJacobiScaling", max_num_iterations="setMaxNumIterations",
                   max_num_consecutive_invalid_steps="setMaxNumConsecutiveInvalidSteps", min_lm_diagonal="setMinLmDiagonal",
                   max_trust_region_radius="setMaxTrustRegionRadius")
    for k, v in dict(options(name), **(override or {})).items():
        getattr(o, setters[k])(v)
    if "replay" in c:
        o.setGraphReplay(c["replay"])
    if "resident" in c:
        o.setResidentKernels(c["resident"])
    for k, v in c.get("knobs", {}).items():
        getattr(o, k)(*v) if isinstance(v, tuple) else getattr(o, k)(v)
    return o


def device_run(name, stats=(), override=None, built=None, end_stats=()):
    """Steps a StepSolver over the case to its end; the run in the reference's shape, plus xs (x after create and after every
    step), the named stats read after create and (end_stats) those read after the last step.  built: device_problem's tuple, where
    the caller has made it."""
    problem, params, n, keep = device_problem(name) if built is None else built
    solver = sk.StepSolver(device_options(name, override), problem)
    st = {nm: solver.stat(nm) for nm in stats}
    summary = sk.Solver.Summary()
    solver.finish(summary)
    xs = [params.toArray(n)]
    steps = 0
    while not solver.step():
        solver.finish(summary)
        xs.append(params.toArray(n))
        steps += 1
        assert steps <= 200, "the solve does not return"
    solver.finish(summary)
    return dict(x=params.toArray(n), xs=xs, log=summary.iterations(), termination=TERMINATION[summary.terminationType()], message=summary.message(),
                num_successful_steps=summary.numSuccessfulSteps(), num_unsuccessful_steps=summary.numUnsuccessfulSteps(),
                final_cost=summary.finalCost(), stats=st, end_stats={nm: solver.stat(nm) for nm in end_stats}, report=summary.fullReport())
