"""What the leaves compute, from the mathematical definitions, in mpmath / sympy at 60 digits and more: CPU only.

Nothing here is taken from csrc/ or oracle/, and nothing calls them.  A rotation is R = exp([a]x); its quaternion is
(cos(t/2), sin(t/2) a/t); the inverse maps are the principal logarithm (angle in [0, pi]); a quaternion acts on a point by
q p q*; a loss is its rho(s) alone, rho' and rho'' are sympy derivatives of that expression; Plus of a manifold is written
from its definition and its Jacobian is the derivative of that Plus.  Derivatives of the rotations and of Plus are central
differences with h = 1e-25 at 60 digits (truncation h^2 f''' / 6 ~ 1e-50 f''', rounding 1e-60 / h = 1e-35, both far below the
1e-16 they are compared at); at a point where a map is only one-sidedly smooth (angle pi, trace 0) the branch is fixed at the
point and continued smoothly around it, which is the derivative the definition has on that side.

Two things are not independent of the code or not done as one might expect.  Which of q and -q rotationMatrixToQuaternion
returns is a convention, not mathematics: matrix_sign_index takes it from the comment and code of csrc/rotation.hpp (w >= 0 where
the trace is not negative, else the component of the largest diagonal entry, the first of equals), so that choice is not checked
here, only that the quaternion returned is one of the two (R(q) = R, test_leaf_reference_cpu.py).  Functors 1 (Snavely) and 12
are differentiated by the same central differences, not by sympy: they are built on the rotation reference, which is mpmath
code, and h = 1e-25 at 60 digits leaves 1e-35.  Functors 2 to 9 and 11 are sympy expressions with sympy derivatives.

generate() returns every reference value of tests/leaf_cases.py as (hi, lo) pairs of doubles, hi + lo carrying about 32 digits;
`python tests/leaf_reference.py` writes them to tests/golden/leaf_reference.npz, the only thing the GPU test reads.

compare() is the one yardstick, used for the oracle (CPU) and the device (GPU) alike: |got - ref| <= C[family] * unit, with the
units below and the constants C measured as profiles/leaf_error.txt records."""
import os

import numpy as np

import leaf_cases as lc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_reference.npz")
U = 2.0 ** -53
TINY = 2.0 ** -1074  # one subnormal step: what a result that passes through the subnormal range may lose

# ---- the bounds --------------------------------------------------------------------------------------------------------------
# |got - ref| <= C * (u * scale + TINY); scale = the largest |ref| of the output block (rotations, functors), |x| (manifolds),
# the entry's own natural size (losses, see loss_scale).  Each C is 8 x the worst ratio of the CPU oracle over the whole case
# list, rounded up to a power of two, at least 4 (profiles/leaf_error.txt holds the ratios); the 8 is for the device's libm
# (sincos, exp, log, atan2 are a few ulp, not correctly rounded) and its fused multiply-adds.
#
# Two families have a bound of another form, both for inherited behaviour that is pinned, not fixed:
#  * Jet parts of angleAxisToRotationMatrix, angleAxisRotatePoint and Snavely's camera columns.
#    theta^2 <= ulp(1): the code returns I + [a]x, whose derivative is the constant generator.  The exact map is
#    I + A(t) [a]x + B(t) [a]x^2 with A = sin t / t = 1 - t^2/6 + ..., B = (1 - cos t) / t^2 = 1/2 - t^2/24 + ...; its derivative
#    along v differs from [v]x by B ([v]x [a]x + [a]x [v]x) + O(t^2), of norm at most 2 B t |v| <= t |v| (|[a]x| = t).  Applied to
#    a point and relative to the block's scale that is an error of at most C1 * theta * scale with C1 = 1 for |v| <= 1; the
#    seeds have |v|_inf <= 1.375 over up to 9 entries, the measured ratio decides.
#    theta^2 > ulp(1): the matrix is c I + s [w]x + (1 - c) w w^T with w = a / t.  1 - c is formed by subtraction: absolute error
#    u on a value of t^2 / 2.  In the values that is harmless (it multiplies w w^T, size 1: error u).  In the Jet parts the
#    term's derivative holds (1 - c) d(w w^T) with d(w) = O(|v| / t): u times 1 / t.  Bound: C2 * (u + u / theta) * scale.
#  * The homogeneous vector where householder_vector takes its degenerate branch on an x that is not exactly +-|x| e_n
#    (0 < sigma <= kHouseholderPole x_n^2): bound C3 * sqrt(ulp(1)) * |x|, the form the old absolute threshold was thought to
#    need.  The reference showed the branch to be an O(1) step from the exact reflection instead (I against I - 2 h h^T / |h|^2,
#    h the head of x), so the threshold went down to 2^-400 relative, where x is the pole to working precision, and no input of the
#    case list is inside the branch any more: the family is empty and its constant the minimum, 4.  Raising the threshold
#    again would put inputs back into it, where they would fail.
C = {
    "rotation_value": 64.0, "rotation_jet": 128.0, "rotation_jet_first_order": 16.0, "rotation_jet_cancel": 64.0,
    "rotation_bilinear_value": 256.0, "rotation_bilinear_jet": 256.0,
    "loss": 32.0, "loss_tolerant": 256.0, "param": 64.0, "param_degenerate": 4.0,
    "functor": 128.0, "snavely": 512.0, "snavely_jet_first_order": 8.0, "snavely_jet_cancel": 16.0,
    "corrector": 32.0,
}
SMALL_ANGLE_OPS = (lc.AA2R, lc.AAROT)


def split(v):
    """mp value(s) -> (hi, lo) doubles."""
    import mpmath as mp
    a = np.empty(np.shape(v), dtype=object)
    a[...] = v
    hi = np.array([float(x) for x in a.ravel()], dtype=np.float64)
    lo = np.array([float(mp.mpf(x) - mp.mpf(h)) if np.isfinite(h) else 0.0 for x, h in zip(a.ravel(), hi)], dtype=np.float64)
    return hi.reshape(a.shape), lo.reshape(a.shape)


def error(got, hi, lo):
    """|got - (hi + lo)| in doubles: got - hi is exact when they are close, and a large error needs no digits."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
    return np.where(np.isnan(e), np.inf, e)


def ratios(got, hi, lo, unit):
    """Error over unit, entry by entry; `unit` broadcasts against the outputs."""
    return error(got, hi, lo) / (unit + TINY)


class Tally:
    """Worst ratio per family and the number of reference values compared."""

    def __init__(self, record_only=False):
        self.worst, self.detail, self.count, self.record_only = {}, {}, 0, record_only  # record_only: measure, do not assert

    def add(self, family, r, n, what=""):
        w = float(np.max(r)) if np.size(r) else 0.0
        self.worst[family] = max(self.worst.get(family, 0.0), w)
        self.detail[(family, what)] = max(self.detail.get((family, what), 0.0), w)
        self.count += n


def compare(family, got, hi, lo, unit, tally=None, what=""):
    """Assert |got - ref| <= C[family] * unit everywhere; returns the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == hi.shape == lo.shape, (what, got.shape, hi.shape)
    r = ratios(got, hi, lo, unit)
    if tally is not None:
        tally.add(family, r, got.size, what)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= C[family] and not (tally is not None and tally.record_only):
        k = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError("%s %s: error %.3g = %.3g units at %r, bound %g units (got %r, ref %r)"
                             % (family, what, error(got, hi, lo)[k], worst, k, C[family], got[k], hi[k]))
    return worst


def block_scale(hi, axes):
    return np.max(np.abs(hi), axis=axes, keepdims=True)


# ---- comparing one family of outputs: shared by the CPU (oracle) and the GPU (device) tests -----------------------------------
def check_rotation(ref, op, K, got, tally=None):
    """got: [n, out(, 1 + K)] row-major.  Values against rot/<op>/v, Jet parts against rot/<op>/j<K>."""
    what = "%s K=%d" % (lc.OP_NAMES[op], K)
    vhi, vlo = ref["rot/%d/v/hi" % op], ref["rot/%d/v/lo" % op]
    val = got if K == 0 else got[:, :, 0]
    # crossProduct / dotProduct cancel: their error is relative to |x| |y|, not to the result the bound's scale is taken from
    plain = "rotation_bilinear" if op in (lc.CROSS, lc.DOT) else "rotation"
    compare(plain + "_value", val, vhi, vlo, U * block_scale(vhi, 1), tally, what)
    if K == 0:
        return
    # the seeds of width K are the first K of width 4 (leaf_cases._dyadic), so one set of Jet references serves 1, 3 and 4
    jhi, jlo = ref["rot/%d/j4/hi" % op][:, :, :K], ref["rot/%d/j4/lo" % op][:, :, :K]
    scale = block_scale(jhi, (1, 2))
    jet = got[:, :, 1:]
    if op not in SMALL_ANGLE_OPS:
        compare(plain + "_jet", jet, jhi, jlo, U * scale, tally, what)
        return
    theta = np.sqrt(np.sum(lc.rotation_inputs()[op][:, :3] ** 2, axis=1))[:, None, None]
    first = (theta * theta <= lc.ULP1)[:, 0, 0]
    with np.errstate(divide="ignore"):
        compare("rotation_jet_first_order", jet[first], jhi[first], jlo[first], (U + theta[first]) * scale[first], tally, what)
        compare("rotation_jet_cancel", jet[~first], jhi[~first], jlo[~first], (U + U / theta[~first]) * scale[~first], tally, what)


def loss_scale(s, hi):
    """rho, rho' and rho'' are each held to their own magnitude, at every s."""
    return np.abs(hi).copy()


def check_loss(ref, i, got, tally=None):
    hi, lo = ref["loss/%d/hi" % i], ref["loss/%d/lo" % i]
    # a tolerant leaf evaluates exp at x = (s - a) / b: the rounding of x, u |x|, is a relative error of e^x, |x| up to 100 here
    family = "loss_tolerant" if "tolerant" in repr(lc.LOSS_SPECS[i]) else "loss"
    spec, s = lc.LOSS_SPECS[i], lc.loss_s(lc.LOSS_SPECS[i])
    scale = loss_scale(s, hi)
    if spec[0] == "tolerant":
        # beyond x = 36.7 the code returns rho' = 1, rho'' = 0 for 1 / (1 + e^-x) and e^-x / (b (1 + e^-x)^2): it drops
        # e^-36.7 = 1.04 u of rho', and that over b of rho'', whose scale there is therefore 1 / b
        tail = (s - spec[1]) / spec[2] > 36.7
        scale[tail, 2] = np.maximum(scale[tail, 2], 1.0 / spec[2])
    compare(family, got, hi, lo, U * scale, tally, repr(spec))


def check_param(ref, key, x, plus, jac, jac_rows, tally=None, degenerate=None):
    """plus [m, n] against par/<key>/plus, jac [len(jac_rows), n, l] against par/<key>/jac; unit from |x|."""
    xn = np.sqrt(np.sum((x / np.abs(x).max(axis=1, keepdims=True)) ** 2, axis=1)) * np.abs(x).max(axis=1)
    deg = np.zeros(len(x), dtype=bool) if degenerate is None else degenerate
    for name, got, rows in (("plus", plus, np.arange(len(x))), ("jac", jac, jac_rows)):
        hi, lo = ref["par/%s/%s/hi" % (key, name)], ref["par/%s/%s/lo" % (key, name)]
        unit = xn[rows].reshape((-1,) + (1,) * (hi.ndim - 1))
        d = deg[rows]
        compare("param", got[~d], hi[~d], lo[~d], U * unit[~d], tally, "%s %s" % (key, name))
        compare("param_degenerate", got[d], hi[d], lo[d], np.sqrt(lc.ULP1) * unit[d], tally, "%s %s" % (key, name))


def check_functor(ref, fid, res, jac, tally=None):
    """res [m, nres], jac [m, nres, sum N] (None: the cost-only call)."""
    rhi, rlo = ref["fun/%d/r/hi" % fid], ref["fun/%d/r/lo" % fid]
    plain = "snavely" if fid == 1 else "functor"
    compare(plain, res, rhi, rlo, U * block_scale(rhi, 1), tally, "functor %d residuals" % fid)
    if jac is None:
        return
    jhi, jlo = ref["fun/%d/j/hi" % fid], ref["fun/%d/j/lo" % fid]
    scale = block_scale(jhi, (1, 2))
    if fid != 1:
        compare("functor", jac, jhi, jlo, U * scale, tally, "functor %d jacobian" % fid)
        return
    theta = lc.snavely_theta(lc.functor_inputs(1)[1])[:, None, None]
    first = (theta * theta <= lc.ULP1)[:, 0, 0]
    compare("snavely", jac[:, :, 3:], jhi[:, :, 3:], jlo[:, :, 3:], U * scale, tally, "Snavely, the columns past the rotation")
    cam = jac[:, :, :3]
    with np.errstate(divide="ignore"):
        compare("snavely_jet_first_order", cam[first], jhi[first][:, :, :3], jlo[first][:, :, :3], (U + theta[first]) * scale[first],
                tally, "Snavely camera rotation")
        compare("snavely_jet_cancel", cam[~first], jhi[~first][:, :, :3], jlo[~first][:, :, :3],
                (U + U / theta[~first]) * scale[~first], tally, "Snavely camera rotation")


def run_rotation(backend, ref, tally, op):
    """backend.rotation(op, array, row_major, K) -> array: both strides, doubles and every Jet width, one call each."""
    np.testing.assert_array_equal(ref["rot/%d/x" % op], lc.rotation_inputs()[op])
    for row_major in (False, True):
        for K in (0,) + lc.JET_DIMS:
            out = backend.rotation(op, lc.rotation_call(op, row_major, K), row_major, K)
            check_rotation(ref, op, K, lc.rotation_result(op, row_major, out), tally)
    return tally


def run_losses(backend, ref, tally):
    """backend.loss(spec, s) -> [n, 3]"""
    for i, spec in enumerate(lc.LOSS_SPECS):
        np.testing.assert_array_equal(ref["loss/%d/x" % i], lc.loss_s(spec))
        check_loss(ref, i, backend.loss(spec, lc.loss_s(spec)), tally)
    return tally


def run_params(backend, ref, tally):
    """backend.param(key, x, delta, jac_rows) -> (plus [m, n], jac [len(jac_rows), n, l])"""
    for key, (_, x, d, rows) in param_groups().items():
        np.testing.assert_array_equal(ref["par/%s/x" % key], np.concatenate([x, d], axis=1))
        plus, jac = backend.param(key, x, d, rows)
        check_param(ref, key, x, plus, jac, rows, tally, lc.homogeneous_degenerate(x) if key[0] == "h" else None)
    return tally


def run_functor(backend, ref, tally, fid):
    """backend.functor(fid, consts, params, want_jacobian) -> (residuals [nres], jacobian [nres, sum N] or None)"""
    c, p = lc.functor_inputs(fid)
    np.testing.assert_array_equal(ref["fun/%d/x" % fid], np.concatenate([c, p], axis=1))
    full = [backend.functor(fid, c[i], p[i], True) for i in range(len(p))]
    check_functor(ref, fid, np.array([r for r, _ in full]), np.array([j for _, j in full]), tally)
    check_functor(ref, fid, np.array([backend.functor(fid, c[i], p[i], False)[0] for i in range(len(p))]), None, tally)
    return tally


def check_corrector(r, J, rt, Jt, cost, rho, tally=None, what=""):
    """The two properties that define the Triggs corrector, in long double, on a raw (r, J) and a corrected (rt, Jt) block:
        Jt^T rt = rho' J^T r        Jt^T Jt = rho' J^T J + 2 rho'' J^T r r^T J   where the alpha branch is taken (s > 0, rho'' > 0)
                                    Jt^T Jt = rho' J^T J                          where it is not,
    and the block's cost, rho / 2.  Units: u rho' |J| |r|, u (rho' + 2 |rho''| s) |J|^2, u rho / 2.  Returns the three ratios."""
    LD = np.longdouble
    r, J, rt, Jt, rho = (np.asarray(a, dtype=np.float64).astype(LD) for a in (r, J, rt, Jt, rho))
    s = r @ r
    alpha = bool(s > 0 and rho[2] > 0)
    g, Jn = J.T @ r, np.sqrt((J * J).sum())
    want_H = rho[1] * (J.T @ J) + (2 * rho[2] * np.outer(g, g) if alpha else 0)
    ratio = np.array([np.abs(Jt.T @ rt - rho[1] * g).max() / (U * rho[1] * Jn * np.sqrt(s) + TINY),
                      np.abs(Jt.T @ Jt - want_H).max() / (U * (rho[1] + 2 * abs(rho[2]) * s) * Jn * Jn + TINY),
                      abs(LD(cost) - rho[0] / 2) / (U * rho[0] / 2 + TINY)], dtype=np.float64)
    if tally is not None:
        tally.add("corrector", ratio, 3, what)
    if not ratio.max() <= C["corrector"] and not (tally is not None and tally.record_only):
        raise AssertionError("corrector %s: gradient, Hessian, cost off by %r units, bound %g" % (what, ratio.tolist(), C["corrector"]))
    return alpha


def run_corrector(backend, tally):
    """backend.correct(spec, r, J) -> (corrected r, corrected J, cost); backend.loss(spec, s) -> [n, 3].  Returns the branches met."""
    branches = set()
    for spec, r, J in lc.corrector_inputs():
        rt, Jt, cost = backend.correct(spec, r, J)
        rho = backend.loss(spec, np.array([float(r @ r)]))[0]
        branches.add(check_corrector(r, J, rt, Jt, cost, rho, tally, "%r k=%d" % (spec, len(r))))
    return branches


def run_all(backend, ref, tally):
    """Every case of tests/leaf_cases.py through `backend` (the oracle or the device) against `ref`."""
    for op in range(14):
        run_rotation(backend, ref, tally, op)
    run_losses(backend, ref, tally)
    run_params(backend, ref, tally)
    for fid in lc.FUNCTORS:
        run_functor(backend, ref, tally, fid)
    return tally


def expected_count(ref, prefix=""):
    """How many values the run_* of the keys under `prefix` compare: each rotation value under both strides and four widths, each
    Jet part of width 4 under both strides and 8 / 4 times (widths 1, 3, 4 read its first columns), each functor residual with
    and without its Jacobian, everything else once."""
    n = 0
    for k, v in ref.items():
        if k.endswith("/hi") and k.startswith(prefix):
            n += v.size * (8 if k.startswith("rot") and "/v/" in k else 4 if k.startswith("rot") else 2 if k.startswith("fun") and "/r/" in k else 1)
    return n


def load():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


# ==============================================================================================================================
# The reference itself: mpmath / sympy from here on (imported inside the functions, the GPU machine need not have them)
# ==============================================================================================================================
DPS = 60


def _mp():
    import mpmath as mp
    mp.mp.dps = DPS
    return mp


def H():
    return _mp().mpf("1e-25")


def vec(x):
    mp = _mp()
    return [mp.mpf(float(v)) for v in x]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm(a):
    return _mp().sqrt(dot(a, a))


def qmul(z, w):
    """Hamilton product, (w, x, y, z) = scalar first."""
    zv, wv = z[1:], w[1:]
    c = cross(zv, wv)
    return [z[0] * w[0] - dot(zv, wv)] + [z[0] * wv[i] + w[0] * zv[i] + c[i] for i in range(3)]


def qconj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def exp_so3(a):
    """Rodrigues: I + sin t / t [a]x + (1 - cos t) / t^2 [a]x^2, rows of a 3 x 3 list; 1 - cos t as 2 sin^2(t/2)."""
    mp = _mp()
    t = norm(a)
    A = mp.sin(t) / t if t != 0 else mp.mpf(1)
    B = 2 * (mp.sin(t / 2) / t) ** 2 if t != 0 else mp.mpf(1) / 2
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    K2 = [[dot(K[i], [K[0][j], K[1][j], K[2][j]]) for j in range(3)] for i in range(3)]
    return [[(1 if i == j else 0) + A * K[i][j] + B * K2[i][j] for j in range(3)] for i in range(3)]


def quaternion_of_angle_axis(a):
    mp = _mp()
    t = norm(a)
    k = mp.sin(t / 2) / t if t != 0 else mp.mpf(1) / 2
    return [mp.cos(t / 2)] + [k * x for x in a]


def log_quaternion(q, w_negative):
    """Angle-axis of q / |q| with the angle in [0, pi]: for w < 0 it is -q that has the short angle.  `w_negative` is decided at
    the point; around it the same expression continues smoothly."""
    mp = _mp()
    sgn = -1 if w_negative else 1
    n = norm(q[1:])
    if n == 0:
        return [mp.mpf(0)] * 3
    k = 2 * mp.atan2(sgn * n, sgn * q[0]) / n
    return [k * x for x in q[1:]]


def quaternion_of_matrix(R, positive):
    """The unit quaternion q with R(q) = R and q[positive] > 0.  Each q_i^2 is a combination of the diagonal, the products
    q_i q_j are combinations of the off-diagonal pairs; divide by the largest q_i."""
    mp = _mp()
    tr = R[0][0] + R[1][1] + R[2][2]
    sq = [(1 + tr) / 4] + [(1 + 2 * R[i][i] - tr) / 4 for i in range(3)]
    p = max(range(4), key=lambda i: sq[i])
    qp = mp.sqrt(sq[p])
    prod = {(0, 1): (R[2][1] - R[1][2]) / 4, (0, 2): (R[0][2] - R[2][0]) / 4, (0, 3): (R[1][0] - R[0][1]) / 4,
            (1, 2): (R[0][1] + R[1][0]) / 4, (1, 3): (R[0][2] + R[2][0]) / 4, (2, 3): (R[1][2] + R[2][1]) / 4}
    q = [qp if i == p else prod[(min(i, p), max(i, p))] / qp for i in range(4)]
    return [-x for x in q] if q[positive] < 0 else q


def matrix_sign_index(R):
    """Which component the quaternion of R has positive: w where the trace is not negative, else the one of the largest diagonal
    entry (the first of equals), the convention csrc/rotation.hpp documents."""
    if R[0][0] + R[1][1] + R[2][2] >= 0:
        return 0
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    return i + 1


def scaled_rotation(q):
    """Columns q e_j q*: |q|^2 times the rotation of q."""
    cols = [qmul(qmul(q, [0] + [1 if i == j else 0 for i in range(3)]), qconj(q))[1:] for j in range(3)]
    return [[cols[j][i] for j in range(3)] for i in range(3)]


def euler_matrix(e):
    """(pitch, roll, yaw) in degrees about x, y, z: R = Rz(yaw) Ry(roll) Rx(pitch)."""
    mp = _mp()
    p, r, y = [v * mp.pi / 180 for v in e]
    Rx = [[1, 0, 0], [0, mp.cos(p), -mp.sin(p)], [0, mp.sin(p), mp.cos(p)]]
    Ry = [[mp.cos(r), 0, mp.sin(r)], [0, 1, 0], [-mp.sin(r), 0, mp.cos(r)]]
    Rz = [[mp.cos(y), -mp.sin(y), 0], [mp.sin(y), mp.cos(y), 0], [0, 0, 1]]
    mm = lambda A, B: [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return mm(Rz, mm(Ry, Rx))


def flat(R):
    return [R[i][j] for i in range(3) for j in range(3)]


def unflat(x):
    return [list(x[0:3]), list(x[3:6]), list(x[6:9])]


def matvec(R, p):
    return [dot(R[i], p) for i in range(3)]


def rotation_function(op, x0):
    """The map of operation `op` around the input x0 (mp list, matrices row-major): x -> outputs (matrices row-major)."""
    if op == lc.AA2Q:
        return quaternion_of_angle_axis
    if op == lc.Q2AA:
        neg = x0[0] < 0
        return lambda q: log_quaternion(q, neg)
    if op in (lc.R2Q, lc.R2AA):
        pos = matrix_sign_index(unflat(x0))
        if op == lc.R2Q:
            return lambda x: quaternion_of_matrix(unflat(x), pos)
        neg = quaternion_of_matrix(unflat(x0), pos)[0] < 0
        return lambda x: log_quaternion(quaternion_of_matrix(unflat(x), pos), neg)
    if op == lc.AA2R:
        return lambda a: flat(exp_so3(a))
    if op == lc.EULER2R:
        return lambda e: flat(euler_matrix(e))
    if op == lc.Q2SR:
        return lambda q: flat(scaled_rotation(q))
    if op == lc.Q2R:
        return lambda q: [v / dot(q, q) for v in flat(scaled_rotation(q))]
    if op == lc.UQROT:
        return lambda x: qmul(qmul(x[:4], [0] + list(x[4:])), qconj(x[:4]))[1:]
    if op == lc.QROT:
        return lambda x: [v / dot(x[:4], x[:4]) for v in qmul(qmul(x[:4], [0] + list(x[4:])), qconj(x[:4]))[1:]]
    if op == lc.QPROD:
        return lambda x: qmul(x[:4], x[4:])
    if op == lc.CROSS:
        return lambda x: cross(x[:3], x[3:])
    if op == lc.DOT:
        return lambda x: [dot(x[:3], x[3:])]
    if op == lc.AAROT:
        return lambda x: matvec(exp_so3(x[:3]), x[3:])
    raise ValueError(op)


def directional(f, x, v):
    """J v by central differences."""
    h = H()
    a = f([xi + h * vi for xi, vi in zip(x, v)])
    b = f([xi - h * vi for xi, vi in zip(x, v)])
    return [(p - q) / (2 * h) for p, q in zip(a, b)]


def rotation_reference(op):
    """values [n, out], {K: derivative parts [n, out, K]} as object arrays of mpf."""
    xs = lc.rotation_inputs()[op]
    n, m = len(xs), lc.OUT_LEN[op]
    vals = np.empty((n, m), dtype=object)
    widest = max(lc.JET_DIMS)
    jets = {widest: np.empty((n, m, widest), dtype=object)}
    seeds = {widest: lc.rotation_seeds(op, widest)}
    for K in lc.JET_DIMS:
        np.testing.assert_array_equal(lc.rotation_seeds(op, K), seeds[widest][:, :, :K])
    for i in range(n):
        x = vec(xs[i])
        f = rotation_function(op, x)
        vals[i, :] = f(x)
        for k in range(widest):
            jets[widest][i, :, k] = directional(f, x, vec(seeds[widest][i, :, k]))
    return vals, jets


# ---- losses: rho(s) only; the derivatives are sympy's -------------------------------------------------------------------------
LOSS_DPS = 1200  # whatever cancels in the defining expressions and in sympy's derivatives of them leaves noise below 1e-1100: under
# the smallest subnormal where the value itself is, and 800 digits behind it where it is a double


def _rho_expr(spec, s, s_val, sp, mp):
    """(expression in the symbol s, its value at s_val).  A piecewise loss contributes the piece its argument lies in; the
    threshold is the squared scale as a double, the parameter the loss is built with."""
    if spec is None:
        return s, s_val
    kind = spec[0]
    if kind == "composed":
        g, gv = _rho_expr(spec[2], s, s_val, sp, mp)
        t = sp.Symbol("t%d" % id(spec))
        f, fv = _rho_expr(spec[1], t, gv, sp, mp)
        return f.subs(t, g), fv
    if kind == "scaled":
        f, fv = _rho_expr(spec[1], s, s_val, sp, mp)
        k = sp.Rational(*float(spec[2]).as_integer_ratio())
        return k * f, mp.mpf(float(spec[2])) * fv
    a = sp.Rational(*float(spec[1]).as_integer_ratio())
    b2 = sp.Rational(*float(spec[1] * spec[1]).as_integer_ratio())  # a^2 as the double the loss holds
    inside = s_val <= mp.mpf(float(spec[1] * spec[1]))
    if kind == "huber":
        e = s if inside else 2 * sp.sqrt(b2) * sp.sqrt(s) - b2
    elif kind == "softlone":
        e = 2 * a * a * (sp.sqrt(1 + s / (a * a)) - 1)
    elif kind == "cauchy":
        e = a * a * sp.log(1 + s / (a * a))
    elif kind == "tukey":
        e = b2 / 6 * (1 - (1 - s / b2) ** 3) if inside else b2 / 6 + 0 * s
    elif kind == "tolerant":
        b = sp.Rational(*float(spec[2]).as_integer_ratio())
        e = b * sp.log(1 + sp.exp((s - a) / b)) - b * sp.log(1 + sp.exp(-a / b))
    else:
        raise ValueError(kind)
    return e, sp.lambdify(s, e, "mpmath")(s_val)


def loss_reference(spec, s_values):
    """[len(s), 3] object array of (rho, rho', rho'') as mpf."""
    import mpmath as mp
    import sympy as sp
    out = np.empty((len(s_values), 3), dtype=object)
    old = mp.mp.dps
    mp.mp.dps = LOSS_DPS
    try:
        s = sp.Symbol("s", positive=True)
        for i, sv in enumerate(s_values):
            svm = sv if isinstance(sv, mp.mpf) else mp.mpf(float(sv))
            e, _ = _rho_expr(spec, s, svm, sp, mp)
            for d in range(3):
                out[i, d] = mp.mpf(sp.lambdify(s, sp.diff(e, s, d), "mpmath")(svm))
    finally:
        mp.mp.dps = old
    return out


# ---- manifolds ----------------------------------------------------------------------------------------------------------------
def quaternion_plus(x, d):
    """exp(delta) (x) x, exp(delta) = (cos |d|, sin |d| d / |d|)."""
    mp = _mp()
    n = norm(d)
    k = mp.sin(n) / n if n != 0 else mp.mpf(1)
    return qmul([mp.cos(n)] + [k * v for v in d], x)


def homogeneous_plus(x, d):
    """|x| H(x) [1/2 sinc(|d|/2) d ; cos(|d|/2)], H the reflection that takes x to |x| e_n (the identity when x is there)."""
    mp = _mp()
    n = len(x)
    nd = norm(d)
    k = mp.sin(nd / 2) / nd if nd != 0 else mp.mpf(1) / 2
    y = [k * v for v in d] + [mp.cos(nd / 2)]
    xn = norm(x)
    w = list(x)
    w[n - 1] = w[n - 1] - xn
    ww = dot(w, w)
    if ww == 0:
        return [xn * v for v in y]
    c = 2 * dot(w, y) / ww
    return [xn * (y[i] - c * w[i]) for i in range(n)]


def subset_plus(const):
    def plus(x, d):
        d = list(d)
        return [xi if i in const else xi + d.pop(0) for i, xi in enumerate(x)]
    return plus


def plus_jacobian(plus, x, local):
    mp = _mp()
    cols = []
    for c in range(local):
        e = [mp.mpf(1 if i == c else 0) for i in range(local)]
        cols.append(directional(lambda d: plus(x, d), [mp.mpf(0)] * local, e))
    return [[cols[c][r] for c in range(local)] for r in range(len(x))]


def param_reference(plus, xs, ds, jac_rows):
    local = ds.shape[1]
    P = np.empty(xs.shape, dtype=object)
    J = np.empty((len(jac_rows), xs.shape[1], local), dtype=object)
    for i in range(len(xs)):
        P[i, :] = plus(vec(xs[i]), vec(ds[i]))
    for k, i in enumerate(jac_rows):
        J[k, :, :] = plus_jacobian(plus, vec(xs[i]), local)
    return P, J


def param_groups():
    """key -> (plus, x, delta, rows whose Jacobian is kept: one per distinct x)."""
    g = {}
    step = len(lc.DELTA_NORMS)
    for n in lc.HOMOGENEOUS_SIZES:
        x, d = lc.homogeneous_inputs(n)
        g["h%d" % n] = (homogeneous_plus, x, d, np.arange(0, len(x), step))
    x, d = lc.quaternion_inputs()
    g["q"] = (quaternion_plus, x, d, np.arange(0, len(x), step))
    for size, const in lc.SUBSETS:
        x, d = lc.subset_inputs(size, const)
        g["s%d_%s" % (size, "".join(map(str, const)))] = (subset_plus(const), x, d, np.arange(len(x)))
    return g


# ---- functors: sympy expressions of the reference project's examples and specs ------------------------------------------------
def functor_expressions(fid, c, p):
    """Residuals of functor `fid` in the sympy symbols c (constants) and p (all parameter blocks, concatenated)."""
    import sympy as sp
    if fid == 2:    # EX/CurveFitting.scala:92-98: y - exp(m x + c)
        return [c[1] - sp.exp(p[0] * c[0] + p[1])]
    if fid == 3:    # EX/Powell.scala:14-21: x1 + 10 x2
        return [p[0] + 10 * p[1]]
    if fid == 4:    # EX/Powell.scala:24-31: sqrt(5) x3 - x4, as the reference writes it
        return [sp.sqrt(5) * p[0] - p[1]]
    if fid == 5:    # EX/Powell.scala:34-42: (x2 - 2 x3)^2
        return [(p[0] - 2 * p[1]) ** 2]
    if fid == 6:    # EX/Powell.scala:45-53: sqrt(10) (x1 - x4)^2
        return [sp.sqrt(10) * (p[0] - p[1]) ** 2]
    if fid == 7:    # TEST/AutodiffCostFuntionSpec.scala:14-26: x . y - a
        return [p[0] * p[2] + p[1] * p[3] - c[0]]
    if fid == 8:    # TEST/AutodiffCostFuntionSpec.scala:55-69
        x, y = p[:2], p[2:]
        return [x[0] * y[0] + x[1] * y[1] - c[0], x[0] * y[0] - x[1] * y[1] + c[0], x[0] * x[1] + y[0] * y[1] + 10 * c[0]]
    if fid == 9:    # TEST/AutodiffCostFuntionSpec.scala:111-119: the sum of ten scalars
        return [sum(p)]
    if fid == 11:   # EX/HelloWorld.scala:11-14: 10 - x
        return [10 - p[0]]
    raise ValueError(fid)


def snavely(c, x):
    """EX/SimpleBundleAdjuster.scala:79-119: P = R(a) X + t, p = -P / P.z, r = f (1 + k1 |p|^2 + k2 |p|^4) p - observed."""
    P = [u + t for u, t in zip(matvec(exp_so3(x[0:3]), x[9:12]), x[3:6])]
    xp, yp = -P[0] / P[2], -P[1] / P[2]
    r2 = xp * xp + yp * yp
    f = x[6] * (1 + x[7] * r2 + x[8] * r2 * r2)
    return [f * xp - c[0], f * yp - c[1]]


def quaternion_rotation_error(c, x):
    """Functor 12: R(q / |q|) p - t with c = (p, t)."""
    rot = qmul(qmul(x, [0] + list(c[:3])), qconj(x))[1:]
    return [v / dot(x, x) - t for v, t in zip(rot, c[3:])]


def functor_reference(fid):
    """residuals [m, nres], Jacobian [m, nres, sum N] as mpf."""
    import sympy as sp
    mp = _mp()
    nres, sizes, nc = lc.FUNCTORS[fid]
    cs, ps = lc.functor_inputs(fid)
    npar = sum(sizes)
    R = np.empty((len(ps), nres), dtype=object)
    J = np.empty((len(ps), nres, npar), dtype=object)
    if fid in (1, 12):
        fn = snavely if fid == 1 else quaternion_rotation_error
        for i in range(len(ps)):
            c, x = vec(cs[i]), vec(ps[i])
            R[i, :] = fn(c, x)
            for j in range(npar):
                J[i, :, j] = directional(lambda y: fn(c, y), x, [mp.mpf(1 if k == j else 0) for k in range(npar)])
        return R, J
    c = sp.symbols("c0:%d" % max(nc, 1))
    p = sp.symbols("p0:%d" % npar)
    exprs = functor_expressions(fid, c, p)
    fr = sp.lambdify([c, p], exprs, "mpmath")
    fj = sp.lambdify([c, p], [[sp.diff(e, v) for v in p] for e in exprs], "mpmath")
    for i in range(len(ps)):
        cv, pv = vec(cs[i]) if nc else [mp.mpf(0)], vec(ps[i])
        R[i, :] = [mp.mpf(v) for v in fr(cv, pv)]
        J[i, :, :] = [[mp.mpf(v) for v in row] for row in fj(cv, pv)]
    return R, J


# ---- everything ---------------------------------------------------------------------------------------------------------------
def generate(only=None):
    """name -> float64 array: every input (`.../x`) and every reference value (`.../hi`, `.../lo`)."""
    out = {}

    def put(key, obj):
        out[key + "/hi"], out[key + "/lo"] = split(obj)

    for op in range(14):
        if only and "rot" not in only:
            break
        vals, jets = rotation_reference(op)
        out["rot/%d/x" % op] = np.array(lc.rotation_inputs()[op])
        put("rot/%d/v" % op, vals)
        for K in jets:
            put("rot/%d/j%d" % (op, K), jets[K])
    for i, spec in enumerate(lc.LOSS_SPECS):
        if only and "loss" not in only:
            break
        out["loss/%d/x" % i] = lc.loss_s(spec)
        put("loss/%d" % i, loss_reference(spec, lc.loss_s(spec)))
    for key, (plus, x, d, rows) in param_groups().items():
        if only and "par" not in only:
            break
        out["par/%s/x" % key] = np.concatenate([x, d], axis=1)
        P, J = param_reference(plus, x, d, rows)
        put("par/%s/plus" % key, P)
        put("par/%s/jac" % key, J)
    for fid in lc.FUNCTORS:
        if only and "fun" not in only:
            break
        c, p = lc.functor_inputs(fid)
        out["fun/%d/x" % fid] = np.concatenate([c, p], axis=1)
        R, J = functor_reference(fid)
        put("fun/%d/r" % fid, R)
        put("fun/%d/j" % fid, J)
    return out


def count_values(ref):
    return sum(v.size for k, v in ref.items() if k.endswith("/hi"))


def measure(which):
    """The lines of profiles/leaf_error.txt for `which` = "oracle" or "device": worst ratio and constant per family, and for the
    oracle how far compare() rejects each planted defect and the figures at the inputs where the two defects were first seen."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if which == "oracle":
        from test_leaf_reference_cpu import OracleBackend as Backend, planted_defects
    else:
        from test_gpu_leaf import DeviceBackend as Backend
    ref = load()
    tally = run_all(Backend(), ref, Tally(record_only=True))
    run_corrector(Backend(), tally)
    lines = ["%s: %d values compared" % (which, tally.count), "%-28s %12s %8s" % ("family", "worst ratio", "c")]
    lines += ["%-28s %12.3g %8g" % (k, v, C[k]) for k, v in sorted(tally.worst.items())]
    lines += ["  %-26s %-70s %10.3g" % (f, w, v) for (f, w), v in sorted(tally.detail.items()) if v > C[f] / 16]
    if which == "oracle":
        import oracle
        lines.append("planted defects: times its bound by which compare() rejects each")
        lines += ["  %-48s %10.3g" % kv for kv in planted_defects(ref).items()]
        lines.append("rho at small s, relative error against the reference")
        for spec, sv in ((("softlone", 0.7), 1e-12), (("cauchy", 0.5), 1e-12), (("tukey", 2.0), 1e-12), (("tolerant", 1.5, 0.4), 1e-12),
                         (("tolerant", 40.0, 1.0), 1e-12), (("tolerant", 1.0, 0.01), 0.05)):
            want = loss_reference(spec, [sv])[0, 0]
            lines.append("  %-26r s=%-6g %.3g" % (spec, sv, float(abs(oracle.loss_evaluate(spec, sv)[0] - want) / want)))
        x, d = 1e-9 * np.ones(4), np.array([1e-30, 0.0, 0.0])
        hv = ("homogeneous",)
        lines.append("x = 1e-9 (1, 1, 1, 1): |Plus(x, 1e-30) - x| / |x| = %.3g, max |x^T J| / |x|^2 = %.3g"
                     % (np.linalg.norm(oracle.parameterization_plus(hv, x, d) - x) / np.linalg.norm(x),
                        np.abs(x @ oracle.parameterization_jacobian(hv, x)).max() / (x @ x)))
    return "\n".join(lines)


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:  # python tests/leaf_reference.py oracle | device: what profiles/leaf_error.txt records
        print(measure(sys.argv[1]))
        sys.exit(0)
    np.savez_compressed(FIXTURE, **generate())
    print("wrote %s: %d bytes, %d reference values" % (FIXTURE, os.path.getsize(FIXTURE), count_values(load())))
