"""The inputs at which the leaves (csrc/rotation.hpp, loss.hpp, parameterization.hpp, functors.hpp) are held to
tests/leaf_reference.py: numpy only, deterministic, built once per process.  Every input listed here has a reference value in
tests/golden/leaf_reference.npz and is compared; the one input without a value is the zero quaternion of
quaternionToRotation, which must raise (ZERO_QUATERNION_RAISES).

The edges are the ones the code branches on or loses digits at: theta^2 against 0 and ulp(1) (1.4e-8 / 1.6e-8 straddle
sqrt(ulp(1)) = 1.49e-8), theta at and next to pi, squared vector parts that are subnormal or underflow, quaternions with w <= 0,
rotation matrices on each branch of the trace / largest-diagonal selection, s at 0, at the piece boundaries and far out, homogeneous
vectors at and next to +-|x| e_n at three scales."""
import numpy as np

U = 2.0 ** -53
ULP1 = 2.0 ** -52
HOUSEHOLDER_POLE = 2.0 ** -400  # csrc/parameterization.hpp kHouseholderPole
ZERO_QUATERNION_RAISES = np.zeros((1, 4))  # quaternionToRotation: no reference value, must raise

(AA2Q, Q2AA, R2Q, R2AA, AA2R, EULER2R, Q2SR, Q2R, UQROT, QROT, QPROD, CROSS, DOT, AAROT) = range(14)
OP_NAMES = ("angleAxisToQuaternion", "quaternionToAngleAxis", "rotationMatrixToQuaternion", "rotationMatrixToAngleAxis",
            "angleAxisToRotationMatrix", "eulerAnglesToRotationMatrix", "quaternionToScaledRotation", "quaternionToRotation",
            "unitQuaternionRotatePoint", "quaternionRotatePoint", "quaternionProduct", "crossProduct", "dotProduct",
            "angleAxisRotatePoint")
IN_LEN = (3, 4, 9, 9, 3, 3, 4, 4, 7, 7, 8, 6, 6, 6)
OUT_LEN = (4, 3, 4, 3, 9, 9, 9, 9, 3, 3, 4, 3, 1, 3)
MATRIX_IN, MATRIX_OUT = (R2Q, R2AA), (AA2R, EULER2R, Q2SR, Q2R)
JET_DIMS = (1, 3, 4)

THETAS = (0.0, 1e-200, 1e-160, 1e-12, 1.4e-8, 1.6e-8, 1e-6, 1e-3, 1.0, 3.0, np.pi - 1e-6, np.pi - 1e-10, np.pi, 4.0, 6.2)


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _skew(a):
    K = np.zeros(a.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -a[..., 2], a[..., 1], a[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -a[..., 0], -a[..., 1], a[..., 0]
    return K


def _qmul(z, w):
    return np.stack([z[..., 0] * w[..., 0] - z[..., 1] * w[..., 1] - z[..., 2] * w[..., 2] - z[..., 3] * w[..., 3],
                     z[..., 0] * w[..., 1] + z[..., 1] * w[..., 0] + z[..., 2] * w[..., 3] - z[..., 3] * w[..., 2],
                     z[..., 0] * w[..., 2] - z[..., 1] * w[..., 3] + z[..., 2] * w[..., 0] + z[..., 3] * w[..., 1],
                     z[..., 0] * w[..., 3] + z[..., 1] * w[..., 2] - z[..., 2] * w[..., 1] + z[..., 3] * w[..., 0]], axis=-1)


def _angle_axes(rng):
    """39 angle-axis vectors: every theta of THETAS about two random axes, and 1.4e-8, 1, pi about the coordinate axes."""
    out = []
    for t in THETAS:
        for _ in range(2):
            out.append(t * _unit(rng.normal(size=3)))
    for t in (1.4e-8, 1.0, np.pi):
        out.extend(t * np.eye(3))
    return np.array(out)


def _quaternion_of(aa):
    """Some double quaternion near the rotation aa: an input, so how well it is rounded does not matter."""
    t = np.sqrt(np.sum(aa * aa, axis=-1, keepdims=True))
    k = np.where(t > 0, np.sin(0.5 * t) / np.where(t > 0, t, 1.0), 0.5)
    return np.concatenate([np.cos(0.5 * t), k * aa], axis=-1)


def _matrix_of(aa):
    """Some double matrix near exp([aa]x), [n, 3, 3]."""
    t = np.sqrt(np.sum(aa * aa, axis=-1))[:, None, None]
    K = _skew(aa)
    safe = np.where(t > 1e-4, t, 1.0)
    a = np.where(t > 1e-4, np.sin(safe) / safe, 1.0 - t * t / 6.0)
    b = np.where(t > 1e-4, (1.0 - np.cos(safe)) / (safe * safe), 0.5 - t * t / 24.0)
    return np.eye(3) + a * K + b * (K @ K)


def _unit_quaternions(rng):
    """w > 0, w < 0, w = 0, vector parts whose square is subnormal (1e-160) or underflows (1e-170), the identity."""
    aa = _angle_axes(rng)
    q = _quaternion_of(aa[::2][:15])                      # one per theta
    neg = -q[[2, 5, 7, 8, 9, 10, 11, 13]]                 # the same rotations with w < 0
    w0 = np.concatenate([np.zeros((4, 1)), np.concatenate([np.eye(3), _unit(rng.normal(size=(1, 3)))])], axis=1)
    tiny = []
    for m in (1e-160, 1e-170):
        for w in (1.0, -1.0):
            tiny.append(np.concatenate([[w], m * _unit(rng.normal(size=3))]))
    return np.concatenate([q, neg, w0, np.array(tiny), [[1.0, 0, 0, 0], [-1.0, 0, 0, 0]]])


def _matrices(rng):
    aa = [t * _unit(rng.normal(size=3)) for t in THETAS[3:] for _ in range(2)]         # 1e-12 .. 6.2
    for tr in (1e-9, -1e-9, 1e-3, -1e-3):                                              # trace = 1 + 2 cos(theta) next to 0
        aa.append(np.arccos(0.5 * (tr - 1.0)) * _unit(rng.normal(size=3)))
    for lead in range(3):                                                              # trace < 0, each largest diagonal entry
        for t in (3.0, np.pi - 1e-6):
            ax = 0.2 * rng.normal(size=3)
            ax[lead] = 1.0
            aa.append(t * _unit(ax))
    R = list(_matrix_of(np.array(aa)))
    R += [np.diag(d) for d in ([1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1], [1.0, 1, 1])]  # angle pi exactly about x, y, z; the identity
    for _ in range(2):                                                                  # angle pi about a random axis: 2 a a^T - I
        ax = _unit(rng.normal(size=3))
        R.append(2.0 * np.outer(ax, ax) - np.eye(3))
    return np.array(R).reshape(-1, 9)                                                   # row-major: x[3 i + j] = R(i, j)


def _eulers(rng):
    e = [[0, 0, 0], [90, 0, 0], [0, 90, 0], [0, 0, 90], [-90, 0, 0], [0, -90, 0], [0, 0, -90], [180, 0, 0], [0, 180, 0], [0, 0, 180],
         [360, 0, 0], [0, 360, 0], [0, 0, 360], [90, 90, 90], [-90, 90, 180], [180, -90, 360], [360, 180, -90], [90, 45, -30]]
    return np.concatenate([np.array(e, dtype=np.float64), rng.uniform(-180, 180, (20, 3)), rng.uniform(-1e-6, 1e-6, (2, 3))])


_ROT = None


def rotation_inputs():
    """op -> [n, IN_LEN[op]] doubles; matrices row-major (to_layout() gives the column-major call its order)."""
    global _ROT
    if _ROT is not None:
        return _ROT
    rng = np.random.default_rng(20240501)
    aa, uq, R = _angle_axes(rng), _unit_quaternions(rng), _matrices(rng)
    scaled = np.concatenate([uq[:33] * s for s in (1e-3, 1.0, 1e3)])[::2]              # |q| in {1e-3, 1, 1e3}
    pts = lambda n: rng.normal(size=(n, 3)) * rng.choice([1e-3, 1.0, 50.0], size=(n, 1))
    vec = np.concatenate([rng.normal(size=(30, 6)), np.concatenate([np.eye(3), np.roll(np.eye(3), 1, axis=0)], axis=1),
                          rng.normal(size=(6, 6)) * rng.choice([1e-8, 1e8], size=(6, 1))])
    _ROT = {AA2Q: aa, Q2AA: uq, R2Q: R, R2AA: R, AA2R: aa, EULER2R: _eulers(rng), Q2SR: scaled, Q2R: scaled,
            UQROT: np.concatenate([uq, pts(len(uq))], axis=1), QROT: np.concatenate([scaled, pts(len(scaled))], axis=1),
            QPROD: np.concatenate([scaled[:len(uq)], uq[::-1]], axis=1), CROSS: vec, DOT: vec,
            AAROT: np.concatenate([aa, pts(len(aa))], axis=1)}
    for op, x in _ROT.items():
        assert x.shape[1] == IN_LEN[op] and 30 <= len(x) <= 50, (op, x.shape)
        x.setflags(write=False)
    return _ROT


def _dyadic(n, m, K, salt):
    """Infinitesimal parts without a random generator: multiples of 1/4 in [-1.25, 1.25], no zero column."""
    i, e, k = np.ogrid[:n, :m, :K]
    return (((7 * i + 3 * e + 5 * k + (i * e) % 3 + salt) % 11) - 5) / 4.0 + 0.125 * (e == k)


def rotation_seeds(op, K):
    """[n, IN_LEN, K] infinitesimal parts.  A rotation matrix and the unit quaternion of unitQuaternionRotatePoint are moved along
    their manifold ([w]x R, 1/2 (0, w) q): off it the operation has no definition, only whatever the formula happens to extend to."""
    x = rotation_inputs()[op]
    n = len(x)
    v = _dyadic(n, IN_LEN[op], K, op)
    if op in MATRIX_IN:
        w = _dyadic(n, 3, K, op)
        R = x.reshape(n, 3, 3)
        v = np.stack([(_skew(w[:, :, k]) @ R).reshape(n, 9) for k in range(K)], axis=2)
    if op == UQROT:
        w = _dyadic(n, 3, K, op)
        for k in range(K):
            v[:, :4, k] = 0.5 * _qmul(np.concatenate([np.zeros((n, 1)), w[:, :, k]], axis=1), x[:, :4])
    return v


def to_layout(a, row_major):
    """[n, 9, ...] held row-major -> the order a call with `row_major` reads or writes (its own inverse)."""
    if row_major:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a.reshape((len(a), 3, 3) + a.shape[2:]).swapaxes(1, 2).reshape(a.shape))


def rotation_call(op, row_major, K):
    """The array one rotation `apply(op, ., row_major, K)` call takes."""
    x = rotation_inputs()[op]
    a = x if K == 0 else np.concatenate([x[:, :, None], rotation_seeds(op, K)], axis=2)
    return to_layout(a, row_major) if op in MATRIX_IN else np.ascontiguousarray(a)


def rotation_result(op, row_major, out):
    """A call's output, matrices brought back to row-major."""
    return to_layout(out, row_major) if op in MATRIX_OUT else out


# ---- losses ------------------------------------------------------------------------------------------------------------------
LOSS_SPECS = [("huber", 1.3), ("softlone", 0.7), ("cauchy", 0.5), ("tukey", 2.0), ("tolerant", 1.5, 0.4),
              ("scaled", ("cauchy", 0.8), 2.5), ("scaled", None, 0.25), ("composed", ("huber", 1.1), ("softlone", 0.9)),
              ("composed", ("scaled", ("cauchy", 1.0), 3.0), ("tolerant", 0.7, 0.2)),
              ("tolerant", 40.0, 1.0), ("tolerant", 1.0, 0.01), ("huber", 1e-3), ("cauchy", 1e3),
              ("scaled", ("composed", ("cauchy", 0.8), ("scaled", ("composed", ("huber", 1.1), ("softlone", 0.9)), 0.5)), 2.0)]
LOSS_S = (0.0, 1e-300, 1e-30, 1e-12, 1e-6, 0.05, 1.0, 60.0, 1e6, 1e12, 1e300)


def loss_s(spec):
    s = list(LOSS_S)
    if spec[0] in ("huber", "tukey"):
        b = spec[1] * spec[1]  # the threshold as the code forms it
        s += [b * (1.0 - ULP1), b, b * (1.0 + ULP1)]
    if spec[0] == "tolerant":
        s += [spec[1] + spec[2] * (36.7 - 1e-9), spec[1] + spec[2] * (36.7 + 1e-9)]
    return np.array(s)


# ---- local parameterizations -------------------------------------------------------------------------------------------------
HOMOGENEOUS_SIZES = (2, 3, 4, 16)
SUBSETS = ((5, (0,)), (5, (4,)), (5, (0, 3)), (4, (0, 1, 2)), (4, (1, 2, 3)), (3, ()))
DELTA_NORMS = (0.0, 1e-30, 1e-8, 1e-2, 1.0, np.pi, 2.0 * np.pi)
_PAR = {}


def _deltas(rng, n, m):
    d = np.stack([DELTA_NORMS[i % len(DELTA_NORMS)] * _unit(rng.normal(size=m)) for i in range(n)])
    return d


def homogeneous_inputs(n):
    """(x [m, n], delta [m, n - 1]): each shape of x at scales 1, 1e-9, 1e9, each with every delta norm."""
    if n not in _PAR:
        rng = np.random.default_rng(7000 + n)
        e = np.zeros(n)
        e[-1] = 1.0
        shapes = [rng.normal(size=n), rng.normal(size=n), 2.5 * e, -0.5 * e]
        for eps in (1e-9, 1.4e-8, 1.6e-8, 1e-4):
            for piv in (1.0, -1.0):
                x = piv * e
                x[0] = eps
                shapes.append(x)
        z = rng.normal(size=n)
        z[-1] = 0.0                                     # x_pivot = 0
        shapes.append(z)
        xs = np.array([c * x for x in shapes for c in (1.0, 1e-9, 1e9)])
        xs = np.repeat(xs, len(DELTA_NORMS), axis=0)
        ds = _deltas(rng, len(xs), n - 1)
        xs.setflags(write=False)
        ds.setflags(write=False)
        _PAR[n] = (xs, ds)
    return _PAR[n]


def homogeneous_degenerate(x):
    """True where householder_vector takes its degenerate branch on a vector that is not exactly +-|x| e_n."""
    sigma = np.sum(x[:, :-1] ** 2, axis=1)
    return (sigma > 0.0) & (sigma <= HOUSEHOLDER_POLE * x[:, -1] ** 2)


def quaternion_inputs():
    if "q" not in _PAR:
        rng = np.random.default_rng(7100)
        q = _unit(rng.normal(size=(7, 4)))
        q[1::2, 0] = -np.abs(q[1::2, 0])               # w < 0
        q[::2, 0] = np.abs(q[::2, 0])
        xs = np.repeat(np.concatenate([q, 1e-3 * q, 1e3 * q, [[1.0, 0, 0, 0], [0.0, 0, 1, 0]]]), len(DELTA_NORMS), axis=0)
        ds = _deltas(rng, len(xs), 3)
        _PAR["q"] = (xs, ds)
    return _PAR["q"]


def subset_inputs(size, const):
    key = ("s", size, const)
    if key not in _PAR:
        rng = np.random.default_rng(7200 + size + 10 * len(const))
        _PAR[key] = (rng.normal(size=(8, size)) * 3.0, rng.normal(size=(8, size - len(const))))
    return _PAR[key]


# ---- functors ----------------------------------------------------------------------------------------------------------------
# id -> (number of residuals, block sizes, number of constants); csrc/functors.hpp
FUNCTORS = {1: (2, (9, 3), 2), 2: (1, (1, 1), 2), 3: (1, (1, 1), 0), 4: (1, (1, 1), 0), 5: (1, (1, 1), 0), 6: (1, (1, 1), 0),
            7: (1, (2, 2), 1), 8: (3, (2, 2), 1), 9: (1, (1,) * 10, 0), 11: (1, (1,), 0), 12: (3, (4,), 6)}
SNAVELY_NORMS = (0.0, 1e-9, 1.4e-8, 1.6e-8, 1e-6, 1e-3, 1.0, np.pi - 1e-6)
_FUN = {}


def functor_inputs(fid):
    """(consts [m, nc], params [m, sum N]): 8 points, Snavely 8 more at the camera angle-axis norms of SNAVELY_NORMS."""
    if fid not in _FUN:
        nres, sizes, nc = FUNCTORS[fid]
        rng = np.random.default_rng(8000 + fid)
        m = 8
        c = rng.normal(size=(m, nc))
        p = rng.normal(size=(m, sum(sizes)))
        if fid == 1:
            m = 16
            cam = np.concatenate([rng.normal(0, 0.3, (m, 3)), rng.normal(0, 1, (m, 3)), rng.uniform(400, 1200, (m, 1)),
                                  rng.normal(0, 1e-6, (m, 1)), rng.normal(0, 1e-11, (m, 1))], axis=1)
            for i, t in enumerate(SNAVELY_NORMS):
                cam[8 + i, :3] = t * _unit(rng.normal(size=3))
            p = np.concatenate([cam, rng.normal(0, 1, (m, 3)) + [0, 0, -5]], axis=1)
            c = rng.normal(0, 100, (m, 2))
        if fid == 2:
            p *= 0.3
        _FUN[fid] = (c, p)
    return _FUN[fid]


def snavely_theta(p):
    return np.sqrt(np.sum(p[:, :3] ** 2, axis=1))


# ---- the corrector -----------------------------------------------------------------------------------------------------------
CORRECTOR_LOSSES = [("tolerant", 1.5, 0.4), ("scaled", ("tolerant", 0.7, 0.2), 2.0), ("tolerant", 40.0, 1.0), ("cauchy", 0.5),
                    ("huber", 1.3), ("tukey", 2.0), ("softlone", 0.7)]
_COR = None


def corrector_inputs():
    """(loss, r [k], J [k, 4]) for k = 1, 2, 3, three draws per loss and k at |r| scaled by 1/4, 1, 4.  r lies on a grid of 1/32,
    so |r|^2 is the same double in whatever order and with whatever fused multiply-adds it is summed: rho is then evaluated at
    exactly the squared norm the code under test formed."""
    global _COR
    if _COR is None:
        rng = np.random.default_rng(9100)
        _COR = []
        for spec in CORRECTOR_LOSSES:
            for k in (1, 2, 3):
                for scale in (0.25, 1.0, 4.0):
                    r = rng.integers(1, 13, size=k) * rng.choice([-1.0, 1.0], size=k) / 8.0 * scale
                    _COR.append((spec, r, rng.normal(size=(k, 4))))
    return _COR
