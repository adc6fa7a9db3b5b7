"""An extended-precision reference of a recorded functor body ("tape", skeres_amd/tape.py) with a running error bound.

Test infrastructure, CPU only: mpmath, numpy and the pure-Python recorder; nothing of the native library.  Three evaluators
of the tuple (instructions, literals, registers, outputs) that sk_cost_function_new_tape takes, and a generated corpus:

``reference(tape, x, captured)``
    Forward-mode autodiff from the textbook rules over pairs (value at PREC bits; bound e on the error of a float64
    evaluation of the same quantity).  + - x: the propagated bound plus u |result|, u = 2^-53.  A library function f:
    max |f'| over [x - e, x + e] times e, plus k_f u |f(x)|, k_f from the ULP_* table below.  The derivative of a function is
    formed from the same bounded operations (asin' = 1 / sqrt(1 - x x): a product, a difference, a square root, a quotient),
    so its bound carries the cancellation of 1 - x x near the ends of the domain.  A quotient is bounded in the order a
    reciprocal-multiply evaluates it (g' = 1 / g, q = f g', q' = g' (f' - q g')), as is atan2's derivative
    (t = 1 / (x x + y y), x t, -(y t)).  The bound is first order in u for ONE operation order; a comparison against it allows a
    factor 2 for another order (FMA contraction, a true division, tan' as 1 / cos^2).
    A comparison whose operands are closer than their bounds raises ``Undecided`` (exact operands — bound 0 — always decide,
    equality included), as does an |x| whose argument's sign lies within its bound.  A SELECT copies the arm taken; the other arm may be anything: an operation outside its domain
    poisons its register and a poisoned OUTPUT raises ``Poisoned``.

``run_np(tape, X, captured, dtype, W, defects)``
    The same tape in numpy, one lane per row of X, in float64 (the "twin": what a correct device evaluation computes up to
    operation order) or np.longdouble (the LM-level models of tests/step_check.py).  It is written as the pass loop of the
    device interpreter's description in DESIGN.md — passes of W derivative slots over a flat register array, component c of
    register r at r (W + 1) + c — so W = dim is plain forward mode, and W = 3, 2, 1 must give the same bits.  ``defects`` plants
    wrong rules (tests/test_tape_reference_cpu.py shows that each exceeds the bound).

``jet_twin(functor, x)``
    The generic body itself over rotation.Jet in float64: an evaluation that involves neither the recorder nor a tape.

The corpus (``random_cases``, ``directed_cases``) is generated from seeds: random generic bodies written with
skeres_amd.tape's functions and recorded through tape.record, so the recorder and its register allocation are inside the loop.
"""
import numpy as np
import mpmath

import skeres_amd as sk
from skeres_amd import tape as T
from skeres_amd.rotation import Jet

PREC = 200
M = mpmath.mp.clone()
M.prec = PREC
mpf = M.mpf
U = mpf(2) ** -53

# Allowances for the PLATFORM's math library, in ulp: the OpenCL full-profile limits for double precision that OCML is specified
# against (OpenCL C specification, "Relative error as ULPs", double-precision table; recalled, not copied from a text at hand):
ULP_SQRT = 3
ULP_DIVIDE = 3
ULP_EXP = 3
ULP_LOG = 3
ULP_SIN = 4
ULP_COS = 4
ULP_ASIN = 4
ULP_ACOS = 4
ULP_TAN = 5
ULP_ATAN = 5
ULP_ATAN2 = 6

OPCODE_NAMES = ("MOV", "ADD", "SUB", "MUL", "DIV", "NEG", "SQRT", "EXP", "LOG", "SIN", "COS", "TAN", "ASIN", "ACOS", "ATAN", "ATAN2",
                "ABS", "LT", "LE", "SELECT")
assert [getattr(T, n) for n in OPCODE_NAMES] == list(range(20))


class Undecided(Exception):
    """A comparison whose operands are closer than their error bounds: not a case for the corpus."""


class Poisoned(Exception):
    """An output depends on an operation outside its domain."""


class _Poison(Exception):
    pass


# ---- values with a bound ---------------------------------------------------------------------------------------------
class B:
    """value in extended precision + bound on the error of a float64 evaluation of the same quantity"""
    __slots__ = ("x", "e")

    def __init__(self, x, e=0):
        self.x, self.e = mpf(x), mpf(e)

    def exact(self, v):
        return self.e == 0 and self.x == v


def _rnd(x, e, k=1):
    return B(x, e + k * U * abs(x))


def b_neg(a):
    return B(-a.x, a.e)


def b_add(a, b):
    if b.exact(0):
        return a
    if a.exact(0):
        return b
    return _rnd(a.x + b.x, a.e + b.e)


def b_sub(a, b):
    if b.exact(0):
        return a
    if a.exact(0):
        return b_neg(b)
    return _rnd(a.x - b.x, a.e + b.e)


def b_mul(a, b):
    for p, q in ((a, b), (b, a)):
        if p.exact(0):
            return B(0)
        if p.exact(1):
            return q
        if p.exact(-1):
            return b_neg(q)
    return _rnd(a.x * b.x, abs(a.x) * b.e + abs(b.x) * a.e + a.e * b.e)


def _fn(a, f, absdf, k, domain=None):
    """f(a): max |f'| over [a - e, a + e] (|f'| of every function here is monotone on each side of at most one extremum, which
    lies at the middle of the domain: its values at the two ends and at the centre bound it up to second order in e) times e,
    plus k ulp of the result.  domain(lo, hi): False when the interval leaves the open domain of f."""
    lo, hi = a.x - a.e, a.x + a.e
    if domain is not None and not domain(lo, hi):
        raise _Poison()
    d = max(absdf(a.x), absdf(lo), absdf(hi)) if a.e != 0 else mpf(0)
    return _rnd(f(a.x), d * a.e, k)


def b_inv(a):
    return _fn(a, lambda x: 1 / x, lambda x: 1 / (x * x), ULP_DIVIDE, lambda lo, hi: lo > 0 or hi < 0)


def b_sqrt(a):
    return _fn(a, M.sqrt, lambda x: 1 / (2 * M.sqrt(x)), ULP_SQRT, lambda lo, hi: lo > 0)


def _same_branch_of_tan(lo, hi):
    return M.floor(lo / M.pi + mpf(0.5)) == M.floor(hi / M.pi + mpf(0.5)) and M.cos(lo) != 0 and M.cos(hi) != 0


_ONE = B(1)
_inside = lambda lo, hi: lo > -1 and hi < 1  # noqa: E731


def _unary(op, x):
    """(f(x), f'(x)) as bounded values, the derivative formed from bounded operations"""
    if op == T.SQRT:
        f = b_sqrt(x)
        return f, _scale_half(b_inv(f))
    if op == T.EXP:
        f = _fn(x, M.exp, M.exp, ULP_EXP)
        return f, f
    if op == T.LOG:
        return _fn(x, M.log, lambda t: 1 / abs(t), ULP_LOG, lambda lo, hi: lo > 0), b_inv(x)
    if op == T.SIN:
        return _fn(x, M.sin, lambda t: abs(M.cos(t)), ULP_SIN), _fn(x, M.cos, lambda t: abs(M.sin(t)), ULP_COS)
    if op == T.COS:
        return _fn(x, M.cos, lambda t: abs(M.sin(t)), ULP_COS), b_neg(_fn(x, M.sin, lambda t: abs(M.cos(t)), ULP_SIN))
    if op == T.TAN:
        f = _fn(x, M.tan, lambda t: 1 + M.tan(t) ** 2, ULP_TAN, _same_branch_of_tan)
        return f, b_add(_ONE, b_mul(f, f))
    if op in (T.ASIN, T.ACOS):
        d = b_inv(b_sqrt(b_sub(_ONE, b_mul(x, x))))
        if op == T.ASIN:
            return _fn(x, M.asin, lambda t: 1 / M.sqrt(1 - t * t), ULP_ASIN, _inside), d
        return _fn(x, M.acos, lambda t: 1 / M.sqrt(1 - t * t), ULP_ACOS, _inside), b_neg(d)
    if op == T.ATAN:
        return _fn(x, M.atan, lambda t: 1 / (1 + t * t), ULP_ATAN), b_inv(b_add(_ONE, b_mul(x, x)))
    raise AssertionError(op)


def _scale_half(a):
    return B(a.x / 2, a.e / 2)  # a power of two: exact


class D:
    """dual number over B: a + sum_k v[k] eps_k; v holds the non-zero parts only"""
    __slots__ = ("a", "v")

    def __init__(self, a, v=None):
        self.a, self.v = a, v or {}


_ZERO = B(0)


def _lin(x, y, f):
    return {k: f(x.v.get(k, _ZERO), y.v.get(k, _ZERO)) for k in set(x.v) | set(y.v)}


class Reference:
    """What reference() returns: r [nres], J [nres, dim] as long doubles (the extended values rounded once more: 2^-64 relative),
    r_bound / J_bound as doubles (rounded up), ops: the opcodes of the instructions the outputs depend on."""

    def __init__(self, r, J, r_bound, J_bound, ops):
        self.r, self.J, self.r_bound, self.J_bound, self.ops = r, J, r_bound, J_bound, ops


def reference(tape, x, captured=()):
    ins, consts, nregs, outs = tape
    n = len(x)
    regs = [None] * max(1, int(nregs))

    def val(code):
        kind, idx = (int(code) >> 28) & 7, int(code) & 0x0FFFFFFF
        if kind == T.REGISTER:
            if regs[idx] is None:
                raise _Poison()
            return regs[idx]
        if kind == T.PARAMETER:
            return D(B(float(x[idx])), {idx: _ONE})
        if kind == T.CAPTURED:
            return D(B(float(captured[idx])))
        return D(B(float(consts[idx])))

    for op, dst, a, b, c in np.asarray(ins).reshape(-1, 5).tolist():
        try:
            if op == T.MOV:
                r = val(a)
            elif op == T.ADD:
                p, q = val(a), val(b)
                r = D(b_add(p.a, q.a), _lin(p, q, b_add))
            elif op == T.SUB:
                p, q = val(a), val(b)
                r = D(b_sub(p.a, q.a), _lin(p, q, b_sub))
            elif op == T.MUL:
                p, q = val(a), val(b)
                r = D(b_mul(p.a, q.a), _lin(p, q, lambda s, t: b_add(b_mul(q.a, s), b_mul(p.a, t))))
            elif op == T.DIV:
                p, q = val(a), val(b)
                gi = b_inv(q.a)
                quo = b_mul(p.a, gi)
                r = D(quo, _lin(p, q, lambda s, t: b_mul(gi, b_sub(s, b_mul(quo, t)))))
            elif op == T.NEG:
                p = val(a)
                r = D(b_neg(p.a), {k: b_neg(s) for k, s in p.v.items()})
            elif op == T.ATAN2:
                y, xx = val(a), val(b)
                den = b_add(b_mul(xx.a, xx.a), b_mul(y.a, y.a))
                if den.x - den.e <= 0:
                    raise _Poison()
                t = b_inv(den)
                cy, cx = b_mul(xx.a, t), b_neg(b_mul(y.a, t))
                # |d atan2 / dy| = |x| / (x^2 + y^2), |d atan2 / dx| = |y| / (x^2 + y^2)
                spread = (abs(xx.a.x) + xx.a.e) * y.a.e + (abs(y.a.x) + y.a.e) * xx.a.e
                lo = (max(abs(xx.a.x) - xx.a.e, 0)) ** 2 + (max(abs(y.a.x) - y.a.e, 0)) ** 2
                if spread != 0 and lo <= 0:
                    raise _Poison()
                fa = _rnd(M.atan2(y.a.x, xx.a.x), spread / lo if spread != 0 else 0, ULP_ATAN2)
                r = D(fa, _lin(xx, y, lambda s, t: b_add(b_mul(cx, s), b_mul(cy, t))))
            elif op == T.ABS:
                p = val(a)
                if p.a.e != 0 and abs(p.a.x) <= p.a.e:
                    raise Undecided("the sign of |x|'s argument lies within its error bound")
                r = D(b_neg(p.a), {k: b_neg(s) for k, s in p.v.items()}) if p.a.x < 0 else p
            elif op in (T.LT, T.LE):
                p, q = val(a), val(b)
                if (p.a.e != 0 or q.a.e != 0) and abs(p.a.x - q.a.x) <= p.a.e + q.a.e:
                    raise Undecided("comparison within the error bound")
                r = D(B(1.0 if (p.a.x < q.a.x if op == T.LT else p.a.x <= q.a.x) else 0.0))
            elif op == T.SELECT:
                r = val(b) if val(a).a.x != 0 else val(c)
            elif 0 <= op < len(OPCODE_NAMES):
                p = val(a)
                f, df = _unary(op, p.a)
                r = D(f, {k: b_mul(df, s) for k, s in p.v.items()})
            else:
                raise AssertionError("opcode %d" % op)
        except _Poison:
            r = None
        regs[dst] = r
    nres = len(outs)
    rv, rb = np.zeros(nres, dtype=np.longdouble), np.zeros(nres)
    Jv, Jb = np.zeros((nres, n), dtype=np.longdouble), np.zeros((nres, n))
    for i, o in enumerate(outs):
        try:
            d = val(o)
        except _Poison:
            raise Poisoned("residual %d" % i)
        rv[i], rb[i] = _ld(d.a.x), _up(d.a.e)
        for k, s in d.v.items():
            Jv[i, k], Jb[i, k] = _ld(s.x), _up(s.e)
    return Reference(rv, Jv, rb, Jb, live_opcodes(tape))


def _ld(x):
    """an extended value as a long double (two doubles: head and tail)"""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - mpf(hi)))


def _up(e):
    return 0.0 if e == 0 else float(np.nextafter(float(e), np.inf))  # (float() rounds to nearest: one step up covers it)


def live_opcodes(tape):
    """opcodes of the instructions some output depends on (through either arm of a SELECT)"""
    ins, _, _, outs = tape
    ins = np.asarray(ins).reshape(-1, 5).tolist()
    need = {int(o) & 0x0FFFFFFF for o in outs if (int(o) >> 28) & 7 == T.REGISTER}
    ops = set()
    for op, dst, a, b, c in reversed(ins):
        if dst in need:
            need.discard(dst)
            ops.add(op)
            for o in (a, b, c)[:_ARITY.get(op, 1)]:
                if (o >> 28) & 7 == T.REGISTER:
                    need.add(o & 0x0FFFFFFF)
    return ops


_ARITY = {T.ADD: 2, T.SUB: 2, T.MUL: 2, T.DIV: 2, T.ATAN2: 2, T.LT: 2, T.LE: 2, T.SELECT: 3}


# ---- the tape in numpy: float64 twin, long double model, planted defects ------------------------------------------------
DEFECTS = {  # name -> opcodes the planted rule belongs to
    "tan' = 1 + tan": (T.TAN,),
    "acos' with the sign of asin'": (T.ACOS,),
    "asin' = 1/sqrt(1 + x^2)": (T.ASIN,),
    "atan' = 1/(1 - x^2)": (T.ATAN,),
    "sqrt' = 1/sqrt(x)": (T.SQRT,),
    "cos' = +sin": (T.COS,),
    "sin' rounded to float32": (T.SIN,),
    "log' rounded to float32": (T.LOG,),
    "exp rounded to float32": (T.EXP,),
    "quotient rule without q g'": (T.DIV,),
    "product rule without f g'": (T.MUL,),
    "sum that drops g'": (T.ADD,),
    "difference that adds g'": (T.SUB,),
    "negation that keeps f'": (T.NEG,),
    "move that drops f'": (T.MOV,),
    "atan2 with dy and dx swapped": (T.ATAN2,),
    "abs that keeps f' of a negative": (T.ABS,),
    "select that blends": (T.SELECT,),
    "LE evaluated as LT": (T.LE,),
    "LT evaluated as LE": (T.LT,),
    "last pass writes past dim": tuple(range(20)),
    "register stride W": tuple(range(20)),
}


def run_np(tape, X, captured=(), dtype=np.float64, W=None, defects=()):
    """r [nb, nres], J [nb, nres, dim] of the tape at the rows of X [nb, dim] (captured [nb, ncap] or one row for all).
    W derivative slots per pass (None: dim, one pass)."""
    ins, consts, nregs, outs = tape
    ins = np.asarray(ins).reshape(-1, 5).tolist()
    X = np.atleast_2d(np.asarray(X, dtype=dtype))
    nb, dim = X.shape
    cap = np.atleast_2d(np.asarray(captured, dtype=dtype)) if len(np.asarray(captured).ravel()) else np.zeros((1, 0), dtype=dtype)
    cap = np.broadcast_to(cap, (nb, cap.shape[1]))
    W = dim if W is None else int(W)
    R, nres = max(1, int(nregs)), len(outs)
    stride = W if "register stride W" in defects else W + 1
    f32 = lambda v: v.astype(np.float32).astype(dtype)  # noqa: E731
    one, zero = dtype(1), dtype(0)
    r_out = np.zeros((nb, nres), dtype=dtype)
    J_flat = np.zeros((nb, nres * dim + W), dtype=dtype)  # row-major nres x dim, and room for the planted overrun
    flat = np.zeros((R * (W + 1), nb), dtype=dtype)       # component c of register r at r (W + 1) + c

    with np.errstate(all="ignore"):
        for first in range(0, dim, W):
            def fetch(code):
                kind, idx = (code >> 28) & 7, code & 0x0FFFFFFF
                if kind == T.REGISTER:
                    p = idx * stride
                    return flat[p].copy(), flat[p + 1:p + 1 + W].copy()
                v = np.zeros((W, nb), dtype=dtype)
                if kind == T.PARAMETER:
                    if 0 <= idx - first < W:
                        v[idx - first] = one
                    return X[:, idx].copy(), v
                if kind == T.CAPTURED:
                    return cap[:, idx].copy(), v
                return np.full(nb, dtype(consts[idx])), v

            for op, dst, a, b, c in ins:
                if op == T.MOV:
                    f, v = fetch(a)
                    if "move that drops f'" in defects:
                        v = v * zero
                elif op in (T.ADD, T.SUB):
                    (p, pv), (q, qv) = fetch(a), fetch(b)
                    if op == T.ADD:
                        f, v = p + q, pv if "sum that drops g'" in defects else pv + qv
                    else:
                        f, v = p - q, pv + qv if "difference that adds g'" in defects else pv - qv
                elif op == T.MUL:
                    (p, pv), (q, qv) = fetch(a), fetch(b)
                    f, v = p * q, q * pv if "product rule without f g'" in defects else q * pv + p * qv
                elif op == T.DIV:
                    (p, pv), (q, qv) = fetch(a), fetch(b)
                    f = p / q
                    v = pv / q if "quotient rule without q g'" in defects else (pv - f * qv) / q
                elif op == T.NEG:
                    p, pv = fetch(a)
                    f, v = -p, pv if "negation that keeps f'" in defects else -pv
                elif op == T.ATAN2:
                    (y, yv), (x, xv) = fetch(a), fetch(b)
                    if "atan2 with dy and dx swapped" in defects:
                        yv, xv = xv, yv
                    f, v = np.arctan2(y, x), (x * yv - y * xv) / (x * x + y * y)
                elif op == T.ABS:
                    p, pv = fetch(a)
                    ng = p < 0
                    f, v = np.where(ng, -p, p), pv if "abs that keeps f' of a negative" in defects else np.where(ng, -pv, pv)
                elif op in (T.LT, T.LE):
                    (p, _), (q, qv) = fetch(a), fetch(b)
                    strict = (op == T.LT) != (("LT evaluated as LE" in defects and op == T.LT) or ("LE evaluated as LT" in defects and op == T.LE))
                    f, v = np.where(p < q if strict else p <= q, one, zero).astype(dtype), qv * zero
                elif op == T.SELECT:
                    (s, _), (p, pv), (q, qv) = fetch(a), fetch(b), fetch(c)
                    if "select that blends" in defects:
                        f, v = s * p + (one - s) * q, s * pv + (one - s) * qv
                    else:
                        f, v = np.where(s != 0, p, q), np.where(s != 0, pv, qv)
                else:
                    p, pv = fetch(a)
                    if op == T.SQRT:
                        f = np.sqrt(p)
                        d = one / f if "sqrt' = 1/sqrt(x)" in defects else dtype(0.5) / f
                    elif op == T.EXP:
                        f = np.exp(p)
                        if "exp rounded to float32" in defects:
                            f = f32(f)
                        d = f
                    elif op == T.LOG:
                        f, d = np.log(p), one / p
                        if "log' rounded to float32" in defects:
                            d = f32(d)
                    elif op == T.SIN:
                        f, d = np.sin(p), np.cos(p)
                        if "sin' rounded to float32" in defects:
                            d = f32(d)
                    elif op == T.COS:
                        f, d = np.cos(p), np.sin(p) if "cos' = +sin" in defects else -np.sin(p)
                    elif op == T.TAN:
                        f = np.tan(p)
                        d = one + f if "tan' = 1 + tan" in defects else one + f * f
                    elif op == T.ASIN:
                        f = np.arcsin(p)
                        d = one / np.sqrt(one + p * p) if "asin' = 1/sqrt(1 + x^2)" in defects else one / np.sqrt(one - p * p)
                    elif op == T.ACOS:
                        f = np.arccos(p)
                        d = one / np.sqrt(one - p * p)
                        if "acos' with the sign of asin'" not in defects:
                            d = -d
                    elif op == T.ATAN:
                        f = np.arctan(p)
                        d = one / (one - p * p) if "atan' = 1/(1 - x^2)" in defects else one / (one + p * p)
                    else:
                        raise AssertionError("opcode %d" % op)
                    v = d * pv
                p0 = dst * stride
                flat[p0] = f
                flat[p0 + 1:p0 + 1 + W] = v
            outv = [fetch(int(o)) for o in outs]
            if first == 0:
                for r in range(nres):
                    r_out[:, r] = outv[r][0]
            for w in range(W):
                if first + w >= dim and "last pass writes past dim" not in defects:
                    break
                for r in range(nres):
                    J_flat[:, r * dim + first + w] = outv[r][1][w]
    return r_out, J_flat[:, :nres * dim].reshape(nb, nres, dim)


def jet_twin(functor, x):
    """The generic body over rotation.Jet: (r [nres], J [nres, dim]) in float64."""
    dim = len(x)
    blocks, k = [], 0
    for n in functor.N:
        blocks.append([Jet(float(x[k + j]), k + j, dim) for j in range(n)])
        k += n
    with np.errstate(all="ignore"):
        y = functor.apply(*blocks)
    r = np.array([float(v) for v in y])
    J = np.array([v.infinitesimal if isinstance(v, Jet) else np.zeros(dim) for v in y]).reshape(len(y), dim)
    return r, J


def ratio(value, ref_value, bound):
    """max |value - reference| / bound over the entries; an entry whose bound is 0 (exactly known) must agree exactly: inf if not."""
    d = np.abs(np.asarray(value, dtype=np.longdouble) - ref_value)
    with np.errstate(all="ignore"):
        q = np.where(d == 0, 0.0, np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.inf))
    q = np.where(np.isnan(d), np.inf, q)
    return float(np.max(q)) if q.size else 0.0


def worst_ratio(ref, r, J):
    return max(ratio(r, ref.r, ref.r_bound), ratio(J, ref.J, ref.J_bound))


# ---- renumbering a tape's registers --------------------------------------------------------------------------------------
def renumber(tape, R, seed=0):
    """The same tape with its registers renumbered into a declared file of R >= registers: a random injection that uses R - 1."""
    ins, consts, nregs, outs = tape
    nregs = int(nregs)
    assert R >= max(1, nregs)
    rng = np.random.default_rng(seed)
    image = rng.permutation(R)[:nregs]
    if nregs and R - 1 not in image:
        image[int(rng.integers(nregs))] = R - 1
    remap = lambda o: (int(o) & ~0x0FFFFFFF) | int(image[int(o) & 0x0FFFFFFF]) if (int(o) >> 28) & 7 == T.REGISTER else int(o)  # noqa: E731
    out_ins = []
    for op, dst, a, b, c in np.asarray(ins).reshape(-1, 5).tolist():
        ops = [a, b, c]
        for k in range(_ARITY.get(op, 1)):
            ops[k] = remap(ops[k])
        out_ins.append([op, int(image[dst])] + ops)
    return (np.asarray(out_ins, dtype=np.int32).reshape(-1, 5), consts, R, np.asarray([remap(o) for o in outs], dtype=np.int32))


def with_moves(tape):
    """A hand-edited tape: every output goes through a MOV into a register of its own, the first parameter through another."""
    ins, consts, nregs, outs = tape
    ins, nregs = np.asarray(ins).reshape(-1, 5).tolist(), int(nregs)
    new_outs = []
    for o in outs:
        ins.append([T.MOV, nregs, int(o), 0, 0])
        new_outs.append((T.REGISTER << 28) | nregs)
        nregs += 1
    return (np.asarray(ins, dtype=np.int32).reshape(-1, 5), consts, nregs, np.asarray(new_outs, dtype=np.int32))


def pick_width(num_registers, threads):
    """The interpreter's plan as DESIGN.md states it: the widest of W = 3, 2, 1 whose register file, registers x (W + 1) x threads
    doubles, leaves room for two workgroups in 144 KiB of LDS, else the widest that fits at all; 0: none.  Returns (W, bytes)."""
    size = lambda W: max(1, num_registers) * (W + 1) * threads * 8  # noqa: E731
    for budget in (72 * 1024, 144 * 1024):
        for W in (3, 2, 1):
            if size(W) <= budget:
                return W, size(W)
    return 0, 0


# ---- the corpus --------------------------------------------------------------------------------------------------------------
KINDS = ("add", "sub", "mul", "div", "neg", "sqrt", "exp", "log", "sin", "cos", "tan", "tanp", "asin", "acos", "atan", "atan2",
         "atan2q", "abs", "where", "wherele", "wherege", "pow3", "lit", "cap")


class Body:
    """A random generic body: steps over a pool of values, written with the generic functions of skeres_amd.tape.  Steps keep
    their arguments inside the functions' domains by construction, and cover both signs and all quadrants."""

    def __init__(self, rng, sizes, nres, nsteps, ncap=2, touch_all=False, kinds=KINDS):
        self.N, self.k, self.ncap = list(sizes), nres, ncap
        dim = sum(sizes)
        npool = dim + ncap
        self.steps = []
        for _ in range(nsteps):
            kind = str(rng.choice(kinds))
            if kind == "cap" and ncap == 0:
                kind = "lit"
            recent = npool - 1 - int(rng.integers(min(npool, 6)))  # one argument from the latest values: chains, not only leaves
            i, j, l = recent, int(rng.integers(npool)), int(rng.integers(max(1, ncap)))
            if j == i and npool > 1:
                j = (i + 1) % npool                 # (a < a is no comparison to test)
            self.steps.append((kind, i, j, l, float(rng.uniform(0.5, 2.0))))
            npool += 1
        self.outs = [int(rng.integers(dim + ncap, npool)) if nsteps else int(rng.integers(npool)) for _ in range(nres)]
        if nsteps:
            self.outs[0] = npool - 1
        # every parameter enters some residual: residual k % nres gets  + w_k x_k pool[j_k]
        # (touch_all = "leaves": pool[j_k] a parameter or a captured double, so the terms keep no register alive)
        top = dim + ncap if touch_all == "leaves" else npool
        self.touch = [(k, int(rng.integers(top)), float(rng.uniform(0.5, 2.0))) for k in range(dim)] if touch_all else []

    def apply(self, captured, *blocks):
        flat = [v for b in blocks for v in b]
        pool = flat + list(captured)
        cap0 = len(flat)
        for kind, i, j, l, c in self.steps:
            a, b = pool[i], pool[j]
            if kind == "add": r = a + b
            elif kind == "sub": r = a - c * b
            elif kind == "mul": r = a * b
            elif kind == "div": r = a / (c + b * b)
            elif kind == "neg": r = -a + 0.5 * b
            elif kind == "sqrt": r = T.sqrt(c + a * a)
            elif kind == "exp": r = T.exp(T.sin(a))
            elif kind == "log": r = T.log(c + a * a)
            elif kind == "sin": r = T.sin(a)
            elif kind == "cos": r = T.cos(a)
            elif kind == "tan": r = T.tan(0.7 * T.sin(a))
            elif kind == "tanp": r = T.tan(1.45 * T.sin(a))     # up to 0.12 from the pole: tan' up to 70
            elif kind == "asin": r = T.asin(0.8 * T.sin(a))
            elif kind == "acos": r = T.acos(0.8 * T.cos(a))     # both signs of the argument
            elif kind == "atan": r = T.atan(a)
            elif kind == "atan2": r = T.atan2(a, c + b * b)
            elif kind == "atan2q": r = T.atan2(T.sin(a) + 0.25 * c, T.cos(b) - 0.3)   # all four quadrants
            elif kind == "abs": r = abs(a) + 0.25 * b
            elif kind == "where": r = T.where(a < b, lambda: T.sqrt(b - a), lambda: 1.0 / (c + (a - b)))
            elif kind == "wherele": r = T.where(a <= c * b, lambda: T.log(c * b - a + 1.0), lambda: T.sqrt(a - c * b))
            elif kind == "wherege": r = T.where(a >= b, lambda: (a - b) * a, lambda: T.exp(a - b))
            elif kind == "pow3": r = T.sin(a) ** 3
            elif kind == "cap": r = a * pool[cap0 + l] + c
            else: r = c * a + 0.25
            pool.append(r)
        out = [pool[o] for o in self.outs]
        for k, j, w in self.touch:
            out[k % self.k] = out[k % self.k] + (w * flat[k]) * pool[j]
        return out


class BodyFunctor(sk.TracedCostFunctor):
    """A Body as the generic functor a user would write: records through tape.record, evaluates over floats and Jets."""

    def __init__(self, body, captured=()):
        super().__init__(body.k, *body.N, captured=captured)
        self.body = body

    def apply(self, *blocks):
        return self.body.apply(self.captured_values(), *blocks)


class FixedTapeFunctor(sk.TracedCostFunctor):
    """A functor whose tape is given (a renumbered or hand-built one): TracedCostFunction and addResidualBlocksTraced pass it on."""

    def __init__(self, tape, nres, sizes, captured=()):
        super().__init__(nres, *sizes, captured=captured)
        self._fixed = tape

    def tape(self):
        return self._fixed


class Case:
    def __init__(self, name, functor, x, directed=False, tape=None):
        self.name, self.functor, self.x, self.directed = name, functor, np.asarray(x, dtype=np.float64), directed
        self.tape = functor.tape() if tape is None else tape
        self.sizes, self.nres, self.captured = list(functor.N), functor.kNumResiduals, tuple(functor.captured)
        self.dim = int(sum(self.sizes))
        self._ref = None

    def reference(self):
        """Reference, or the exception (Undecided / Poisoned) that drops the case; computed once"""
        if self._ref is None:
            try:
                self._ref = reference(self.tape, self.x, self.captured)
            except (Undecided, Poisoned) as e:
                self._ref = e
        return self._ref

    def device_functor(self):
        return self.functor if self.tape is self.functor.tape() else FixedTapeFunctor(self.tape, self.nres, self.sizes, self.captured)


def _body_case(name, rng, sizes, nres, nsteps, ncap, directed=False, touch_all=False, kinds=KINDS, spread=1.0):
    body = Body(rng, sizes, nres, nsteps, ncap, touch_all=touch_all, kinds=kinds)
    f = BodyFunctor(body, captured=rng.normal(0, 1, ncap))
    return Case(name, f, rng.normal(0, spread, sum(sizes)), directed=directed)


def random_cases(n=150, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        sizes = [int(rng.integers(1, 6)) for _ in range(int(rng.integers(1, 6)))]
        out.append(_body_case("random-%d" % c, rng, sizes, int(rng.integers(1, 5)), int(rng.integers(3, 40)), int(rng.integers(0, 4)),
                              spread=float(rng.choice([0.5, 1.0, 3.0]))))
    return out


class _Equality(sk.TracedCostFunctor):
    """LT / LE at equality, in the four forms a body can write them: x < y, x <= y, x > y, x >= y against a parameter, a
    literal and a captured double — all exact, so always decided."""

    def __init__(self, form, other, c):
        super().__init__(2, 2, 1, captured=(c,))
        self.form, self.other = form, other

    def apply(self, x, y):
        (c,) = self.captured_values()
        a = x[0]
        b = {"parameter": x[1], "literal": 0.75, "captured": c}[self.other]
        cond = {"lt": lambda: a < b, "le": lambda: a <= b, "gt": lambda: a > b, "ge": lambda: a >= b}[self.form]()
        return [T.where(cond, lambda: T.sin(a) * y[0], lambda: T.cos(a) + y[0] * y[0]), T.where(cond, 2.0 * a, -3.0 * y[0]) + x[1]]


class _Passthrough(sk.TracedCostFunctor):
    """literals, captured doubles and parameters as outputs: no instruction at all"""

    def __init__(self):
        super().__init__(4, 2, 1, captured=(7.5,))

    def apply(self, x, y):
        (c,) = self.captured_values()
        return [x[1], y[0], 3.25, c]


class _Signs(sk.TracedCostFunctor):
    """the rules where a sign or a quadrant matters, at a point chosen by the case: acos / asin of both signs, abs of both signs,
    atan2 in a given quadrant, tan on both sides of zero"""

    def __init__(self):
        super().__init__(3, 2, 2)

    def apply(self, p, q):
        return [T.acos(p[0]) * T.asin(p[0]) + abs(p[1]) * q[0], T.atan2(q[0], q[1]) + T.atan(p[1]) * p[0],
                T.tan(p[1]) - abs(q[1] * p[0]) / T.sqrt(q[0] * q[0] + 1.0)]


def directed_cases(seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for dim in (1, 2, 3, 4, 5, 7, 12, 13, 63, 64):   # each of W = 3, 2, 1 divides some and not others
        out.append(_body_case("dim-%d" % dim, rng, [dim], 2, 24, 1, directed=True, touch_all=True))
    for nres in (1, 2, 15, 16):
        out.append(_body_case("residuals-%d" % nres, rng, [3, 2], nres, 30, 2, directed=True, touch_all=True))
    for nb in (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 48, 63, 64):
        out.append(_body_case("blocks-%d" % nb, rng, [1] * nb, 3, 20, 1, directed=True, touch_all=True))
    out.append(_body_case("blocks-7-13-1-43", rng, [7, 13, 1, 43], 5, 30, 3, directed=True, touch_all=True))
    for form in ("lt", "le", "gt", "ge"):
        for other in ("parameter", "literal", "captured"):
            v = {"parameter": 0.4, "literal": 0.75, "captured": -1.25}[other]
            out.append(Case("equality-%s-%s" % (form, other), _Equality(form, other, -1.25), [v, 0.4, 0.9], directed=True))
    out.append(Case("passthrough", _Passthrough(), [1.5, -2.0, 4.0], directed=True))
    for k, x in enumerate([(-0.6, -1.2, 0.5, 0.8), (0.6, 1.2, 0.5, -0.8), (-0.95, -0.3, -0.5, -0.8), (0.95, 0.3, -0.5, 0.8), (-0.1, 1.5, 2.0, -1e-3),
                           (0.1, -1.5, -2.0, 1e-3)]):
        out.append(Case("signs-%d" % k, _Signs(), x, directed=True))
    for k in range(4):  # hand-edited tapes: MOV is an opcode the recorder never emits
        base = _body_case("moves-%d" % k, rng, [2, 3], 3, 12, 1, directed=True, touch_all=True)
        out.append(Case(base.name, base.functor, base.x, directed=True, tape=with_moves(base.tape)))
    return out


def corpus():
    return random_cases() + directed_cases()


# ---- singular points: pinned against what the generic body gives over rotation.Jet (jet_twin), NaNs included ----------------
class _Singular(sk.TracedCostFunctor):
    def __init__(self, form):
        super().__init__(2, 2, captured=(0.0,))
        self.form = form

    def apply(self, x):
        (c,) = self.captured_values()
        u, v = x[0], x[1]
        if self.form == "sqrt":      # sqrt at 0: the seeded part becomes inf, the others inf * 0; of 0 u: every part inf * 0
            return [T.sqrt(u) + v, T.sqrt(c * u) * v]   # (sqrt of the captured double ALONE is a float on the host, a Jet on a tape)
        if self.form == "abs":       # abs at +0 / -0: not negative, so the value (its sign included) and the derivative pass through
            return [abs(u) * 3.0, abs(u * v) + v]
        if self.form == "nan-arm":   # the arm not taken is NaN in value and derivative (sqrt of a negative, log of a negative)
            return [T.where(u < v, lambda: u * v, lambda: T.sqrt(u - v) * T.log(u - v)), T.where(u >= v, lambda: T.sqrt(u - v), lambda: v - u)]
        if self.form == "inf-arm":   # ... and infinite: 1 / 0, exp of a large number, a quotient whose derivative overflows too
            return [T.where(u < v, lambda: u + v, lambda: 1.0 / (u - u)), T.where(u > v, lambda: T.exp(800.0 * u) / (v - v), lambda: T.sin(v))]
        raise AssertionError(self.form)


def singular_cases():
    """[(name, functor, x, expected (r, J) or None: what jet_twin gives)]"""
    P = T.PARAMETER << 28
    out = [("sqrt-at-0", _Singular("sqrt"), [0.0, 1.5], None),
           ("abs-at-plus-0", _Singular("abs"), [0.0, -2.0], None),
           ("abs-at-minus-0", _Singular("abs"), [-0.0, 2.0], None),
           ("abs-negative", _Singular("abs"), [-0.5, 2.0], None),
           ("nan-in-the-arm-not-taken", _Singular("nan-arm"), [1.0, 3.0], None),
           ("inf-in-the-arm-not-taken", _Singular("inf-arm"), [1.0, 3.0], None),
           ("passthrough", _Passthrough(), [1.5, -2.0, 4.0], None)]
    for form in ("lt", "le", "gt", "ge"):
        out.append(("equality-" + form, _Equality(form, "parameter", 0.0), [0.4, 0.4, 0.9], None))
    # a NaN condition (a hand-built tape: a body cannot write one): NaN != 0 holds, so as for Python's `if` the first arm is taken
    nan_select = (np.array([[T.SELECT, 0, P | 0, P | 1, P | 2]], dtype=np.int32), np.zeros(0), 1, np.array([T.REGISTER << 28], dtype=np.int32))
    out.append(("nan-condition", FixedTapeFunctor(nan_select, 1, [3]), [float("nan"), 2.5, -4.0], (np.array([2.5]), np.array([[0.0, 1.0, 0.0]]))))
    return out
