"""Backward error of a Cholesky factorisation and of the solve it gives, on matrices whose 128 x 128 diagonal blocks are
ill-conditioned.

CPU only: numpy, scipy and long double, nothing of skeres_amd's native library.  The role tests/step_check.py has for the LM
step, for the block-envelope Cholesky (chol_kernels.hip): the device forms a panel by multiplying with the explicit inverse
of the diagonal block, which is where a blocked Cholesky loses accuracy as those blocks get ill-conditioned, and a forward
comparison with another double-precision factor says nothing there.

Every matrix is Jacobi-scaled to an exact unit diagonal, as the solver's systems are.  Every row of any Cholesky factor of
such a matrix has 2-norm 1, so (|L||L^T|)_ij <= 1 whatever the elimination order.

    factor_ratio   = max_ij |A - L L^T|_ij / (gamma_{m_ij} (|L||L^T|)_ij)          gamma_k = k u / (1 - k u), u = 2^-53
    solve_row_ratio = max_i |A x - b|_i / (gamma_{3m+1} ||x||_1)                   m = the largest m_ij
    eta            = ||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf)           (reported, not asserted)

m_ij is the length of the dot product the blocked algorithm forms for entry (i, j): the columns k <= j inside the envelope of
both rows, rounded up to a multiple of 128, plus 128 for the product with the inverse diagonal block that replaces the division,
plus 1.  For an unblocked substitution Cholesky, factor_ratio <= 1 is Higham, Accuracy and Stability of Numerical Algorithms,
Theorem 10.3, and it holds for any order of summation; solve_row_ratio <= 1 follows from Theorem 10.4 with (|L||L^T|)_ij <= 1,
and since it does not mention the factor it applies to the dissected and segmented solves too.  Neither bound is a property of
an algorithm that multiplies with an explicit inverse; DESIGN.md section 4 says what is and is not promised.

Arithmetic.  A - L L^T is formed from products that are EXACT and sums in long double: over 1024 columns at a time every
row of L is scaled by a power of two and cut into slices of 20 bits, so a double-precision matrix product of two slices
is an integer below 2^53 times the grid, free of rounding, and the slice products are added up in long double
(_exact_nt; compared with a plain long-double product in tests/test_chol_check_cpu.py).  The few entries whose bound is not far above what the slices leave out
are plain long-double dot products.  The denominators |L||L^T| are double-precision products: their relative error of
a few thousand u moves a ratio by less than 1e-12 of itself.  Residuals A x - b are long double throughout.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse.linalg as spla

LD = np.longdouble
U_DOUBLE = 2.0 ** -53
BLOCK = 128
TILE = 32
DENSE_MAX = 1300          # above this factor_ratio samples
SAMPLE_ROWS, SAMPLE_COLS = 8, 2   # the lattice of the sampled form: 16 entries of every tile
KAPPAS = (1e2, 1e3, 1e4, 1e6, 1e8)
COND_MAX = 1e13
# Heights (active block rows below the diagonal) at which cholesky_plan changes regime: at most 24 trailing block rows run under
# the resident chain.  With jumps of the height (every hand-over of test_gpu_parity._PLAN_SHAPES is one) these are the places
# whose block rows the sampled factor_ratio reads entry by entry (regime_rows).
PLAN_THRESHOLDS = (24,)

# The kappa_b each shape carries: the largest of KAPPAS at which LAPACK factors the matrix and cond(A) <= COND_MAX
# (established by tests/test_chol_check_cpu.py::test_kappa_b_is_the_largest_the_shape_carries).
KAPPA_B = {
    ("hard_blocks", 128): 1e8,
    ("hard_blocks", 129): 1e8,
    ("hard_blocks", 257): 1e8,
    ("hard_blocks", 700): 1e4,
    ("banded_hard", "band"): 1e3,
    ("banded_hard", "resident-then-wide-then-resident"): 1e3,
    ("banded_hard", "odd-resident-run"): 1e3,
    ("banded_hard", "two-wide-parts"): 1e3,
    ("bordered_hard", "narrow-border"): 1e3,
    ("bordered_hard", "first-column-border"): 1e3,
    ("bordered_hard", "three-revisits"): 1e3,
    ("scalar_band", 40): 1e3,
}

# The bordered shapes of the GPU tests: three of test_bordered_factorisation_vs_numpy's seven.
BORDERED_SHAPES = {
    "narrow-border": ("band", (40,), (20,)),                        # a border narrower than a block
    "first-column-border": ("odd-resident-run", (500,), (0,)),      # reached by the very first block column
    "three-revisits": ("band", (200, 300, 250), (30, 18, 5)),
}


def _require_long_double():
    if np.finfo(LD).nmant < 63:
        raise RuntimeError("chol_check needs an 80-bit long double (np.finfo(np.longdouble).nmant = %d)" % np.finfo(LD).nmant)


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U_DOUBLE) / (1 - k * LD(U_DOUBLE))


# ---------------------------------------------------------------------------------------------------------------------
# matrix families
# ---------------------------------------------------------------------------------------------------------------------
def _unit_diagonal(A):
    """D A D with D = diag(A)^-1/2, exactly symmetric, the diagonal exactly 1."""
    d = 1.0 / np.sqrt(np.diag(A))
    low = np.tril(A * d[:, None] * d[None, :], -1)
    out = low + low.T
    out[np.arange(len(d)), np.arange(len(d))] = 1.0
    return out


def _gram(L0):
    """L0 L0^T, block column by block column over the rows each one reaches (the envelope keeps this far below n^3)."""
    n = L0.shape[0]
    A = np.zeros((n, n))
    for c in range(0, n, BLOCK):
        rows = np.nonzero(np.any(L0[:, c:c + BLOCK] != 0, axis=1))[0]
        cut = np.nonzero(np.diff(rows) > 1)[0] + 1             # a few contiguous runs: the band, the border
        runs = [(rows[a], rows[b - 1] + 1) for a, b in zip(np.r_[0, cut], np.r_[cut, len(rows)])] if len(rows) else []
        for a0, a1 in runs:
            for b0, b1 in runs:
                A[a0:a1, b0:b1] += L0[a0:a1, c:c + BLOCK] @ L0[b0:b1, c:c + BLOCK].T
    return A


def graded(n, kappa, seed):
    """Q diag(kappa^-t) Q^T, t linear on [0, 1], scaled to a unit diagonal: cond about 0.9 kappa."""
    rng = np.random.default_rng([int(seed), int(n), 17])
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    t = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
    return _unit_diagonal((Q * float(kappa) ** (-t)) @ Q.T)


def _hard_diagonal(L0, kappa_b, seed):
    """Every 128 x 128 diagonal block of L0 (on the grid of the whole matrix) := the Cholesky factor of a graded(., kappa_b)."""
    n = L0.shape[0]
    for c in range(0, n, BLOCK):
        e = min(n, c + BLOCK)
        L0[c:e, c:e] = np.linalg.cholesky(graded(e - c, kappa_b, seed + 1000 + c))
    return L0


def hard_blocks(n, kappa_b, seed):
    """A = L0 L0^T scaled; L0's diagonal blocks are factors of graded(., kappa_b) (condition about sqrt(kappa_b)), its
    off-diagonal part 0.3 / sqrt(n) N(0, 1)."""
    rng = np.random.default_rng([int(seed), int(n), 29])
    L0 = np.tril(rng.normal(0.0, 0.3 / np.sqrt(n), (n, n)), -1)
    _hard_diagonal(L0, kappa_b, seed)
    return _unit_diagonal(_gram(L0))


def plan_envelope(heights):
    """`last` of the block envelope `heights` describes (active block rows below the diagonal per block column; one more block
    column, the one with the right-hand side, follows), as test_factorisation_plans_vs_numpy builds it."""
    from test_gpu_parity import _envelope_last
    nblk = len(heights) + 1
    first_col = np.arange(nblk)
    for c, h in enumerate(heights):
        for r in range(c, min(nblk - 1, c + h + 1)):
            first_col[r] = min(first_col[r], c)
    return _envelope_last(first_col)


def _banded_factor(n, last, rng):
    """L0 confined to the block envelope `last` (the rows _banded_spd fills), the off-diagonal blocks of column c scaled by
    0.3 / sqrt(128 (h_c + 1)); diagonal blocks left to _hard_diagonal."""
    nblk = len(last)
    L0 = np.zeros((n, n))
    for c in range(nblk):
        c0, c1 = BLOCK * c, min(n, BLOCK * (c + 1))
        lr = min(int(last[c]), nblk - 2)
        r1 = min(n, BLOCK * (lr + 1))
        if c0 < n and r1 > c1:
            L0[c1:r1, c0:c1] = rng.normal(0.0, 0.3 / np.sqrt(BLOCK * (lr - c + 1)), (r1 - c1, c1 - c0))
    return L0


def banded_hard(heights, off_grid, kappa_b, seed):
    """hard_blocks' construction with L0 confined to the block envelope of `heights`; A = L0 L0^T has the same envelope.
    Returns (A, last)."""
    last = plan_envelope(heights)
    n = BLOCK * len(last) - off_grid
    rng = np.random.default_rng([int(seed), n, 31])
    L0 = _hard_diagonal(_banded_factor(n, last, rng), kappa_b, seed)
    return _unit_diagonal(_gram(L0)), last


def bordered_hard(heights, border_rows, reach_blocks, kappa_b, seed, off_grid=70):
    """banded_hard followed by a border with the shapes of test_gpu_parity._bordered_spd: border row group g couples with 37
    columns of block reach_blocks[g] of the band and with 30 columns late in the band; the border is dense among itself.
    Returns (A, border_begin)."""
    last = plan_envelope(heights)
    nb = BLOCK * len(last) - off_grid
    m = int(sum(border_rows))
    n = nb + m
    rng = np.random.default_rng([int(seed), n, 37])
    L0 = np.zeros((n, n))
    L0[:nb, :nb] = _banded_factor(nb, last, rng)
    s = 0.3 / np.sqrt(37 + 30 + m)
    row = nb
    for rows, blk in zip(border_rows, reach_blocks):
        c0 = min(nb - 40, BLOCK * blk + 11)
        L0[row:row + rows, c0:c0 + 37] = rng.normal(0.0, s, (rows, 37))
        L0[row:row + rows, nb - 90:nb - 60] = rng.normal(0.0, s, (rows, 30))
        row += rows
    L0[nb:, nb:] = np.tril(rng.normal(0.0, s, (m, m)), -1)
    _hard_diagonal(L0, kappa_b, seed)
    return _unit_diagonal(_gram(L0)), nb


def scalar_band_hard(n, w, kappa_b, seed):
    """A scalar band of half-width w (test_multiway_dissection_with_separators_narrower_than_a_block's shape) with hard
    diagonal blocks."""
    rng = np.random.default_rng([int(seed), n, 41])
    L0 = np.zeros((n, n))
    for d in range(1, w + 1):
        L0[np.arange(d, n), np.arange(0, n - d)] = rng.normal(0.0, 0.3 / np.sqrt(w), n - d)
    band = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) <= w
    G = np.zeros((n, n))
    _hard_diagonal(G, kappa_b, seed)
    L0 = np.where(band & (G != 0), G, L0)      # the hard diagonal blocks, cut to the band
    return _unit_diagonal(_gram(L0))


def plan_case(shape, kappa_b=None, off_grid=70):
    from test_gpu_parity import _PLAN_SHAPES
    kb = KAPPA_B[("banded_hard", shape)] if kappa_b is None else kappa_b
    return banded_hard(_PLAN_SHAPES[shape], off_grid, kb, seed=len(shape))


def bordered_case(name, kappa_b=None):
    from test_gpu_parity import _PLAN_SHAPES
    shape, border_rows, reach_blocks = BORDERED_SHAPES[name]
    kb = KAPPA_B[("bordered_hard", name)] if kappa_b is None else kappa_b
    return bordered_hard(_PLAN_SHAPES[shape], border_rows, reach_blocks, kb, seed=len(name))


def right_hand_sides(A, seed):
    """(name, b): b random, and b = A s with s = +-1 (formed in long double, rounded once)."""
    rng = np.random.default_rng([int(seed), A.shape[0], 43])
    b0 = rng.normal(size=A.shape[0])
    s = rng.integers(0, 2, A.shape[0]) * 2.0 - 1.0
    return [("random", b0), ("A.sign", np.asarray(_matvec(A, s), dtype=np.float64))]


# ---------------------------------------------------------------------------------------------------------------------
# envelopes: first_block[rb] = the first block column in which block row rb is active
# ---------------------------------------------------------------------------------------------------------------------
def envelope_dense(n):
    return np.zeros((n + BLOCK - 1) // BLOCK, dtype=np.int64)


def envelope_from_last(last, n):
    """Block row r is active in block column c when r <= last[c]; the block row behind the band (the right-hand side's) holds
    nothing of the matrix but its diagonal block."""
    nb = (n + BLOCK - 1) // BLOCK
    last = np.asarray(last, dtype=np.int64)[:nb]
    fb = np.arange(nb, dtype=np.int64)
    for r in range(nb):
        reach = np.nonzero(last[:r + 1] >= r)[0]
        fb[r] = reach[0] if len(reach) else r
    return fb


def envelope_from_matrix(A, border_begin=None):
    """From the non-zero blocks of tril(A); from border_begin on a row, once reached, stays active, and so does every row
    behind it (the bordered envelope of chol_envelope.hpp)."""
    n = A.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    fb = np.arange(nb, dtype=np.int64)
    low = np.tril(A)
    for r in range(nb):
        cols = np.nonzero(np.any(low[BLOCK * r:BLOCK * (r + 1)] != 0, axis=0))[0]
        fb[r] = cols[0] // BLOCK if len(cols) else r
    if border_begin is not None:
        for r in range(border_begin // BLOCK + 1, nb):
            fb[r] = min(fb[r], fb[r - 1])
    return fb


def regime_rows(heights):
    """The block rows just before and after each change of regime of the plan: block columns where the height jumps by more
    than one block or crosses one of PLAN_THRESHOLDS."""
    rows = set()
    for c in range(1, len(heights)):
        a, b = heights[c - 1], heights[c]
        if abs(a - b) > 1 or any((a <= t) != (b <= t) for t in PLAN_THRESHOLDS):
            rows.update((c - 1, c))
    return sorted(rows)


def max_m(envelope, n):
    """The largest m_ij of the envelope."""
    fb = np.asarray(envelope, dtype=np.int64)
    return int(BLOCK * np.max(np.arange(len(fb)) - fb + 1) + BLOCK + 1)


# ---------------------------------------------------------------------------------------------------------------------
# extended-precision products
# ---------------------------------------------------------------------------------------------------------------------
_SLICES = 6
_KCHUNK = 1024


def _slices(X, count=_SLICES):
    """X = sum of the returned arrays, exactly: slice s (1-based) a multiple of 2^-20s below 2^-20(s-1), the last the rest."""
    out, R = [], np.array(X, dtype=np.float64)
    for s in range(1, count):
        H = np.rint(R * 2.0 ** (20 * s))
        H *= 2.0 ** (-20 * s)
        out.append(H)
        R -= H
    out.append(R)
    return out


def _row_scales(Xc):
    """Per row the power of two that brings the row's largest magnitude below 1, and its inverse."""
    _, e = np.frexp(np.max(np.abs(Xc), axis=1))
    e = np.clip(e, -900, 900)
    return np.ldexp(1.0, -e), np.ldexp(1.0, e)


def _exact_nt(X, Y, levels=_SLICES):
    """(X Y^T in long double, a bound on what was left out), X [p, K] and Y [q, K] doubles.  Per chunk of 1024 columns every
    row is scaled by a power of two to magnitude below 1 and cut into `levels` slices; a product of two slices over 1024
    columns is an integer below 2^50 times the grid, and the sum of the at most six products of one level stays below 2^52:
    exact in double.  The levels are added up in long double and the scaling undone.  Slice pairs beyond 2^-20 levels of the
    scaled entries are left out; the second result bounds them (and the rounding of the products with the last slice, 2^-53
    of that) entry by entry."""
    out = np.zeros((X.shape[0], Y.shape[0]), dtype=LD)
    left = np.zeros((X.shape[0], Y.shape[0]))
    dropped = 2.0 ** (3 - 20 * levels)
    for a in range(0, X.shape[1], _KCHUNK):
        Xc, Yc = X[:, a:a + _KCHUNK], Y[:, a:a + _KCHUNK]
        sx, ux = _row_scales(Xc)
        sy, uy = _row_scales(Yc)
        Xs = _slices(Xc * sx[:, None], levels)
        Ys = Xs if Y is X else _slices(Yc * sy[:, None], levels)
        acc = np.zeros(out.shape, dtype=LD)
        for level in range(levels - 1, -1, -1):
            G = Xs[level] @ Ys[0].T
            for p in range(level):
                G += Xs[p] @ Ys[level - p].T
            acc += G
        out += acc * ux.astype(LD)[:, None] * uy.astype(LD)[None, :]
        left += (Xc.shape[1] * dropped) * np.outer(ux, uy)
    return out, left


def _matvec(A, x):
    """A x in long double, in chunks of rows."""
    xl = np.asarray(x, dtype=LD)
    out = np.empty(A.shape[0], dtype=LD)
    for a in range(0, A.shape[0], 256):
        out[a:a + 256] = A[a:a + 256].astype(LD) @ xl
    return out


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def _entry_bound(i, j, fb):
    """(gamma_{m_ij}, whether (i, j) lies in the lower envelope): the dot product of entry (i, j) runs over the block columns from
    the later of the two rows' first ones up to j's."""
    ib, jb = i // BLOCK, j // BLOCK
    m = BLOCK * (jb - np.maximum(fb[ib], fb[jb]) + 1) + BLOCK + 1
    return gamma(m), (i >= j) & (jb >= fb[ib])


def _quotient(R, bound):
    """|R| / bound, 0 where both vanish, inf where only the bound does."""
    R = np.abs(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = R / bound
    q = np.where(bound > 0, q, np.where(R > 0, LD(np.inf), LD(0)))
    return np.where(np.isnan(q), LD(np.inf), q)


def _block_ratio(A, Lt, I, J, fb):
    """The worst quotient over rows I x columns J (index arrays, ascending) of the lower envelope, and where."""
    k0 = min(BLOCK * int(np.min(fb[I // BLOCK])), int(J[0]))
    k1 = int(J[-1]) + 1
    X = Lt[I, k0:k1]
    Y = X if I is J else Lt[J, k0:k1]
    D = np.abs(X) @ np.abs(Y).T
    g, valid = _entry_bound(I[:, None], J[None, :], fb)
    bound = g * D
    for levels in (4, _SLICES):         # four slices do where the rows of L do not decay along the block row; six elsewhere
        P, left = _exact_nt(X, Y, levels)
        if not np.any(valid & (left > 1e-3 * bound) & (D > 0)):
            break
    R = A[np.ix_(I, J)].astype(LD) - P
    # entries whose bound is not far above what _exact_nt left out: plain long-double dot products
    ra, rb = np.nonzero(valid & (left > 1e-3 * bound) & (D > 0))
    for c in range(0, len(ra), 256):
        a, b = ra[c:c + 256], rb[c:c + 256]
        R[a, b] = A[I[a], J[b]].astype(LD) - (X[a].astype(LD) * Y[b].astype(LD)).sum(axis=1)
    q = np.where(valid, _quotient(R, bound), LD(0))
    w = np.unravel_index(np.argmax(q), q.shape)
    return float(q[w]), (int(I[w[0]]), int(J[w[1]]))


def _lattice(r, n, fb, rng):
    """Of block row r: SAMPLE_ROWS random rows of every 32-row tile row, SAMPLE_COLS random columns of every 32-column tile
    column of its envelope before the diagonal block: SAMPLE_ROWS * SAMPLE_COLS entries of every tile."""
    i0, i1 = BLOCK * r, min(n, BLOCK * (r + 1))
    I = np.concatenate([t + np.sort(rng.choice(min(TILE, i1 - t), min(SAMPLE_ROWS, i1 - t), replace=False)) for t in range(i0, i1, TILE)])
    cols = [t + np.sort(rng.choice(TILE, SAMPLE_COLS, replace=False)) for t in range(BLOCK * int(fb[r]), i0, TILE)]
    return I, (np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64))


def outside_envelope(L, fb):
    """The largest magnitude of L above the diagonal or before its row's envelope (NaN counts as inf)."""
    worst = np.abs(np.triu(L, 1)).max() if L.shape[0] > 1 else 0.0
    for r in range(len(fb)):
        if fb[r] > 0:
            worst = max(worst, np.abs(L[BLOCK * r:BLOCK * (r + 1), :BLOCK * fb[r]]).max())
    return float("inf") if np.isnan(worst) else float(worst)


def factor_ratio(A, L, envelope=None, rows=(), sampled=None, seed=0, where=False):
    """max_ij |A - L L^T|_ij / (gamma_{m_ij} (|L||L^T|)_ij) over the lower envelope.  envelope: first block column per block row
    (None: dense); a non-zero of L outside it gives inf.  Dense up to n = DENSE_MAX.  Above that (or with sampled=True):
    every entry of every diagonal 128-block, every entry of the block rows `rows` (regime_rows), and of every 32 x 32 tile
    of the envelope, whether A has a non-zero there or only L, the SAMPLE_ROWS x SAMPLE_COLS entries of a random lattice
    (_lattice: 16 per tile, drawn per block row from `seed`).  where=True: (ratio, (i, j))."""
    _require_long_double()
    n = A.shape[0]
    L = np.asarray(L, dtype=np.float64)
    fb = envelope_dense(n) if envelope is None else np.asarray(envelope, dtype=np.int64)
    if not np.all(np.isfinite(L)) or outside_envelope(L, fb) > 0:
        return (float("inf"), None) if where else float("inf")
    Lt = np.tril(L)
    if sampled is None:
        sampled = n > DENSE_MAX
    found = []
    if not sampled:
        for i0 in range(0, n, 2 * BLOCK):
            i1 = min(n, i0 + 2 * BLOCK)
            found.append(_block_ratio(A, Lt, np.arange(i0, i1), np.arange(0, i1), fb))
    else:
        rng = np.random.default_rng([int(seed), n, 47])
        for r in range(len(fb)):
            i0, i1 = BLOCK * r, min(n, BLOCK * (r + 1))
            if r in rows:
                found.append(_block_ratio(A, Lt, np.arange(i0, i1), np.arange(BLOCK * int(fb[r]), i1), fb))
                continue
            D = np.arange(i0, i1)
            found.append(_block_ratio(A, Lt, D, D, fb))
            I, J = _lattice(r, n, fb, rng)
            if len(J):
                found.append(_block_ratio(A, Lt, I, J, fb))
    best = max(found, key=lambda t: t[0])
    return best if where else best[0]


def residual(A, x, b):
    """|A x - b| per row, long double."""
    return np.abs(_matvec(A, x) - np.asarray(b, dtype=LD))


def solve_metrics(A, x, b, m):
    """(solve_row_ratio, eta) from one residual."""
    _require_long_double()
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        return float("inf"), float("inf")
    r = np.max(residual(A, x, b))
    na = np.max(np.abs(A).sum(axis=1))
    return (float(r / (gamma(3 * m + 1) * np.sum(np.abs(x.astype(LD))))),
            float(r / (LD(na) * np.max(np.abs(x)) + np.max(np.abs(b)))))


def solve_row_ratio(A, x, b, m):
    """max_i |A x - b|_i / (gamma_{3m+1} ||x||_1) for a unit-diagonal A; m the largest m_ij (max_m)."""
    return solve_metrics(A, x, b, m)[0]


def eta(A, x, b):
    """The normwise backward error ||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf) (reported, not asserted)."""
    return solve_metrics(A, x, b, 1)[1]


def cond_estimate(A, L=None):
    """cond_2(A): eigvalsh up to n = 1500; above, Lanczos for the largest eigenvalue of A and of A^-1 through the factor L."""
    n = A.shape[0]
    if n <= 1500:
        w = np.linalg.eigvalsh(A)
        return float(w[-1] / w[0]) if w[0] > 0 else float("inf")
    if L is None:
        L = np.linalg.cholesky(A)
    v0 = np.random.default_rng(n).normal(size=n)
    hi = spla.eigsh(spla.LinearOperator((n, n), matvec=lambda v: A @ v, dtype=np.float64), k=1, which="LA", v0=v0, tol=1e-2)[0][0]
    Lf = np.asfortranarray(L)   # (once, not at every solve)
    inv = spla.LinearOperator((n, n), matvec=lambda v: sla.cho_solve((Lf, True), v, check_finite=False), dtype=np.float64)
    lo = 1.0 / spla.eigsh(inv, k=1, which="LA", v0=v0, tol=1e-2)[0][0]
    return float(hi / lo)


# ---------------------------------------------------------------------------------------------------------------------
# the two emulations, both in double
# ---------------------------------------------------------------------------------------------------------------------
class Lapack:
    """np.linalg.cholesky with cho_solve.  Raises np.linalg.LinAlgError when A is not positive definite."""

    def __init__(self, A):
        self.L = np.linalg.cholesky(A)

    def solve(self, b):
        return sla.cho_solve((self.L, True), b, check_finite=False)


class BlockedExplicitInverse:
    """A right-looking blocked Cholesky at block size 128 whose panel is A21 inv(L11)^T and whose solves multiply with the
    inverse diagonal blocks: the device's algorithm in outline.  envelope (first block column per block row) confines the
    trailing updates to the active rows.  defect: None or one of

        ("skip_tile", jb, i, j)     the 32 x 32 tile that holds entry (i, j) left out of block column jb's trailing update
        ("skip_panel", jb, cb)      block column jb's trailing update not applied to block column cb
        ("float32_L",)              L rounded to float32
        ("float32_inv", jb)         inv(L11) of block column jb rounded to float32
        ("drop_term", i, j, k)      the term L_ik L_jk left out of entry (i, j)
        ("transpose_tile", jb, i)   the 32 x 32 tile of block column jb's panel at row i, first 32 columns, transposed
    """

    def __init__(self, A, envelope=None, defect=None):
        n = A.shape[0]
        fb = envelope_dense(n) if envelope is None else np.asarray(envelope, dtype=np.int64)
        kind = defect[0] if defect else None
        S = np.array(A, dtype=np.float64)
        L = np.zeros((n, n))
        self.W = []
        rb_of = np.arange(n) // BLOCK
        for jb in range(len(fb)):
            c0, c1 = BLOCK * jb, min(n, BLOCK * (jb + 1))
            L11 = np.linalg.cholesky(S[c0:c1, c0:c1])
            W = sla.solve_triangular(L11, np.eye(c1 - c0), lower=True, check_finite=False)
            if kind == "float32_inv" and defect[1] == jb:
                W = W.astype(np.float32).astype(np.float64)
            L[c0:c1, c0:c1] = L11
            self.W.append(W)
            act = np.nonzero((np.arange(n) >= c1) & (fb[rb_of] <= jb))[0]
            if len(act) == 0:
                continue
            P = S[act, c0:c1] @ W.T
            if kind == "transpose_tile" and defect[1] == jb:
                t = int(np.searchsorted(act, defect[2]))
                P[t:t + TILE, :TILE] = P[t:t + TILE, :TILE].T.copy()
            L[act, c0:c1] = P
            U = P @ P.T
            if kind == "skip_tile" and defect[1] == jb:
                ti = np.nonzero(act // TILE == defect[2] // TILE)[0]
                tj = np.nonzero(act // TILE == defect[3] // TILE)[0]
                U[np.ix_(ti, tj)] = 0.0
                U[np.ix_(tj, ti)] = 0.0
            if kind == "skip_panel" and defect[1] == jb:
                cc = np.nonzero(act // BLOCK == defect[2])[0]
                U[:, cc] = 0.0
                U[cc, :] = 0.0
            if kind == "drop_term" and c0 <= defect[3] < c1:
                i, j, k = np.searchsorted(act, defect[1]), np.searchsorted(act, defect[2]), defect[3] - c0
                U[i, j] -= P[i, k] * P[j, k]
                if i != j:
                    U[j, i] -= P[i, k] * P[j, k]
            cut = np.nonzero(np.diff(act) > 1)[0] + 1          # act is a few contiguous runs (the band, the border)
            runs = list(zip(np.r_[0, cut], np.r_[cut, len(act)]))
            for ka, (a0, a1) in enumerate(runs):                # the lower part is all anything reads
                for b0, b1 in runs[:ka + 1]:
                    S[act[a0]:act[a1 - 1] + 1, act[b0]:act[b1 - 1] + 1] -= U[a0:a1, b0:b1]
        if kind == "float32_L":
            L = L.astype(np.float32).astype(np.float64)
        self.L = L
        self.fb = fb

    def solve(self, b):
        n = self.L.shape[0]
        L = self.L
        z = np.array(b, dtype=np.float64)
        nb = len(self.W)
        for jb in range(nb):
            c0, c1 = BLOCK * jb, min(n, BLOCK * (jb + 1))
            z[c0:c1] = self.W[jb] @ z[c0:c1]
            z[c1:] -= L[c1:, c0:c1] @ z[c0:c1]
        for jb in range(nb - 1, -1, -1):
            c0, c1 = BLOCK * jb, min(n, BLOCK * (jb + 1))
            z[c0:c1] = self.W[jb].T @ (z[c0:c1] - L[c1:, c0:c1].T @ z[c1:])
        return z


def blocked_explicit_inverse(A, envelope=None, defect=None):
    return BlockedExplicitInverse(A, envelope, defect)


# ---------------------------------------------------------------------------------------------------------------------
# matrices that are not positive definite
# ---------------------------------------------------------------------------------------------------------------------
def indefinite_in_block(A, L, block, shift=None, delta=1e-6):
    """A with one negative eigenvalue whose defect a factorisation first meets in 128-block `block`, all diagonal entries 1.

    The Schur complement that block's factorisation starts from is S = L_bb L_bb^T (L: LAPACK's factor of A).  With (mu, v) its
    smallest eigenpair, v padded with zeros to the whole matrix, A - (mu + delta) v v^T has the Schur complement
    S - (mu + delta) v v^T there, whose smallest eigenvalue is -delta: far above n u, so every correct factorisation fails in
    that block and none before it.  The unit diagonal is then restored by a diagonal congruence, which keeps the signs of all
    leading minors.  (An eigenvector of A itself, cut to one block, has a Rayleigh quotient far above lambda_min for these
    families: subtracting lambda_min + delta along it leaves A positive definite.)  shift: what to subtract instead of
    mu + delta, as a multiple of 1 / (v^T A^-1 v) <= mu, below which A - a v v^T stays positive definite (0.5: a neighbour)."""
    n = A.shape[0]
    c0, c1 = BLOCK * block, min(n, BLOCK * (block + 1))
    Lbb = L[c0:c1, c0:c1]
    w, V = np.linalg.eigh(Lbb @ Lbb.T)
    v = np.zeros(n)
    v[c0:c1] = V[:, 0]
    amount = w[0] + delta if shift is None else shift / float(v @ sla.cho_solve((L, True), v, check_finite=False))
    return _unit_diagonal(A - amount * np.outer(v, v))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_chol_check_cpu.py and tests/test_gpu_chol_check.py
# ---------------------------------------------------------------------------------------------------------------------
DENSE_CASES = ([("graded", n, kappa) for n in (5, 127, 128, 129, 257, 700) for kappa in (1e4, 1e8, 1e12)]
               + [("hard_blocks", n) for n in (128, 129, 257, 700)])
PLAN_CASES = [("plan", s) for s in ("band", "odd-resident-run", "resident-then-wide-then-resident", "two-wide-parts")]
BORDERED_CASES = [("bordered", s) for s in sorted(BORDERED_SHAPES)]
SCALAR_BAND_CASE = ("scalar_band", 40)
LARGEST_CASE = ("plan", "two-wide-parts")
# (case, the 128-block the defect sits in): the first block, a middle block, the last partial block, the border of a bordered system
NPD_CASES = [(("graded", 700, 1e4), 0), (("hard_blocks", 700), 3), (("graded", 700, 1e8), 5), (("bordered", "three-revisits"), 44)]
NAN_CASE = (("graded", 257, 1e4), (200, 3))


def case_matrix(cid, kappa_b):
    """The matrix of a hard case at another kappa_b than the one it carries."""
    kind = cid[0]
    if kind == "hard_blocks":
        return hard_blocks(cid[1], kappa_b, seed=cid[1])
    if kind == "plan":
        return plan_case(cid[1], kappa_b)[0]
    if kind == "bordered":
        return bordered_case(cid[1], kappa_b)[0]
    if kind == "scalar_band":
        return scalar_band_hard(BLOCK * 30 - 17, cid[1], kappa_b, seed=cid[1])
    raise ValueError(cid)


def case_id(cid):
    return "-".join("%g" % v if isinstance(v, float) else str(v) for v in cid)


class Case:
    """A: the matrix (full, symmetric); envelope: first block column per block row; rows: block rows the sampled factor_ratio
    reads whole; m: the largest m_ij; kappa_b: of the hard families (None for graded); last / border_begin: what the device's
    entry point is told about the envelope."""

    def __init__(self, cid):
        from test_gpu_parity import _PLAN_SHAPES
        self.cid, self.name = cid, case_id(cid)
        self.last = self.border_begin = self.kappa_b = None
        self.rows = ()
        kind = cid[0]
        if kind == "graded":
            self.A = graded(cid[1], cid[2], seed=cid[1])
            self.envelope = envelope_dense(cid[1])
        elif kind == "hard_blocks":
            self.kappa_b = KAPPA_B[cid] if len(cid) == 2 else cid[2]
            self.A = hard_blocks(cid[1], self.kappa_b, seed=cid[1])
            self.envelope = envelope_dense(cid[1])
        elif kind == "plan":
            self.kappa_b = KAPPA_B[("banded_hard", cid[1])] if len(cid) == 2 else cid[2]
            self.heights = _PLAN_SHAPES[cid[1]]
            self.A, self.last = plan_case(cid[1], self.kappa_b)
            self.envelope = envelope_from_last(self.last, self.A.shape[0])
            self.rows = tuple(regime_rows(self.heights))
        elif kind == "bordered":
            self.kappa_b = KAPPA_B[("bordered_hard", cid[1])] if len(cid) == 2 else cid[2]
            self.heights = _PLAN_SHAPES[BORDERED_SHAPES[cid[1]][0]]
            self.A, self.border_begin = bordered_case(cid[1], self.kappa_b)
            self.envelope = envelope_from_matrix(self.A, self.border_begin)
            self.rows = tuple(regime_rows(self.heights)) + (self.border_begin // BLOCK, min(self.border_begin // BLOCK + 1, len(self.envelope) - 1))
        elif kind == "scalar_band":
            self.kappa_b = KAPPA_B[cid] if len(cid) == 2 else cid[2]
            self.A = scalar_band_hard(BLOCK * 30 - 17, cid[1], self.kappa_b, seed=cid[1])
            self.envelope = envelope_from_matrix(self.A)
        else:
            raise ValueError(cid)
        self.n = self.A.shape[0]
        self.m = max_m(self.envelope, self.n)
        self.rhs = right_hand_sides(self.A, seed=self.n)

    def measure(self, L, xs):
        """{"factor_ratio", "where", "solve_row_ratio": [per right-hand side], "eta": [...]} of a factor (or None) and the solutions
        of self.rhs."""
        out = {}
        if L is not None:
            out["factor_ratio"], out["where"] = factor_ratio(self.A, L, self.envelope, rows=self.rows, where=True)
        both = [solve_metrics(self.A, x, b, self.m) for x, (_, b) in zip(xs, self.rhs)]
        out["solve_row_ratio"] = [t[0] for t in both]
        out["eta"] = [t[1] for t in both]
        return out


def record(case, who, plan, measured):
    """With CHOL_CHECK_LOG set, appends one JSON line: case, who (lapack | emulation | device), plan, the ratios, kappa_b."""
    import json
    import os
    path = os.environ.get("CHOL_CHECK_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case.name, "n": case.n, "kappa_b": case.kappa_b, "who": who, "plan": plan,
                                "factor_ratio": measured.get("factor_ratio"), "where": measured.get("where"),
                                "solve_row_ratio": measured["solve_row_ratio"], "eta": measured["eta"]}) + "\n")
