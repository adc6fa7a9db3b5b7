"""A numpy restatement of sk_covariance_compute (ceres::Covariance by the normal-equations Cholesky), in float64 and in long double.

Written independently of the plan of skeres_amd/csrc/covariance_plan.cpp: the Jacobian comes from the models of tests/step_check.py
(the oracle's functors, tests/tape_reference.py for recorded ones) as tests/cgnr_cases.py builds them, the normal matrix is summed
residual block by residual block into a dense array, and the factorisation and the triangular solves are column loops of this file
(numpy's linalg has no long double).

    J        the model's Jacobian, loss-corrected, restricted to the TANGENT columns of the blocks that move (a subset block: its
             free coordinates; a quaternion block: the model's three tangent columns; a constant block: none);
    H        J^T J;  d = diag(H)^(-1/2);  H~ = D H D;  H~ = L L^T;  L X = Sel (the columns of the requested blocks);
    tangent  C_ab = d_a d_b (X^T X)_ab;   ambient  P_a C_ab P_b^T with P = dPlus/ddelta at x (oracle.parameterization_jacobian);
    a constant block has covariance zero with everything; a diagonal entry of H that is exactly 0 raises RankDeficient.

A case describes its parameter blocks as Block(size, tangent, model_cols, constant, lift): model_cols are the block's tangent
columns in the model's column space, lift is None (identity), ("subset", held) or ("quaternion",)."""
import collections

import numpy as np

import oracle

LD = np.longdouble
U = 2.0 ** -53

Block = collections.namedtuple("Block", "size tangent model_cols constant lift")


class RankDeficient(Exception):
    def __init__(self, block, coordinate):
        Exception.__init__(self, "block %d coordinate %d" % (block, coordinate))
        self.block, self.coordinate = block, coordinate


def columns(blocks):
    """(first tangent column per block, or -1; N) over the blocks that move, in block order."""
    first, n = [], 0
    for b in blocks:
        moving = not b.constant and b.tangent > 0
        first.append(n if moving else -1)
        n += b.tangent if moving else 0
    return first, n


def _column_map(blocks, model_n):
    """model column -> tangent column (-1: not a column of H)."""
    first, _ = columns(blocks)
    out = np.full(model_n, -1, dtype=np.int64)
    for b, f in zip(blocks, first):
        if f >= 0:
            out[np.asarray(b.model_cols, dtype=np.int64)] = f + np.arange(b.tangent)
    return out


def normal_matrix(model, x, blocks, T, defect=None):
    """(H [N, N] in dtype T, the number of unordered pairs of moving blocks that share a residual block).  defect(J terms of one
    residual block as [(J [k, w], tangent columns [w])], index of the residual block) may return a replacement (planted defects)."""
    first, n = columns(blocks)
    cmap = _column_map(blocks, model.n)
    owner = np.full(n, -1, dtype=np.int64)
    for i, (b, f) in enumerate(zip(blocks, first)):
        if f >= 0:
            owner[f:f + b.tangent] = i
    H = np.zeros((n, n), dtype=T)
    pairs = set()
    index = 0
    for r, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        nb = r.shape[0]
        cols = [cmap[t_first[:, None] + np.arange(J.shape[2])] for J, t_first in terms]
        for i in range(nb):
            mine = []
            for (J, _), c in zip(terms, cols):
                keep = c[i] >= 0
                if np.any(keep):
                    mine.append((J[i][:, keep].astype(T), c[i][keep]))
            if defect is not None:
                mine = defect(mine, index)
            for Ja, ca in mine:
                for Jb, cb in mine:
                    H[np.ix_(ca, cb)] += Ja.T @ Jb
                    for p in set(owner[ca]):
                        for q in set(owner[cb]):
                            pairs.add((max(p, q), min(p, q)))
            index += 1
    return H, len(pairs)


def normal_matrix_from_crs(jac, blocks):
    """H in long double from a CRSMatrix of Problem::Evaluate whose columns are the blocks in block order, each with its tangent size
    (a constant block keeps its columns there and has no entries)."""
    first, n = columns(blocks)
    emap, e = [], 0
    for b, f in zip(blocks, first):
        emap += list(f + np.arange(b.tangent)) if f >= 0 else [-1] * b.tangent
        e += b.tangent
    assert e == jac.num_cols, (e, jac.num_cols)
    emap = np.asarray(emap, dtype=np.int64)
    H = np.zeros((n, n), dtype=LD)
    for r in range(jac.num_rows):
        a, z = jac.rows[r], jac.rows[r + 1]
        c = emap[jac.cols[a:z]]
        assert np.all(c >= 0)
        v = jac.values[a:z].astype(LD)
        H[np.ix_(c, c)] += np.outer(v, v)
    return H


def cholesky(A):
    """Lower factor of A by a column loop, in A's dtype; None where a pivot is not positive."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0 or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward(L, B):
    """X with L X = B, row by row."""
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def lift_matrix(block, xb, T):
    """P = dPlus/ddelta at xb: size x tangent."""
    if block.lift is None:
        return np.eye(block.size, dtype=T)
    if block.lift[0] == "subset":
        P = np.zeros((block.size, block.tangent), dtype=T)
        free = [i for i in range(block.size) if i not in set(block.lift[1])]
        for c, i in enumerate(free):
            P[i, c] = 1
        return P
    return np.asarray(oracle.parameterization_jacobian(block.lift, np.asarray(xb, dtype=np.float64)), dtype=T).reshape(block.size, block.tangent)


def selected_inverse(H, blocks, selected, T, scale=True):
    """(C [k, k]: the block of H^-1 over the columns of the selected moving blocks, in the order given; offsets of the blocks in it;
    min L_jj^2 / max L_jj^2 of the scaled matrix's factor).  scale False: the planted defect "a missing d_i d_j"."""
    first, n = columns(blocks)
    H = H.astype(T)
    diag = np.diag(H).copy()
    zero = np.flatnonzero(diag == 0)
    if len(zero):
        j = int(zero[0])
        b = max(i for i, f in enumerate(first) if 0 <= f <= j)
        raise RankDeficient(b, j - first[b])
    d = 1 / np.sqrt(diag)
    Hs = H * d[:, None] * d[None, :]
    L = cholesky(Hs)
    if L is None:
        raise RankDeficient(-1, -1)
    sel, off = [], [0]
    for b in selected:
        sel += list(first[b] + np.arange(blocks[b].tangent))
        off.append(len(sel))
    sel = np.asarray(sel, dtype=np.int64)
    E = np.zeros((n, len(sel)), dtype=T)
    E[sel, np.arange(len(sel))] = 1
    X = forward(L, E)
    C = X.T @ X
    if scale:
        C = C * d[sel][:, None] * d[sel][None, :]
    piv = np.diag(L) ** 2
    return C, off, float(piv.min() / piv.max()), Hs


def covariance(H, blocks, x, offsets, pairs, T, scale=True):
    """The requested blocks: {"tangent": {(a, b): array}, "ambient": {...}, "ratio", "kappa", "N", "k"}; pairs are block indices,
    answered in the order given ((b, a) is (a, b) transposed); the diagonal blocks of every named block are included."""
    named = []
    for a, b in pairs:
        for q in (a, b):
            if q not in named:
                named.append(q)
    moving = [q for q in named if not blocks[q].constant and blocks[q].tangent > 0]
    C, off, ratio, Hs = selected_inverse(H, blocks, moving, T, scale)
    pos = {q: i for i, q in enumerate(moving)}
    out = {"tangent": {}, "ambient": {}, "ratio": ratio, "N": H.shape[0], "k": off[-1],
           "kappa": float(np.linalg.cond(Hs.astype(np.float64)))}
    want = list(pairs) + [(q, q) for q in named]
    for a, b in want:
        A, B = blocks[a], blocks[b]
        if a in pos and b in pos:
            t = C[off[pos[a]]:off[pos[a] + 1], off[pos[b]]:off[pos[b] + 1]]
            Pa = lift_matrix(A, x[offsets[a]:offsets[a] + A.size], T)
            Pb = lift_matrix(B, x[offsets[b]:offsets[b] + B.size], T)
            amb = Pa @ t @ Pb.T
        else:
            t, amb = np.zeros((A.tangent, B.tangent), dtype=T), np.zeros((A.size, B.size), dtype=T)
        out["tangent"][(a, b)] = t
        out["ambient"][(a, b)] = amb
    return out


def metric(got, ref, ref_aa, ref_bb):
    """max |got - ref| over the block / sqrt(max diag C_aa . max diag C_bb); inf where the shapes differ."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return float("inf")
    scale = np.sqrt(LD(np.max(np.diag(ref_aa))) * LD(np.max(np.diag(ref_bb))))
    if scale == 0:
        return 0.0 if not np.any(got != 0) else float("inf")
    return float(np.max(np.abs(got.astype(LD) - ref.astype(LD))) / scale)


def deviation(got, ref, pairs, spaces=("tangent", "ambient")):
    """The largest metric over the pairs and spaces: got and ref as covariance() returns them (ref supplies the scales)."""
    worst = 0.0
    for space in spaces:
        for a, b in pairs:
            worst = max(worst, metric(got[space][(a, b)], ref[space][(a, b)], ref[space][(a, a)], ref[space][(b, b)]))
    return worst
