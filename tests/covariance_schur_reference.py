"""A numpy restatement of sk_covariance_compute WITH THE SCHUR ELIMINATION (sk_covariance_options_set_schur_elimination), in float64
and in long double, written independently of the plan of skeres_amd/csrc/covariance_plan.cpp.

The Jacobian is a list of (row, tangent column, value) triples — from the models of tests/step_check.py (model_coo) or from the
CRSMatrix that sk_problem_evaluate returns (crs_coo); no dense N x N matrix is ever formed, so a problem of 33 054 columns is a case.

    E        the greedy independent set: two moving blocks are neighbours when a row of J stores both; the blocks are visited in
             ascending order of (number of distinct neighbours, block index), and a block joins E when no neighbour is in E yet.  A
             row therefore stores at most one e-block: J = [J_F | J_E] with J_F dense [rows, n_F] and J_E one short vector per row;
    H        U = J_F^T J_F,  V_e = sum over the rows of e,  W_e = J_F^T J_e;  d = diag(H)^(-1/2) over all columns;
    e-blocks V~_e = L_e L_e^T and L_e^-1 by column loops batched over the blocks,  X_e = L_e^-1 W~_e^T  [size(e), n_F];
    S~       U~ - sum_e X_e^T X_e = L_S L_S^T (covariance_reference.cholesky, a column loop);  C~_FF = S~^-1 over the selected columns;
    back     C~_Fe = -C~_FF X_e^T L_e^-1;   C~_ee' = delta_ee' L_e^-T L_e^-1 + L_e^-T (X_e C~_FF X_e'^T) L_e'^-1;
    tangent  C_ab = d_a d_b C~_ab;  ambient  P_a C_ab P_b^T as covariance_reference.covariance does it.

eliminate(..., defect=...) plants one defect in its own output (tests/test_covariance_schur_cpu.py): "drop_term" (one Schur term
X_ge X_g'e^T is not subtracted), "no_delta" (delta L^-T L^-1 omitted), "flip_fe" (the sign of the (f, e) blocks), "truncate" (F(e) cut
to its first 64 members in the back-substitution)."""
import numpy as np

import covariance_reference as cv

LD = np.longdouble


def model_coo(model, x, blocks, T):
    """(rows, tangent columns, values in T, number of rows) of the model's loss-corrected Jacobian over the blocks that move."""
    cmap = cv._column_map(blocks, model.n)
    rows, cols, vals, row0 = [], [], [], 0
    for r, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        nb, k = terms[0][0].shape[0], terms[0][0].shape[1]
        rr = row0 + np.arange(nb)[:, None] * k + np.arange(k)[None, :]
        for J, t_first in terms:
            w = J.shape[2]
            c = cmap[np.asarray(t_first, dtype=np.int64)[:, None] + np.arange(w)]
            R, Cc = np.broadcast_to(rr[:, :, None], (nb, k, w)), np.broadcast_to(c[:, None, :], (nb, k, w))
            keep = Cc >= 0
            rows.append(R[keep]); cols.append(Cc[keep]); vals.append(np.asarray(J)[keep].astype(T))
        row0 += nb * k
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), row0


def crs_coo(jac, blocks, T=LD):
    """The same from a CRSMatrix of Problem::Evaluate whose columns are the blocks in block order, each with its tangent size."""
    first, _ = cv.columns(blocks)
    emap = []
    for b, f in zip(blocks, first):
        emap += list(f + np.arange(b.tangent)) if f >= 0 else [-1] * b.tangent
    assert len(emap) == jac.num_cols
    ptr = np.asarray(jac.rows[:jac.num_rows + 1], dtype=np.int64)
    rows = np.repeat(np.arange(jac.num_rows, dtype=np.int64), np.diff(ptr))
    cols = np.asarray(emap, dtype=np.int64)[np.asarray(jac.cols[:ptr[-1]], dtype=np.int64)]
    assert np.all(cols >= 0)
    return rows, cols, np.asarray(jac.values[:ptr[-1]]).astype(T), jac.num_rows


def greedy_set(coo, blocks, order=None):
    """(E as a sorted list of block indices, F in block order, {block: sorted neighbours}) from the rows' structure.  order: per
    block its index in the problem's own order (Problem.parameterBlockIndex), which breaks the ties of the visit; None: the
    blocks' order here."""
    rows, cols = coo[0], coo[1]
    first, n = cv.columns(blocks)
    moving = [b for b, f in enumerate(first) if f >= 0]
    owner = np.full(max(n, 1), -1, dtype=np.int64)
    for b in moving:
        owner[first[b]:first[b] + blocks[b].tangent] = b
    nbrs = {b: set() for b in moving}
    if len(rows):
        rb = np.unique(np.stack([rows, owner[cols]], axis=1), axis=0)      # sorted by row, then block
        _, start, count = np.unique(rb[:, 0], return_index=True, return_counts=True)
        for length in np.unique(count):
            if length < 2:
                continue
            at = start[count == length]
            for tup in np.unique(rb[at[:, None] + np.arange(length), 1], axis=0):
                for p in tup:
                    nbrs[int(p)].update(int(q) for q in tup if q != p)
    E = set()
    for b in sorted(moving, key=lambda q: (len(nbrs[q]), q if order is None else order[q])):
        if not (nbrs[b] & E):
            E.add(b)
    return sorted(E), [b for b in moving if b not in E], {b: sorted(v) for b, v in nbrs.items()}


def plan(coo, blocks, order=None):
    """What sk_covariance_elimination_plan reports (eliminated_of_block in the blocks' order here), and "E"."""
    E, F, nbrs = greedy_set(coo, blocks, order)
    of_block = np.full(len(blocks), -1, dtype=np.int64)
    of_block[F] = 0
    of_block[E] = 1
    return dict(E=E, eliminated_of_block=of_block, num_eliminated=len(E), reduced_columns=sum(blocks[b].tangent for b in F),
                schur_terms=sum(len(nbrs[e]) * (len(nbrs[e]) + 1) // 2 for e in E))


def _batched_factor(V):
    """(L, L^-1) of the blocks V [m, s, s] by column loops over s, batched over m; None where a pivot is not positive."""
    m, s = V.shape[0], V.shape[1]
    L, Li = np.zeros_like(V), np.zeros_like(V)
    for j in range(s):
        dj = V[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=1)
        if not np.all(dj > 0) or not np.all(np.isfinite(dj)):
            return None, None
        L[:, j, j] = np.sqrt(dj)
        if j + 1 < s:
            L[:, j + 1:, j] = (V[:, j + 1:, j] - np.einsum("mik,mk->mi", L[:, j + 1:, :j], L[:, j, :j])) / L[:, j, j][:, None]
    eye = np.eye(s, dtype=V.dtype)
    for i in range(s):
        Li[:, i, :] = (eye[i][None, :] - np.einsum("mk,mkj->mj", L[:, i, :i], Li[:, :i, :])) / L[:, i, i][:, None]
    return L, Li


def eliminate(coo, blocks, x, offsets, pairs, T, defect=None, kappa=False, order=None):
    """The requested blocks as covariance_reference.covariance lays them out, plus "E", "F", "reduced_columns", "schur_terms", "k"
    (the selected columns after the expansion of requested e-blocks), "ratio" (over the pivots of every L_e and of L_S) and, with
    kappa, "kappa": kappa_2 of the scaled normal matrix estimated FROM BELOW by 80 power iterations on H~ and on H~^-1."""
    rows, cols, vals, num_rows = coo
    vals = vals.astype(T)
    first, N = cv.columns(blocks)
    E, F, nbrs = greedy_set(coo, blocks, order)
    owner = np.full(max(N, 1), -1, dtype=np.int64)
    for b in E + F:
        owner[first[b]:first[b] + blocks[b].tangent] = b
    fcol, nF = {}, 0
    for b in F:
        fcol[b] = nF
        nF += blocks[b].tangent
    eidx = {b: i for i, b in enumerate(E)}
    nE, smax = len(E), max([blocks[b].tangent for b in E] + [1])
    esize = np.array([blocks[b].tangent for b in E], dtype=np.int64)
    # J_F dense, J_E one vector per row
    red_of_col, e_of_col, a_of_col = np.full(max(N, 1), -1, dtype=np.int64), np.full(max(N, 1), -1, dtype=np.int64), np.zeros(max(N, 1), dtype=np.int64)
    for b in F:
        red_of_col[first[b]:first[b] + blocks[b].tangent] = fcol[b] + np.arange(blocks[b].tangent)
    for b in E:
        e_of_col[first[b]:first[b] + blocks[b].tangent] = eidx[b]
        a_of_col[first[b]:first[b] + blocks[b].tangent] = np.arange(blocks[b].tangent)
    in_f = red_of_col[cols] >= 0
    # the F entries of every row, padded to the longest row with a dummy column n_F (a row names a few blocks: J_F is never formed)
    order = np.argsort(rows[in_f], kind="stable")
    rf, cf, vf = rows[in_f][order], red_of_col[cols[in_f]][order], vals[in_f][order]
    count = np.bincount(rf, minlength=num_rows) if len(rf) else np.zeros(num_rows, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    width = int(count.max()) if len(rf) else 0
    colpad, valpad = np.full((num_rows, max(width, 1)), nF, dtype=np.int64), np.zeros((num_rows, max(width, 1)), dtype=T)
    colpad[rf, np.arange(len(rf)) - start[rf]] = cf
    valpad[rf, np.arange(len(rf)) - start[rf]] = vf
    e_of_row, je = np.full(num_rows, -1, dtype=np.int64), np.zeros((num_rows, smax), dtype=T)
    re, ce, ve = rows[~in_f], cols[~in_f], vals[~in_f]
    e_of_row[re] = e_of_col[ce]
    assert np.all(e_of_row[re] == e_of_col[ce]), "a row stores two e-blocks: E is not independent"
    np.add.at(je, (re, a_of_col[ce]), ve)
    with_e = np.flatnonzero(e_of_row >= 0)
    U, V, W = np.zeros((nF + 1, nF + 1), dtype=T), np.zeros((max(nE, 1), smax, smax), dtype=T), np.zeros((max(nE, 1), smax, nF + 1), dtype=T)
    np.add.at(U, (colpad[:, :, None], colpad[:, None, :]), valpad[:, :, None] * valpad[:, None, :])
    np.add.at(V, e_of_row[with_e], je[with_e][:, :, None] * je[with_e][:, None, :])
    np.add.at(W, (e_of_row[with_e][:, None, None], np.arange(smax)[None, :, None], colpad[with_e][:, None, :]), je[with_e][:, :, None] * valpad[with_e][:, None, :])
    U, W = U[:max(nF, 1), :max(nF, 1)], W[:, :, :max(nF, 1)]
    # d over all columns; the first zero in column order is reported
    diag = np.zeros(max(N, 1), dtype=T)
    for b in F:
        diag[first[b]:first[b] + blocks[b].tangent] = np.diag(U)[fcol[b]:fcol[b] + blocks[b].tangent]
    for b in E:
        diag[first[b]:first[b] + blocks[b].tangent] = np.diag(V[eidx[b]])[:blocks[b].tangent]
    zero = np.flatnonzero(diag[:N] == 0)
    if len(zero):
        b = int(owner[zero[0]])
        raise cv.RankDeficient(b, int(zero[0]) - first[b])
    d = 1 / np.sqrt(diag)
    dF = np.ones(max(nF, 1), dtype=T)
    for b in F:
        dF[fcol[b]:fcol[b] + blocks[b].tangent] = d[first[b]:first[b] + blocks[b].tangent]
    dE = np.ones((max(nE, 1), smax), dtype=T)
    for b in E:
        dE[eidx[b], :blocks[b].tangent] = d[first[b]:first[b] + blocks[b].tangent]
    real = np.arange(smax)[None, :] < (esize[:, None] if nE else np.zeros((1, 1), dtype=np.int64))      # the padding of a short block: an identity
    Vs = V * dE[:, :, None] * dE[:, None, :]
    pad = np.arange(smax)
    Vs[:, pad, pad] = np.where(real, Vs[:, pad, pad], 1)
    L, Li = _batched_factor(Vs)
    if L is None:
        raise cv.RankDeficient(-1, -1)
    X = np.matmul(Li, W * dE[:, :, None] * dF[None, None, :])           # X_e = L_e^-1 W~_e^T: [nE, smax, nF]
    if nE == 0:
        X[...] = 0
    S = U * dF[:, None] * dF[None, :]
    fcols = {e: np.concatenate([fcol[g] + np.arange(blocks[g].tangent) for g in nbrs[e]] + [np.zeros(0, dtype=np.int64)]).astype(np.int64) for e in E}
    for e in E:                                                          # X_e is zero outside the columns of F(e)
        Xe = X[eidx[e]][:, fcols[e]]
        S[np.ix_(fcols[e], fcols[e])] -= Xe.T @ Xe
    if nF == 0:
        S = np.ones((1, 1), dtype=T)
    if defect == "drop_term":
        e = max(E, key=lambda q: len(nbrs[q]))
        g, h = nbrs[e][-1], nbrs[e][0]
        gs, hs = slice(fcol[g], fcol[g] + blocks[g].tangent), slice(fcol[h], fcol[h] + blocks[h].tangent)
        term = X[eidx[e]][:, gs].T @ X[eidx[e]][:, hs]
        S[gs, hs] += term
        if g != h:
            S[hs, gs] += term.T
    LS = cv.cholesky(S)
    if LS is None:
        raise cv.RankDeficient(-1, -1)
    # C~_FF over the selection alone: the requested F blocks and F(e) of every requested e-block
    named, selected = [], []
    for a, b in pairs:
        for q in (a, b):
            if q not in named:
                named.append(q)
                if first[q] >= 0:
                    for g in ([q] if q in fcol else nbrs[q]):
                        if g not in selected:
                            selected.append(g)
    spos, k = {}, 0
    for g in selected:
        spos[g] = k
        k += blocks[g].tangent
    selcols = np.concatenate([fcol[g] + np.arange(blocks[g].tangent) for g in selected] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    unit = np.zeros((S.shape[0], k), dtype=T)
    unit[selcols, np.arange(k)] = 1
    Y = cv.forward(LS, unit)
    Cff = Y.T @ Y
    piv = np.concatenate([(np.diagonal(L, axis1=1, axis2=2) ** 2)[real] if nE else np.zeros(0, dtype=T), np.diag(LS)[:nF] ** 2])
    out = {"tangent": {}, "ambient": {}, "N": N, "E": E, "F": F, "reduced_columns": nF,
           "schur_terms": sum(len(nbrs[e]) * (len(nbrs[e]) + 1) // 2 for e in E), "ratio": float(piv.min() / piv.max()) if len(piv) else 1.0}

    def x_of(e):
        A = X[eidx[e]][:blocks[e].tangent][:, selcols]
        if defect == "truncate":
            for g in nbrs[e][64:]:
                A[:, spos[g]:spos[g] + blocks[g].tangent] = 0
        return A

    def scaled(a, b):
        ta, tb = blocks[a].tangent, blocks[b].tangent
        if a in fcol and b in fcol:
            return Cff[spos[a]:spos[a] + ta, spos[b]:spos[b] + tb]
        if a in fcol:
            return (-1 if defect != "flip_fe" else 1) * Cff[spos[a]:spos[a] + ta] @ x_of(b).T @ Li[eidx[b]][:tb, :tb]
        if b in fcol:
            return scaled(b, a).T
        La, Lb = Li[eidx[a]][:ta, :ta], Li[eidx[b]][:tb, :tb]
        M = x_of(a) @ Cff @ x_of(b).T
        if a == b and defect != "no_delta":
            M = M + np.eye(ta, dtype=T)
        return La.T @ M @ Lb

    out["k"] = k
    for a, b in list(pairs) + [(q, q) for q in named]:
        A, B = blocks[a], blocks[b]
        if first[a] >= 0 and first[b] >= 0:
            t = scaled(a, b) * d[first[a]:first[a] + A.tangent][:, None] * d[first[b]:first[b] + B.tangent][None, :]
            Pa = cv.lift_matrix(A, x[offsets[a]:offsets[a] + A.size], T)
            Pb = cv.lift_matrix(B, x[offsets[b]:offsets[b] + B.size], T)
            amb = Pa @ t @ Pb.T
        else:
            t, amb = np.zeros((A.tangent, B.tangent), dtype=T), np.zeros((A.size, B.size), dtype=T)
        out["tangent"][(a, b)] = t
        out["ambient"][(a, b)] = amb
    if kappa:
        f8 = np.float64
        JF8 = np.zeros((num_rows, nF + 1))
        np.add.at(JF8, (np.arange(num_rows)[:, None], colpad), valpad.astype(f8))
        JF8, je8, dF8, dE8 = JF8[:, :max(nF, 1)], je.astype(f8), dF.astype(f8), dE.astype(f8)
        Li8, X8, S8inv = Li.astype(f8), X.astype(f8), np.linalg.inv(S.astype(f8))

        def times(vF, vE):                                               # H~ v through J
            u = JF8 @ (dF8 * vF)
            u[with_e] += np.sum(je8[with_e] * (dE8 * vE)[e_of_row[with_e]], axis=1)
            wE = np.zeros_like(vE)
            np.add.at(wE, e_of_row[with_e], je8[with_e] * u[with_e][:, None])
            return dF8 * (JF8.T @ u), dE8 * wE * real

        def solve(bF, bE):                                               # H~^-1 b through the elimination
            yE = np.einsum("mij,mj->mi", Li8, bE)
            zF = S8inv @ (bF - X8.reshape(-1, X8.shape[2]).T @ yE.ravel())
            return zF, np.einsum("mji,mj->mi", Li8, yE - X8 @ zF) * real

        rng = np.random.default_rng(0)
        lam = []
        for op in (times, solve):
            vF, vE = rng.normal(0, 1, max(nF, 1)), rng.normal(0, 1, (max(nE, 1), smax)) * real
            if nF == 0:
                vF[...] = 0
            for _ in range(80):
                nrm = np.sqrt(vF @ vF + np.sum(vE * vE))
                vF, vE = vF / nrm, vE / nrm
                wF, wE = op(vF, vE)
                rayleigh = float(vF @ wF + np.sum(vE * wE))
                vF, vE = wF, wE
            lam.append(rayleigh)
        out["kappa"] = lam[0] * lam[1]
    return out
