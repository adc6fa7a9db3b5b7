"""CGNR with the Schur elimination (sk_options_set_schur_elimination) restated in numpy, in double and in long double.  CPU only;
nothing of skeres_amd's native library.  The linearisation is tests/cgnr_reference.py's (_linearize, the products _times and
_transposed and the block sums); the greedy set, the per-block Cholesky, the implicit Schur complement, the conjugate-gradient
loop over it and the Levenberg-Marquardt loop around it are written here.

    E        the greedy independent set: two moving blocks are neighbours when a residual block names both; ascending (distinct
             neighbours, block index in the problem's own order); a block joins E when no neighbour is in E.  F: every other column
             (the columns of blocks that do not move have a zero Jacobian and a zero right-hand side: their step is 0);
    H        J^T J + D2 = [[U, W], [W^T, V]],  D2 = clamp(diag J^T J) / radius over all columns,  V_e = L_e L_e^T per e-block;
    S v      J_F^T (w - J_E V^-1 J_E^T w) + D2_F v with w = J_F v: never formed;   s = b_F - W V^-1 b_E = -J_F^T (r - J_E V^-1 J_E^T r);
    M        JACOBI: per F block g  U_gg + D2_g - sum_e X_ge^T X_ge,  X_ge = L_e^-1 W_ge^T,  W_ge summed over ALL residual blocks on
             the pair (g, e) first;  IDENTITY: none;
    CG       the loop of cgnr_reference's docstring on S y_F = s; no column in F: 0 iterations, status 0;
    back     y_E = V^-1 (b_E - J_E^T (J_F y_F)).

Model cost change, candidate and acceptance come from the full step (y_F, y_E) as in cgnr_reference.solve.  The log has its fields;
first_direction (M^-1 s, zero on E) and scaled_step run over all columns.

solve(..., defect=...) plants one defect (tests/test_cgnr_schur_cpu.py): "diag_u" (M is the block diagonal of U + D2), "per_slot"
(X^T X formed per residual block of a pair instead of per pair), "no_backsub" (y_E = 0)."""
import numpy as np

import cgnr_reference as cr
import step_check as sc

LD = np.longdouble
CONVERGED, ITERATION_LIMIT, BREAKDOWN, ZERO_RHS = 0, 1, 2, 3


def greedy_set(model, x, blocks, order=None):
    """(E, F: sorted lists of moving blocks, {block: neighbours}).  blocks: [(first column, size)]; order: per block its index in the
    problem's own order, which breaks the ties of the visit (None: the order here)."""
    owner = np.full(model.n, -1, dtype=np.int64)
    for b, (start, size) in enumerate(blocks):
        owner[start:start + size] = b
    moving = [b for b, (start, size) in enumerate(blocks) if np.any(model.free[start:start + size])]
    nbrs = {b: set() for b in moving}
    for _, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        ids = [owner[np.asarray(first, dtype=np.int64)] for _, first in terms]
        for a in range(len(ids)):
            for c in range(len(ids)):
                if a != c:
                    for p, q in np.unique(np.stack([ids[a], ids[c]], axis=1), axis=0):
                        if p != q and int(p) in nbrs and int(q) in nbrs:
                            nbrs[int(p)].add(int(q))
    E = set()
    for b in sorted(moving, key=lambda q: (len(nbrs[q]), q if order is None else order[q])):
        if not (nbrs[b] & E):
            E.add(b)
    return sorted(E), [b for b in moving if b not in E], nbrs


def plan(model, x, blocks, order=None):
    """What sk_cgnr_elimination_plan reports, in the blocks' order here.  tangent: the columns of a block that move."""
    E, F, nbrs = greedy_set(model, x, blocks, order)
    of_block = np.full(len(blocks), -1, dtype=np.int64)
    of_block[F], of_block[E] = 0, 1
    slots = {b: 0 for b in E}
    owner = np.full(model.n, -1, dtype=np.int64)
    for b, (start, size) in enumerate(blocks):
        owner[start:start + size] = b
    for _, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        for _, first in terms:
            for b, k in zip(*np.unique(owner[np.asarray(first, dtype=np.int64)], return_counts=True)):
                if int(b) in slots:
                    slots[int(b)] += int(k)
    return dict(E=E, F=F, eliminated_of_block=of_block, num_eliminated=len(E),
                reduced_columns=sum(int(np.sum(model.free[blocks[b][0]:blocks[b][0] + blocks[b][1]])) for b in F),
                long_eliminated_blocks=sum(1 for b in E if slots[b] > 64), fe_pairs=sum(len(nbrs[e]) for e in E))


def _cholesky(A):
    """Lower factors of A [m, s, s] by a column loop, or None where a pivot is not positive."""
    L = np.zeros_like(A)
    for j in range(A.shape[1]):
        d = A[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
        if not np.all(d > 0) or not np.all(np.isfinite(d)):
            return None
        L[:, j, j] = np.sqrt(d)
        L[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum("mik,mk->mi", L[:, j + 1:, :j], L[:, j, :j])) / L[:, j, j][:, None]
    return L


def _forward(L, B):
    """L^-1 B for L [m, s, s], B [m, s, k]."""
    X = np.zeros_like(B)
    for j in range(L.shape[1]):
        X[:, j] = (B[:, j] - np.einsum("mk,mkc->mc", L[:, j, :j], X[:, :j])) / L[:, j, j][:, None]
    return X


def _backward(L, B):
    """L^-T B."""
    X = np.zeros_like(B)
    for j in range(L.shape[1] - 1, -1, -1):
        X[:, j] = (B[:, j] - np.einsum("mk,mkc->mc", L[:, j + 1:, j], X[:, j + 1:])) / L[:, j, j][:, None]
    return X


class _Blocks:
    """Some column blocks grouped by size: index arrays [m, size] per size, factors of their matrices, solves."""

    def __init__(self, blocks, members):
        self.by_size = {}
        for b in members:
            start, size = blocks[b]
            self.by_size.setdefault(size, []).append((b, start))
        self.idx = {size: np.array([s for _, s in v], dtype=np.int64)[:, None] + np.arange(size) for size, v in self.by_size.items()}
        self.ids = {size: [b for b, _ in v] for size, v in self.by_size.items()}

    def factor(self, mats):
        """mats: {size: [m, size, size]}.  False where one is not positive definite."""
        self.L = {}
        for size, A in mats.items():
            L = _cholesky(A)
            if L is None:
                return False
            self.L[size] = L
        return True

    def solve(self, v):
        """(L L^T)^-1 v on the blocks' columns, zero elsewhere."""
        z = np.zeros_like(v)
        for size, L in self.L.items():
            idx = self.idx[size]
            z[idx] = _backward(L, _forward(L, v[idx][:, :, None]))[:, :, 0]
        return z


class Linearisation:
    """What one Jacobian gives every linear solve at its point: the block sums and, per (F block, e-block) pair, W_ge."""

    def __init__(self, lin, n, blocks, E, F, T):
        self.lin, self.n, self.blocks, self.T = lin, n, blocks, T
        self.emask = np.zeros(n, dtype=bool)
        for b in E:
            self.emask[blocks[b][0]:blocks[b][0] + blocks[b][1]] = True
        self.eb, self.fb = _Blocks(blocks, E), _Blocks(blocks, F)
        sums = cr._block_sums(lin, n, blocks, T)
        self.esums = {size: np.array([sums[b] for b in ids], dtype=T) for size, ids in self.eb.ids.items()}
        self.fsums = {size: np.array([sums[b] for b in ids], dtype=T) for size, ids in self.fb.ids.items()}
        # the terms of the pairs: (g, e, J_g^T J_e) per residual block that names both
        owner = np.full(n, -1, dtype=np.int64)
        for b, (start, _) in enumerate(blocks):
            owner[start] = b
        inE, inF = set(E), set(F)
        by_shape = {}
        for r, terms in lin:
            for Jg, fg in terms:
                g = owner[fg]
                for Je, fe in terms:
                    e = owner[fe]
                    keep = np.array([int(a) in inF and int(c) in inE for a, c in zip(g, e)], dtype=bool)
                    if np.any(keep):
                        by_shape.setdefault((Jg.shape[2], Je.shape[2]), []).append((g[keep], e[keep], np.einsum("bka,bkc->bac", Jg[keep], Je[keep])))
        self.terms = [tuple(np.concatenate([t[k] for t in v]) for k in range(3)) for v in by_shape.values()]

    def schur_diagonal(self, D2, defect=None):
        """{size: [m, size, size]} of the F blocks: U_gg + D2_g - sum_e X_ge^T X_ge with V's factors in self.eb.L."""
        T = self.T
        out = {}
        for size, idx in self.fb.idx.items():
            A = self.fsums[size].copy()
            A[:, np.arange(size), np.arange(size)] += D2[idx]
            out[size] = A
        if defect == "diag_u":
            return out
        fpos = {b: (size, k) for size, ids in self.fb.ids.items() for k, b in enumerate(ids)}
        epos = {b: (size, k) for size, ids in self.eb.ids.items() for k, b in enumerate(ids)}
        for g, e, W in self.terms:
            if defect != "per_slot":      # W_ge: the sum over the pair's residual blocks
                key, inv = np.unique(np.stack([g, e], axis=1), axis=0, return_inverse=True)
                Wsum = np.zeros((len(key),) + W.shape[1:], dtype=T)
                np.add.at(Wsum, inv.ravel(), W)
                g, e, W = key[:, 0], key[:, 1], Wsum
            se = W.shape[2]
            L = self.eb.L[se][[epos[int(c)][1] for c in e]]
            X = _forward(L, np.transpose(W, (0, 2, 1)))                  # [pairs, se, sg]
            np.subtract.at(out[W.shape[1]], [fpos[int(a)][1] for a in g], np.einsum("pja,pjc->pac", X, X))
        return out

    def times_f(self, v):
        return cr._times(self.lin, np.where(self.emask, self.T(0), v))

    def project(self, ws):
        """w - J_E V^-1 J_E^T w per chunk."""
        t = np.where(self.emask, cr._transposed(self.lin, ws, self.n, self.T), self.T(0))
        return [w - m for w, m in zip(ws, cr._times(self.lin, self.eb.solve(t)))]

    def transposed_f(self, ws):
        return np.where(self.emask, self.T(0), cr._transposed(self.lin, ws, self.n, self.T))


def _bad(v):
    return not (v > 0) or not np.isfinite(v)


def conjugate_gradients(A, b, apply_m, o, T):
    """cgnr_reference's loop on A y = b.  Returns (y, iterations, status, zetas, first direction)."""
    x = np.zeros_like(b)
    if not np.any(b != 0):
        return x, 0, ZERO_RHS, [], np.zeros_like(b)
    res, p = b.copy(), np.zeros_like(b)
    rho = rho_last = q0 = T(0)
    zetas, first, it = [], None, 0
    while it < o["max_linear_solver_iterations"]:
        it += 1
        z = apply_m(res)
        rho_last, rho = rho, np.sum(res * z)
        if _bad(rho):
            return x, it - 1, BREAKDOWN, zetas, first
        p = z.copy() if it == 1 else z + (rho / rho_last) * p
        if first is None:
            first = p.copy()
        q = A(p)
        pq = np.sum(p * q)
        if _bad(pq):
            return x, it - 1, BREAKDOWN, zetas, first
        alpha = rho / pq
        x = x + alpha * p
        res = b - A(x) if it % cr.RESIDUAL_RESET_PERIOD == 0 else res - alpha * q
        q1 = -np.sum(x * (b + res)) / 2
        zeta = it * (q1 - q0) / q1
        zetas.append(zeta)
        if zeta < o["eta"] and it >= o["min_linear_solver_iterations"]:
            return x, it, CONVERGED, zetas, first
        q0 = q1
    return x, it, ITERATION_LIMIT, zetas, first if first is not None else np.zeros_like(b)


def linear_solve(Z, D2, b, rs, o, T, defect=None):
    """One linear solve with the elimination: (y over all columns or None, iterations, status, zetas, first direction)."""
    V = {}
    for size, idx in Z.eb.idx.items():
        A = Z.esums[size].copy()
        A[:, np.arange(size), np.arange(size)] += D2[idx]
        V[size] = A
    if not Z.eb.factor(V):
        return None, 0, BREAKDOWN, [], None
    jacobi = o["preconditioner"] == "jacobi"
    if jacobi and not Z.fb.factor(Z.schur_diagonal(D2, defect)):
        return None, 0, BREAKDOWN, [], None
    fmask = ~Z.emask

    def S(v):
        return Z.transposed_f(Z.project(Z.times_f(v))) + np.where(fmask, D2 * v, T(0))

    def apply_m(res):
        return Z.fb.solve(res) if jacobi else res.copy()   # (a column outside every moving block has a zero residual)
    s = -Z.transposed_f(Z.project([r for r in rs]))
    if not Z.fb.ids:
        yF, its, status, zetas, first = np.zeros_like(b), 0, CONVERGED, [], np.zeros_like(b)
    else:
        yF, its, status, zetas, first = conjugate_gradients(S, s, apply_m, o, T)
    if status == BREAKDOWN:
        return None, its, status, zetas, first
    yE = np.zeros_like(b)
    if defect != "no_backsub":
        t = np.where(Z.emask, b - cr._transposed(Z.lin, Z.times_f(yF), Z.n, T), T(0))
        yE = Z.eb.solve(t)
    return yF + yE, its, status, zetas, first


def solve(model, cost, x0, options=None, dtype=np.float64, blocks=None, order=None, defect=None):
    """The Levenberg-Marquardt loop of cgnr_reference.solve with the step above.  Returns (x, log)."""
    T = LD if dtype is LD else np.float64
    o = dict(cr.DEFAULTS)
    o.update(options or {})
    n = model.n
    x = np.array(x0, dtype=np.float64)
    s = sc.jacobi_scale(model, x, o["jacobi_scaling"]).astype(T)
    E, F, _ = greedy_set(model, x, blocks, order)
    radius, decrease_factor = T(o["initial_trust_region_radius"]), T(2)
    log = []

    def evaluate(x):
        lin = cr._linearize(model, x, s, T)
        gs = cr._transposed(lin, [r for r, _ in lin], n, T)
        colsq = np.zeros((n, 1), dtype=T)
        for r, terms in lin:
            for J, first in terms:
                sc._scatter(colsq, first, np.einsum("bkw,bkw->bw", J, J)[:, :, None])
        return lin, colsq[:, 0], gs, float(np.max(np.abs(gs / s))), float(np.sqrt(np.sum(x.astype(T) ** 2))), Linearisation(lin, n, blocks, E, F, T)

    def entry(cost_change=0.0, step_norm=0.0, rho=0.0, valid=1, success=1, **extra):
        e = dict(cost=c, cost_change=float(cost_change), gradient_max_norm=gmax, step_norm=float(step_norm), relative_decrease=float(rho),
                 trust_region_radius=float(radius), step_is_valid=valid, step_is_successful=success, linear_solver_iterations=0, cg_status=-1, zetas=[])
        e.update(extra)
        log.append(e)

    c = cost(x)
    lin, colsq, gs, gmax, xnorm, Z = evaluate(x)
    entry()
    iteration = invalid = 0
    while True:
        if iteration >= o["max_num_iterations"] or gmax <= o["gradient_tolerance"] or radius < o["min_trust_region_radius"]:
            break
        iteration += 1
        D2 = np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])) / radius
        y, its, status, zetas, first = linear_solve(Z, D2, -gs, [r for r, _ in lin], o, T, defect)
        extra = dict(linear_solver_iterations=its, cg_status=status, zetas=[float(v) for v in zetas], first_direction=first)
        ok = y is not None and np.all(np.isfinite(y))
        if ok:
            m = cr._times(lin, y)
            mcc = -sum(np.sum(mm * (r + mm / 2)) for mm, (r, _) in zip(m, lin))
            delta = y * s
            x_new = model.plus(x, delta) if hasattr(model, "plus") else (x.astype(T) + delta).astype(np.float64)
            ok = bool(mcc > 0) and np.all(np.isfinite(x_new))
            extra.update(model_cost_change=float(mcc), scaled_step=np.asarray(y, dtype=T))
        if not ok:
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                entry(valid=0, success=0, **extra)
                break
            radius, decrease_factor = radius / decrease_factor, decrease_factor * 2
            entry(valid=0, success=0, **extra)
            continue
        invalid = 0
        new_cost = cost(x_new)
        if not np.isfinite(new_cost):
            new_cost = np.finfo(np.float64).max
        cost_change = c - new_cost
        step_norm = float(np.sqrt(np.sum((x - x_new) ** 2)))
        if step_norm <= o["parameter_tolerance"] * (xnorm + o["parameter_tolerance"]) or abs(cost_change) <= o["function_tolerance"] * c:
            entry(cost_change, step_norm, 0.0, 1, 0, **extra)
            break
        rho = cost_change / float(mcc)
        if rho > o["min_relative_decrease"]:
            x, c = x_new, new_cost
            lin, colsq, gs, gmax, xnorm, Z = evaluate(x)
            radius = min(T(o["max_trust_region_radius"]), radius / max(T(1) / 3, 1 - (2 * T(rho) - 1) ** 3))
            decrease_factor = T(2)
            entry(cost_change, step_norm, rho, 1, 1, **extra)
        else:
            radius, decrease_factor = radius / decrease_factor, decrease_factor * 2
            entry(cost_change, step_norm, rho, 1, 0, **extra)
    return x, log
