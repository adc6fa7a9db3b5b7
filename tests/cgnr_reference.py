"""CGNR (Ceres 1.x's ConjugateGradientsSolver on the damped normal equations, as recalled: SURVEY.md row a13 is as unpinned)
restated in numpy, with the Levenberg-Marquardt loop around it.  CPU only: numpy and the oracle (residuals and Jacobians in double
through the models of tests/step_check.py, which also give the Jacobi scaling); nothing of skeres_amd's native library, and the
constants are written out here, not read from the C++.

Per LM iteration at radius mu, with J_s the corrected Jacobian scaled by s_j = 1 / (1 + ||J_j||) of the Jacobian at x0:

    D2 = clamp(diag J_s^T J_s, min_lm_diagonal, max_lm_diagonal) / mu,   A = J_s^T J_s + D2 (never formed),   b = -J_s^T r
    x = 0, res = b;  ||b|| = 0: the step is 0 (status 3)
    it = 1, 2, ...:  z = M^-1 res;  rho = res . z;  p = z (it = 1) else z + (rho / rho_last) p;  q = A p;  alpha = rho / p . q
                     x += alpha p;  res = b - A x when it % 10 == 0 else res - alpha q
                     Q1 = -1/2 x . (b + res);  zeta = it (Q1 - Q0) / Q1;  stop (status 0) when zeta < eta and it >= min iterations
                     Q0 = Q1;  stop (status 1) at it = max iterations: the step is used
    rho or p . q zero, negative or not finite: status 2, the step is invalid
    M: JACOBI the block diagonal of A over the parameter blocks (small Cholesky per block), IDENTITY M = I.

The step is delta = x in the scaled space, the model cost change -(J_s delta) . (r + J_s delta / 2) formed from the step, the
candidate x + delta s (through model.plus where the model has one: a tangent-space model).  Acceptance, radius and termination are
the Levenberg-Marquardt loop's of SolverBase.

With dtype=np.longdouble every vector, product and sum is long double (the Jacobian itself comes from the oracle in double, or
from the long-double tape interpreter).  The log has the device's fields (trust_region_radius is the radius AFTER the iteration's
update) plus, per iteration, linear_solver_iterations, cg_status, zetas (the zeta sequence), model_cost_change, first_direction
(M^-1 b, the first search direction) and scaled_step."""
import numpy as np

import oracle
import step_check as sc

LD = np.longdouble

RESIDUAL_RESET_PERIOD = 10
CONVERGED, ITERATION_LIMIT, BREAKDOWN, ZERO_RHS = 0, 1, 2, 3

DEFAULTS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, jacobi_scaling=True,
                max_num_consecutive_invalid_steps=5,
                eta=0.1, max_linear_solver_iterations=500, min_linear_solver_iterations=0, preconditioner="jacobi")


def _linearize(model, x, s, T):
    """[(r [nb, k], [(J_s [nb, k, w], first column [nb])])] at x, in dtype T, columns scaled by s."""
    out = []
    for r, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        ts = []
        for J, first in terms:
            idx = first[:, None] + np.arange(J.shape[2])
            ts.append(((J * s[idx][:, None, :]).astype(T), np.asarray(first, dtype=np.int64)))
        out.append((r.astype(T), ts))
    return out


def _times(lin, v):
    """J_s v per chunk."""
    out = []
    for r, terms in lin:
        m = np.zeros_like(r)
        for J, first in terms:
            m += np.einsum("bkw,bw->bk", J, v[first[:, None] + np.arange(J.shape[2])])
        out.append(m)
    return out


def _transposed(lin, ws, n, T):
    """J_s^T w from the per-chunk rows ws."""
    out = np.zeros((n, 1), dtype=T)
    for (r, terms), w in zip(lin, ws):
        for J, first in terms:
            sc._scatter(out, first, np.einsum("bkw,bk->bw", J, w)[:, :, None])
    return out[:, 0]


def _block_sums(lin, n, blocks, T):
    """Per column block (start, size) the size x size sum of J_b^T J_b over the residual blocks on it."""
    by_width = {}
    for r, terms in lin:
        for J, first in terms:
            w = J.shape[2]
            acc = by_width.setdefault(w, np.zeros((n, w), dtype=T))
            sc._scatter(acc, first, np.einsum("bka,bkc->bac", J, J))
    out = []
    for start, size in blocks:
        out.append(by_width[size][start:start + size].copy() if size in by_width else np.zeros((size, size), dtype=T))
    return out


def _cholesky(A):
    """Lower Cholesky factors of the matrices A [nblk, s, s] (any dtype), or None where one is not positive definite."""
    A = A.copy()
    s = A.shape[1]
    L = np.zeros_like(A)
    for j in range(s):
        d = A[:, j, j] - np.einsum("bk,bk->b", L[:, j, :j], L[:, j, :j])
        if not np.all(d > 0) or not np.all(np.isfinite(d)):
            return None
        L[:, j, j] = np.sqrt(d)
        for i in range(j + 1, s):
            L[:, i, j] = (A[:, i, j] - np.einsum("bk,bk->b", L[:, i, :j], L[:, j, :j])) / L[:, j, j]
    return L


def _cholesky_solve(L, v):
    """(L L^T)^-1 v for L [nblk, s, s], v [nblk, s]."""
    s = L.shape[1]
    y = np.zeros_like(v)
    for j in range(s):
        y[:, j] = (v[:, j] - np.einsum("bk,bk->b", L[:, j, :j], y[:, :j])) / L[:, j, j]
    z = np.zeros_like(v)
    for j in range(s - 1, -1, -1):
        z[:, j] = (y[:, j] - np.einsum("bk,bk->b", L[:, j + 1:, j], z[:, j + 1:])) / L[:, j, j]
    return z


class _Jacobi:
    """M = block diagonal of J_s^T J_s + D2 over the column blocks; the sums are formed once per Jacobian, D2 added per solve."""

    def __init__(self, lin, n, blocks, T):
        self.blocks, self.T = blocks, T
        sums = _block_sums(lin, n, blocks, T)
        self.by_size = {}
        for k, (start, size) in enumerate(blocks):
            self.by_size.setdefault(size, ([], []))
            self.by_size[size][0].append(start)
            self.by_size[size][1].append(sums[k])

    def factor(self, D2):
        self.L = {}
        for size, (starts, mats) in self.by_size.items():
            starts = np.asarray(starts, dtype=np.int64)
            A = np.array(mats, dtype=self.T)
            idx = starts[:, None] + np.arange(size)
            A[:, np.arange(size), np.arange(size)] += D2[idx]
            L = _cholesky(A)
            if L is None:
                return False
            self.L[size] = (idx, L)
        return True

    def apply(self, v):
        z = np.zeros_like(v)
        for size, (idx, L) in self.L.items():
            z[idx] = _cholesky_solve(L, v[idx])
        return z


def _bad(v):
    return not (v > 0) or not np.isfinite(v)


def conjugate_gradients(lin, n, D2, b, precond, o, T):
    """The loop of the module docstring.  Returns (x, iterations, status, zetas, first direction)."""
    def A(v):
        return _transposed(lin, _times(lin, v), n, T) + D2 * v
    x = np.zeros(n, dtype=T)
    if not np.any(b != 0):
        return x, 0, ZERO_RHS, [], np.zeros(n, dtype=T)
    res = b.copy()
    rho = rho_last = T(0)
    p = np.zeros(n, dtype=T)
    q0 = T(0)
    zetas, first = [], None
    it = 0
    while it < o["max_linear_solver_iterations"]:
        it += 1
        z = precond.apply(res) if precond is not None else res.copy()
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
        res = b - A(x) if it % RESIDUAL_RESET_PERIOD == 0 else res - alpha * q
        q1 = -np.sum(x * (b + res)) / 2
        zeta = it * (q1 - q0) / q1
        zetas.append(zeta)
        if zeta < o["eta"] and it >= o["min_linear_solver_iterations"]:
            return x, it, CONVERGED, zetas, first
        q0 = q1
    return x, it, ITERATION_LIMIT, zetas, first if first is not None else np.zeros(n, dtype=T)


def solve(model, cost, x0, options=None, dtype=np.float64, blocks=None, exact=False):
    """The Levenberg-Marquardt loop with CGNR steps from x0.  blocks: [(first column, size)] of the model's parameter blocks (the
    preconditioner's blocks).  exact: the damped normal equations solved by numpy.linalg (double) instead — the trajectory that
    the cross-check with the factorisation solvers is measured against.  Returns (x, log)."""
    T = LD if dtype is LD else np.float64
    o = dict(DEFAULTS)
    o.update(options or {})
    n = model.n
    x = np.array(x0, dtype=np.float64)
    s = sc.jacobi_scale(model, x, o["jacobi_scaling"]).astype(T)
    radius = T(o["initial_trust_region_radius"])
    decrease_factor = T(2)
    log = []

    def evaluate(x):
        lin = _linearize(model, x, s, T)
        gs = _transposed(lin, [r for r, _ in lin], n, T)
        colsq = np.zeros((n, 1), dtype=T)
        for r, terms in lin:
            for J, first in terms:
                sc._scatter(colsq, first, np.einsum("bkw,bkw->bw", J, J)[:, :, None])
        gmax = float(np.max(np.abs(gs / s)))
        pre = _Jacobi(lin, n, blocks, T) if o["preconditioner"] == "jacobi" and not exact else None
        return lin, colsq[:, 0], gs, gmax, float(np.sqrt(np.sum(x.astype(T) ** 2))), pre

    def entry(cost_change=0.0, step_norm=0.0, rho=0.0, valid=1, success=1, **extra):
        e = dict(cost=c, cost_change=float(cost_change), gradient_max_norm=gmax, step_norm=float(step_norm), relative_decrease=float(rho),
                 trust_region_radius=float(radius), step_is_valid=valid, step_is_successful=success, linear_solver_iterations=0, cg_status=-1, zetas=[])
        e.update(extra)
        log.append(e)

    c = cost(x)
    lin, colsq, gs, gmax, xnorm, pre = evaluate(x)
    entry()
    iteration = invalid = 0
    while True:
        if iteration >= o["max_num_iterations"] or gmax <= o["gradient_tolerance"] or radius < o["min_trust_region_radius"]:
            break
        iteration += 1
        D2 = np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])) / radius
        b = -gs
        extra = {}
        ok = True
        if exact:
            y, its, status, zetas, first = _exact(lin, n, D2, b), 0, CONVERGED, [], None
        else:
            if pre is not None and not pre.factor(D2):
                ok, y, its, status, zetas, first = False, None, 0, BREAKDOWN, [], None
            else:
                y, its, status, zetas, first = conjugate_gradients(lin, n, D2, b, pre, o, T)
        extra = dict(linear_solver_iterations=its, cg_status=status, zetas=[float(v) for v in zetas], first_direction=first)
        ok = ok and status != BREAKDOWN and np.all(np.isfinite(y))
        if ok:
            m = _times(lin, y)
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
            radius = radius / decrease_factor
            decrease_factor = decrease_factor * 2
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
            lin, colsq, gs, gmax, xnorm, pre = evaluate(x)
            radius = min(T(o["max_trust_region_radius"]), radius / max(T(1) / 3, 1 - (2 * T(rho) - 1) ** 3))
            decrease_factor = T(2)
            entry(cost_change, step_norm, rho, 1, 1, **extra)
        else:
            radius = radius / decrease_factor
            decrease_factor = decrease_factor * 2
            entry(cost_change, step_norm, rho, 1, 0, **extra)
    return x, log


def _exact(lin, n, D2, b):
    """(J_s^T J_s + D2)^-1 b through the sparse normal equations in double (scipy's sparse LU)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [D2.astype(np.float64)]
    for r, terms in lin:
        idx = [first[:, None] + np.arange(J.shape[2]) for J, first in terms]
        for (Ja, _), ca in zip(terms, idx):
            for (Jb, _), cb in zip(terms, idx):
                blk = np.einsum("bka,bkc->bac", Ja, Jb).astype(np.float64)
                rows.append(np.broadcast_to(ca[:, :, None], blk.shape).ravel())
                cols.append(np.broadcast_to(cb[:, None, :], blk.shape).ravel())
                vals.append(blk.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    return spla.spsolve(A, b.astype(np.float64)).astype(b.dtype)


def tape_cost(model):
    """x -> 1/2 sum |r|^2 of a model whose blocks carry no loss (the rows of chunks() are the residuals themselves)."""
    def cost(x):
        return 0.5 * float(sum(np.sum(r * r) for r, _ in model.chunks(np.asarray(x, dtype=np.float64))))
    return cost


class QuaternionTangentModel(sc._Model):
    """A step_check.TapeModel over x = (a quaternion block, then plain coordinates), in the tangent space: the quaternion's columns
    are its three tangent coordinates, J P(x) with P = dPlus/ddelta at 0 (oracle/parameterization.hpp), the other columns move
    down by one, and plus() is the quaternion's on the first block and an addition on the rest."""

    def __init__(self, tape_model):
        assert tape_model.n >= 4
        self.inner = tape_model
        self.n = tape_model.n - 1
        self.free = np.ones(self.n, dtype=bool)
        self.kind = np.zeros(self.n, dtype=np.int8)

    def chunks(self, x):
        x = np.asarray(x, dtype=np.float64)
        P = np.asarray(oracle.parameterization_jacobian(("quaternion",), x[:4]), dtype=LD).reshape(4, 3)
        for r, terms in self.inner.chunks(x):
            out = []
            for J, first in terms:
                assert np.all(first == 0) or np.all(first >= 4)
                out.append((np.einsum("bkg,gl->bkl", J, P), first) if np.all(first == 0) else (J, first - 1))
            yield r, out

    def plus(self, x, delta):
        x, delta = np.asarray(x, dtype=np.float64), np.asarray(delta, dtype=np.float64)
        return np.concatenate([oracle.parameterization_plus(("quaternion",), x[:4], delta[:3]), x[4:] + delta[3:]])
