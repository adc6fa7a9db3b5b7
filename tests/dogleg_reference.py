"""Traditional dogleg (Ceres 1.x's DoglegStrategy, as recalled: SURVEY.md row a13 is as unpinned) restated in numpy, with the
trust-region loop around it.  CPU only: numpy and the oracle (residuals and Jacobians in double through the models of
tests/step_check.py, which also give the Jacobi scaling); nothing of skeres_amd's native library, and the constants are
written out here, not read from the C++.

    diag_j = sqrt(clamp(||J_s,j||^2, min_lm_diagonal, max_lm_diagonal)),   g_hat = J_s^T r / diag
    Gauss-Newton:  (J_s^T J_s + mu diag^2) y = J_s^T r,  p = -diag y         (mu *= 10 while the matrix is not positive definite)
    Cauchy:        alpha = |g_hat|^2 / |J_s (g_hat / diag)|^2
    step (diag-scaled space): p if |p| <= radius; -(radius / |g_hat|) g_hat if alpha |g_hat| >= radius; else the point of the
    segment from -alpha g_hat to p at distance radius.  Solver's scaled space: / diag.  delta = step * s.

Bundle-adjustment-shaped models are solved through the Schur complement of the points (dense normal equations of the reduced
camera system; the full ones of (150, 3000, 14000) would be 10350 x 10350); everything else through the dense normal equations.
numpy.linalg has no long double: with dtype=np.longdouble the matrix and every product are long double and the solve is
numpy.linalg's in double refined against long-double residuals until the correction is below 2^-60 of the solution.

The log has the device's fields (trust_region_radius is the radius AFTER the iteration's update, as SolverBase logs it) plus
branch ("gn", "cauchy", "interpolated"), reused, mu and the scalars of the interpolation: the step is a s + b g with s = -g_hat / diag
and g = p / diag in the solver's scaled space, and products holds w.r, m.r, |w|^2, w.m, |m|^2 for w = J_s s, m = J_s g (dtype T),
next to the model cost change formed from the step itself (model_cost_change, and model_cost_change_ld in dtype T)."""
import numpy as np

import oracle
import step_check as sc

LD = np.longdouble

MIN_MU = 1e-8
MAX_MU = 1.0
MU_INCREASE_FACTOR = 10.0
INCREASE_THRESHOLD = 0.75
DECREASE_THRESHOLD = 0.25

DEFAULTS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, jacobi_scaling=True,
                max_num_consecutive_invalid_steps=5)


class NotPositiveDefinite(Exception):
    pass


def bal_cost(prob, loss=None):
    """x -> 1/2 sum rho(|r_o|^2) of a BalProblem (oracle residuals, double)."""
    def cost(x):
        r, _, _, _ = oracle.bal_evaluate(prob.num_cameras, prob.num_points, prob.camera_index, prob.point_index, prob.observations,
                                         np.asarray(x, dtype=np.float64), jacobians=False)
        sq = np.einsum("bk,bk->b", r, r)
        if loss is None:
            return 0.5 * float(np.sum(sq))
        return 0.5 * float(sum(oracle.loss_evaluate(loss, float(s))[0] for s in sq))
    return cost


def blocks_cost(model):
    """The same for a step_check.BlocksModel."""
    def cost(x):
        total = 0.0
        for blk in model.blocks:
            params = [x[model.off[i]:model.off[i] + model.sizes[i]] for i in blk[2]]
            ok, res, _ = oracle.evaluate(blk[0], blk[1], params)
            assert ok
            s = float(np.dot(res, res))
            loss = blk[3] if len(blk) > 3 else None
            total += s if loss is None else oracle.loss_evaluate(loss, s)[0]
        return 0.5 * total
    return cost


def _linearize(model, x, s, T):
    """[(r [nb, k], [(J_s [nb, k, w], first column [nb])])] at x, in dtype T, columns scaled by s."""
    out = []
    for r, terms in model.chunks(np.asarray(x, dtype=np.float64)):
        ts = []
        for J, first in terms:
            idx = first[:, None] + np.arange(J.shape[2])
            ts.append(((J * s[idx][:, None, :]).astype(T), first))
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


def _colsq_and_gradient(lin, n, T):
    acc = np.zeros((n, 2), dtype=T)
    for r, terms in lin:
        for J, first in terms:
            sc._scatter(acc, first, np.stack([np.einsum("bkw,bkw->bw", J, J), np.einsum("bkw,bk->bw", J, r)], axis=-1))
    return acc[:, 0], acc[:, 1]


def _solve_spd(A, b, T):
    A64 = A.astype(np.float64)
    try:
        np.linalg.cholesky(A64)
    except np.linalg.LinAlgError:
        raise NotPositiveDefinite()
    y = np.linalg.solve(A64, b.astype(np.float64)).astype(T)
    if T is np.float64:
        return y
    for _ in range(8):
        d = np.linalg.solve(A64, (b - A @ y).astype(np.float64)).astype(T)
        y = y + d
        if np.max(np.abs(d)) <= 2.0 ** -60 * np.max(np.abs(y)):
            break
    return y


def _inv3(V):
    """Inverses of symmetric 3 x 3 matrices [P, 3, 3] by cofactors (any dtype)."""
    a, b, c = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2]
    d, e, f = V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    co = np.empty_like(V)
    co[:, 0, 0] = d * f - e * e
    co[:, 0, 1] = co[:, 1, 0] = c * e - b * f
    co[:, 0, 2] = co[:, 2, 0] = b * e - c * d
    co[:, 1, 1] = a * f - c * c
    co[:, 1, 2] = co[:, 2, 1] = b * c - a * e
    co[:, 2, 2] = a * d - b * b
    det = a * co[:, 0, 0] + b * co[:, 0, 1] + c * co[:, 0, 2]
    if not np.all(det > 0):
        raise NotPositiveDefinite()
    return co / det[:, None, None]


def _gauss_newton_schur(lin, C, P, D2, gs, T):
    """y of (J_s^T J_s + D2) y = gs for camera (9) / point (3) blocks, the points eliminated first."""
    nc = 9 * C
    F = np.concatenate([terms[0][0] for _, terms in lin])
    E = np.concatenate([terms[1][0] for _, terms in lin])
    cam = np.concatenate([terms[0][1] for _, terms in lin]) // 9
    pt = (np.concatenate([terms[1][1] for _, terms in lin]) - nc) // 3
    U = np.zeros((C, 9, 9), dtype=T)
    V = np.zeros((P, 3, 3), dtype=T)
    sc._scatter(U.reshape(C * 9, 9), 9 * cam, np.einsum("bka,bkc->bac", F, F))
    sc._scatter(V.reshape(P * 3, 3), 3 * pt, np.einsum("bka,bkc->bac", E, E))
    U[:, np.arange(9), np.arange(9)] += D2[:nc].reshape(C, 9)
    V[:, np.arange(3), np.arange(3)] += D2[nc:].reshape(P, 3)
    Vinv = _inv3(V)
    W = np.einsum("bka,bkc->bac", F, E)                    # [N, 9, 3]
    S = np.zeros((nc, nc), dtype=T)
    for i in range(C):
        S[9 * i:9 * i + 9, 9 * i:9 * i + 9] = U[i]
    rhs = gs[:nc].copy()
    gp = gs[nc:].reshape(P, 3)
    order = np.argsort(pt, kind="stable")
    bounds = np.flatnonzero(np.r_[True, pt[order][1:] != pt[order][:-1], True])
    for a, b in zip(bounds[:-1], bounds[1:]):
        obs = order[a:b]
        q = pt[obs[0]]
        cams = cam[obs]
        assert len(set(cams.tolist())) == len(cams)
        Wp = W[obs]                                        # [k, 9, 3]
        Tp = np.einsum("iab,bc->iac", Wp, Vinv[q])
        rows = (9 * cams[:, None] + np.arange(9)).ravel()
        S[np.ix_(rows, rows)] -= np.einsum("iab,jcb->iajc", Tp, Wp).reshape(len(rows), len(rows))
        rhs[rows] -= np.einsum("iab,b->ia", Tp, gp[q]).ravel()
    yc = _solve_spd(S, rhs, T)
    t = gp.copy()
    sc._scatter(t, pt, -np.einsum("bac,ba->bc", W, yc.reshape(C, 9)[cam])[:, None, :])
    yp = np.einsum("pab,pb->pa", Vinv, t)
    return np.concatenate([yc, yp.ravel()])


def _gauss_newton_dense(lin, n, D2, gs, T):
    A = np.zeros((n, n), dtype=T)
    for r, terms in lin:
        cols = [first[:, None] + np.arange(J.shape[2]) for J, first in terms]
        for (Ja, _), ca in zip(terms, cols):
            for (Jb, _), cb in zip(terms, cols):
                blk = np.einsum("bka,bkc->bac", Ja, Jb)
                for i in range(blk.shape[0]):
                    A[np.ix_(ca[i], cb[i])] += blk[i]
    A[np.arange(n), np.arange(n)] += D2
    return _solve_spd(A, gs, T)


def solve(model, cost, x0, options=None, dtype=np.float64, schur=None):
    """The trust-region loop with the dogleg strategy from x0.  schur: (cameras, points) of a bundle-adjustment-shaped model.
    Returns (x, log)."""
    T = LD if dtype is LD else np.float64
    o = dict(DEFAULTS)
    o.update(options or {})
    n = model.n
    x = np.array(x0, dtype=np.float64)
    s = sc.jacobi_scale(model, x, o["jacobi_scaling"]).astype(T)
    radius = T(o["initial_trust_region_radius"])
    mu = MIN_MU
    reuse = False
    log = []

    def evaluate(x):
        lin = _linearize(model, x, s, T)
        colsq, gs = _colsq_and_gradient(lin, n, T)
        gmax = float(np.max(np.abs(gs / s)))
        return lin, colsq, gs, gmax, float(np.sqrt(np.sum(x.astype(T) ** 2)))

    def entry(cost_change=0.0, step_norm=0.0, rho=0.0, valid=1, success=1, **extra):
        e = dict(cost=c, cost_change=float(cost_change), gradient_max_norm=gmax, step_norm=float(step_norm), relative_decrease=float(rho),
                 trust_region_radius=float(radius), step_is_valid=valid, step_is_successful=success, mu=mu)
        e.update(extra)
        log.append(e)

    c = cost(x)
    lin, colsq, gs, gmax, xnorm = evaluate(x)
    entry()
    iteration = invalid = 0
    st = None
    while True:
        if iteration >= o["max_num_iterations"] or gmax <= o["gradient_tolerance"] or radius < o["min_trust_region_radius"]:
            break
        iteration += 1
        was_reused = reuse
        solves, quotients = 0, []   # linear solves of this iteration; (mu, quotient, quotient / 2^-1075, zero columns) of each under the option
        if not reuse:
            diag = np.sqrt(np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])))
            ghat = gs / diag
            y = None
            while mu < MAX_MU:
                try:
                    D2 = T(mu) * diag * diag
                    solves += 1
                    if o.get("zero_columns_in_ieee_double"):
                        # (case i-dogleg of tests/dogleg_cases.py: a column that is exactly zero, with a zero gradient entry, has
                        # min_lm_diagonal / (1 / mu) on its diagonal, formed in IEEE double as the device forms it, in BOTH precisions — where
                        # it underflows to 0 the system is not positive definite; where it is positive the unknown is 0 whatever the value, so
                        # the solve proceeds with a unit diagonal there.  The same option of tests/failure_reference.py says more.)
                        zero = (colsq == 0) & (gs == 0)
                        with np.errstate(under="ignore"):
                            quotient = float(np.float64(o["min_lm_diagonal"]) / (np.float64(1.0) / np.float64(mu)))
                        quotients.append((mu, quotient, float(LD(o["min_lm_diagonal"]) * LD(mu) / LD(2) ** -1075), int(np.count_nonzero(zero))))
                        if zero.any() and quotient == 0.0:
                            raise NotPositiveDefinite()
                        D2[zero] = 1
                    y = _gauss_newton_schur(lin, schur[0], schur[1], D2, gs, T) if schur else _gauss_newton_dense(lin, n, D2, gs, T)
                    break
                except NotPositiveDefinite:
                    mu *= MU_INCREASE_FACTOR
            st = None
            if y is not None and np.all(np.isfinite(y)):
                p = -diag * y
                w = _times(lin, -ghat / diag)
                mg = _times(lin, p / diag)
                gg = np.sum(ghat * ghat)
                ww = sum(np.sum(m * m) for m in w)
                st = dict(diag=diag, ghat=ghat, p=p, gg=gg, gp=np.sum(ghat * p), pp=np.sum(p * p), ww=ww,
                          wr=sum(np.sum(m * r) for m, (r, _) in zip(w, lin)), mr=sum(np.sum(m * r) for m, (r, _) in zip(mg, lin)),
                          wm=sum(np.sum(m * v) for m, v in zip(w, mg)), mm=sum(np.sum(m * m) for m in mg))
        ok = st is not None and st["ww"] > 0 and st["gg"] > 0
        if ok:
            gnorm, pnorm, alpha = np.sqrt(st["gg"]), np.sqrt(st["pp"]), st["gg"] / st["ww"]
            if pnorm <= radius:
                branch, step, ab = "gn", st["p"], (0.0, 1.0)
            elif alpha * gnorm >= radius:
                branch, step, ab = "cauchy", -(radius / gnorm) * st["ghat"], (radius / gnorm, 0.0)
            else:
                branch = "interpolated"
                a2 = (alpha * gnorm) ** 2
                ba = -alpha * st["gp"]
                bma2 = a2 - 2 * ba + st["pp"]
                cc = ba - a2
                d = np.sqrt(cc * cc + bma2 * (radius * radius - a2))
                beta = (d - cc) / bma2 if cc <= 0 else (radius * radius - a2) / (d + cc)
                step = -alpha * (1 - beta) * st["ghat"] + beta * st["p"]
                ab = (alpha * (1 - beta), beta)
            dogleg_norm = np.sqrt(np.sum(step * step))
            scaled = step / st["diag"]
            m = _times(lin, scaled)
            mcc = -sum(np.sum(mm * (r + mm / 2)) for mm, (r, _) in zip(m, lin))
            x_new = (x.astype(T) + scaled * s).astype(np.float64)
            ok = bool(mcc > 0) and np.all(np.isfinite(x_new))
        if not ok:
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                entry(valid=0, success=0)
                break
            mu *= MU_INCREASE_FACTOR
            reuse = False
            entry(valid=0, success=0)
            continue
        invalid = 0
        extra = dict(solves=solves, quotients=quotients, branch=branch, reused=was_reused, dogleg_step_norm=float(dogleg_norm), model_cost_change=float(mcc),
                     w_r=float(st["wr"]), g_g=float(st["gg"]), scaled_step=np.asarray(scaled, dtype=T),
                     a=float(ab[0]), b=float(ab[1]), products=tuple(T(st[f]) for f in ("wr", "mr", "ww", "wm", "mm")), model_cost_change_ld=T(mcc))
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
            lin, colsq, gs, gmax, xnorm = evaluate(x)
            if rho < DECREASE_THRESHOLD:
                radius = radius * T(0.5)
            elif rho > INCREASE_THRESHOLD:
                radius = min(T(o["max_trust_region_radius"]), max(radius, 3 * dogleg_norm))
            mu = max(MIN_MU, 2.0 * mu / MU_INCREASE_FACTOR)
            reuse = False
            entry(cost_change, step_norm, rho, 1, 1, **extra)
        else:
            radius = radius * T(0.5)
            reuse = True
            entry(cost_change, step_norm, rho, 1, 0, **extra)
    return x, log


def model_cost_change(model, x0, x_prev, x_next, jacobi_scaling=True):
    """-m . (r + m / 2) with m = J_s step at x_prev, in long double, for the step recovered from the endpoints:
    step = (x_next - x_prev) / s in the solver's scaled space."""
    s = sc.jacobi_scale(model, np.asarray(x0, dtype=np.float64), jacobi_scaling)
    lin = _linearize(model, x_prev, s, LD)
    step = (np.asarray(x_next, dtype=np.float64).astype(LD) - np.asarray(x_prev, dtype=np.float64).astype(LD)) / s
    m = _times(lin, step)
    return float(-sum(np.sum(mm * (r + mm / 2)) for mm, (r, _) in zip(m, lin)))
