"""Ceres 1.x's trust-region loop under parameter bounds (as recalled: SURVEY.md row a13 is as unpinned) restated in numpy.  CPU only:
numpy and the oracle (residuals and Jacobians in double through the models of tests/step_check.py, which also give the Jacobi
scaling; the Schur and dense solves of tests/dogleg_reference.py); nothing of skeres_amd's native library, and the constants are
written out here, not read from the C++.

    iteration 0:  x <- P(x) = min(max(x, lo), hi); initial cost = cost(P(x))
    gradient_max_norm = max_j |x_j - P(x_j - g_j)|, g = J^T r in the caller's coordinates (not the Jacobi-scaled ones)
    step:         (J_s^T J_s + D^2) y = J_s^T r,  D^2 = clamp(||J_s,j||^2, min, max) / radius,  delta = -y * s;  the model's cost change
                  is that of the unconstrained delta
    line search on phi(alpha) = cost(P(x + alpha delta)) with f0 = cost(x), g0 = g . delta: alpha = 1 first; accept the first alpha
                  with phi finite and phi <= f0 + 1e-4 alpha g0; else the next alpha is the minimiser of the quadratic through
                  (0, f0, slope g0) and (alpha, phi), -g0 alpha^2 / (2 (phi - f0 - g0 alpha)), clamped to [1e-3 alpha, 0.6 alpha]
                  (0.5 alpha after a phi that is not finite); failed after 20 contractions or when alpha max_j |delta_j| < 1e-9;
                  failed, or g0 not negative and finite: alpha = 1.  (Ceres' default interpolation is CUBIC with a Jacobian at every
                  trial point: the quadratic from function values is this project's one departure.)
    candidate P(x + alpha delta); step_norm = |x - candidate|; tolerances, rho, radius update and acceptance as without bounds.

The log has the device's fields (trust_region_radius is the radius AFTER the iteration's update, as SolverBase logs it) plus, per
iteration: step_size (alpha), line_search_evaluations, trials [(alpha, phi)], active_bounds (coordinates of x on a bound after the
iteration), g0, margins (per Armijo test |phi - (f0 + 1e-4 alpha g0)| / f0) and unclamped (per interpolation: the quadratic's
minimiser over the alpha it came from, before the clamp)."""
import numpy as np

import step_check as sc
import dogleg_reference as dr

LD = np.longdouble

SUFFICIENT_DECREASE = 1e-4
MAX_STEP_CONTRACTION = 1e-3
MIN_STEP_CONTRACTION = 0.6
MAX_CONTRACTIONS = 20
MIN_STEP_SIZE = 1e-9

DEFAULTS = dict(dr.DEFAULTS)


def project(x, lo, hi):
    return np.minimum(np.maximum(x, lo), hi)


def line_search(phi_of, f0, g0, max_delta, log=None):
    """(alpha, phi(alpha), trials, margins, unclamped).  phi_of(alpha) -> cost of P(x + alpha delta) (float, may be non-finite)."""
    trials, margins, unclamped = [], [], []
    alpha = 1.0
    phi = phi_of(alpha)
    trials.append((alpha, phi))
    if not (g0 < 0.0 and np.isfinite(g0)):
        return alpha, phi, trials, margins, unclamped
    found = False
    contractions = 0
    while True:
        if np.isfinite(phi):
            bound = f0 + SUFFICIENT_DECREASE * alpha * g0
            margins.append(abs(phi - bound) / f0)
            if phi <= bound:
                found = True
                break
        if contractions == MAX_CONTRACTIONS:
            break
        if np.isfinite(phi):
            nxt = -g0 * alpha * alpha / (2.0 * (phi - f0 - g0 * alpha))
            unclamped.append(nxt / alpha)
            nxt = min(max(nxt, MAX_STEP_CONTRACTION * alpha), MIN_STEP_CONTRACTION * alpha)
        else:
            nxt = 0.5 * alpha
        if nxt * max_delta < MIN_STEP_SIZE:
            break
        alpha = nxt
        contractions += 1
        phi = phi_of(alpha)
        trials.append((alpha, phi))
    if not found and alpha != 1.0:
        alpha = 1.0
        phi = phi_of(alpha)
        trials.append((alpha, phi))
    return alpha, phi, trials, margins, unclamped


def solve(model, cost, x0, lo, hi, options=None, dtype=np.float64, schur=None):
    """The trust-region loop (Levenberg-Marquardt) under the box [lo, hi] from x0.  schur: (cameras, points) of a
    bundle-adjustment-shaped model.  lo = -inf, hi = +inf everywhere gives the unbounded loop.  Returns (x, log)."""
    T = LD if dtype is LD else np.float64
    o = dict(DEFAULTS)
    o.update(options or {})
    n = model.n
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    x = project(np.array(x0, dtype=np.float64), lo, hi)
    s = sc.jacobi_scale(model, x, o["jacobi_scaling"]).astype(T)
    free = np.asarray(model.free, dtype=bool)
    radius = T(o["initial_trust_region_radius"])
    decrease_factor = 2.0
    log = []

    def evaluate(x):
        lin = dr._linearize(model, x, s, T)
        colsq, gs = dr._colsq_and_gradient(lin, n, T)
        xt = x.astype(T)
        pg = np.abs(xt - project(xt - gs / s, lo.astype(T), hi.astype(T)))
        gmax = float(np.max(np.where(free, pg, 0)))
        return lin, colsq, gs, gmax, float(np.sqrt(np.sum(xt ** 2)))

    def active(x):
        return int(np.sum((x == lo) | (x == hi)))

    def entry(cost_change=0.0, step_norm=0.0, rho=0.0, valid=1, success=1, **extra):
        e = dict(cost=c, cost_change=float(cost_change), gradient_max_norm=gmax, step_norm=float(step_norm), relative_decrease=float(rho),
                 trust_region_radius=float(radius), step_is_valid=valid, step_is_successful=success, step_size=1.0,
                 line_search_evaluations=1, trials=[], margins=[], unclamped=[], active_bounds=active(x))
        e.update(extra)
        log.append(e)

    c = cost(x)
    lin, colsq, gs, gmax, xnorm = evaluate(x)
    entry()
    iteration = invalid = 0
    while True:
        if iteration >= o["max_num_iterations"] or gmax <= o["gradient_tolerance"] or radius < o["min_trust_region_radius"]:
            break
        iteration += 1
        D2 = np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])) / radius
        ok = True
        try:
            y = dr._gauss_newton_schur(lin, schur[0], schur[1], D2, gs, T) if schur else dr._gauss_newton_dense(lin, n, D2, gs, T)
        except dr.NotPositiveDefinite:
            ok = False
        if ok:
            step = -y
            m = dr._times(lin, step)
            mcc = -sum(np.sum(mm * (r + mm / 2)) for mm, (r, _) in zip(m, lin))
            delta = step * s
            ok = bool(mcc > 0) and bool(np.all(np.isfinite(delta)))
        if not ok:
            invalid += 1
            entry(valid=0, success=0)
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                break
            radius = radius / T(decrease_factor)
            decrease_factor *= 2.0
            log[-1]["trust_region_radius"] = float(radius)
            continue
        invalid = 0
        g0 = float(np.sum(gs * step))
        max_delta = float(np.max(np.abs(delta)))
        xt = x.astype(T)

        def candidate(alpha):
            return project(xt + T(alpha) * delta, lo.astype(T), hi.astype(T)).astype(np.float64)

        alpha, new_cost, trials, margins, unclamped = line_search(lambda a: cost(candidate(a)), c, g0, max_delta)
        x_new = candidate(alpha)
        extra = dict(step_size=alpha, line_search_evaluations=len(trials), trials=trials, margins=margins, unclamped=unclamped, g0=g0,
                     model_cost_change=float(mcc))
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
            radius = min(T(o["max_trust_region_radius"]), radius / max(T(1) / 3, 1 - (2 * T(rho) - 1) ** 3))
            decrease_factor = 2.0
            entry(cost_change, step_norm, rho, 1, 1, **extra)
        else:
            radius = radius / T(decrease_factor)
            decrease_factor *= 2.0
            entry(cost_change, step_norm, rho, 1, 0, **extra)
    return x, log


def projected_gradient_max_norm(model, x0, x, lo, hi, jacobi_scaling=True):
    """max_j |x_j - P(x_j - g_j)| at x in long double, g from the model's Jacobians (the scaling, taken at x0, cancels)."""
    s = sc.jacobi_scale(model, np.asarray(x0, dtype=np.float64), jacobi_scaling)
    lin = dr._linearize(model, np.asarray(x, dtype=np.float64), s, LD)
    _, gs = dr._colsq_and_gradient(lin, model.n, LD)
    xt = np.asarray(x, dtype=np.float64).astype(LD)
    pg = np.abs(xt - project(xt - gs / s, np.asarray(lo).astype(LD), np.asarray(hi).astype(LD)))
    return float(np.max(np.where(model.free, pg, 0)))
