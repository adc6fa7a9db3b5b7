"""The Levenberg-Marquardt loop of oracle/lm.cpp (minimize(): published Ceres' TrustRegionMinimizer) restated in numpy WITH its
failure paths: evaluations that cannot be made, candidates that cannot be evaluated, linear solves that are not valid.  CPU only:
numpy, the models of tests/step_check.py (a TapeModel for recorded functors, CallableModel below for host-callback blocks) and the
linear algebra tests/dogleg_reference.py shares; neither the oracle nor anything of skeres_amd's native library.

    evaluation with Jacobian   fails if a block reports failure, or a residual or a Jacobian entry is not finite, or the cost
                               1/2 sum r^2 is not finite (residuals near 1e154 and beyond: no case has them)
    cost-only evaluation       fails if a block reports failure or a residual (or the cost) is not finite
    initial evaluation fails   FAILURE "Initial residual and Jacobian evaluation failed.", nothing logged, x0 returned untouched
    linear solve not valid     (not positive definite, a non-finite y, model cost change not > 0): logged with valid = 0; the radius
                               /2, /4, /8, ...; FAILURE after max_num_consecutive_invalid_steps of them, x the last accepted point
    candidate cannot be        a VALID step of cost DBL_MAX: cost_change = cost - DBL_MAX, rho < 0, rejected, the radius as above,
    evaluated                  the counter of invalid steps reset
    evaluation after an        FAILURE "Residual and Jacobian evaluation failed.", the iteration NOT logged and not counted as
    accepted step fails        successful, x the accepted candidate, the final cost not pinned (lm.cpp leaves what evaluate() wrote)

solve() returns a dict: x, log (the device's fields per logged iteration plus model_cost_change, candidate (the point tried),
candidate_failed, radius_exact (no update of the radius so far went through rho: see failure_cases.compare)), termination, message, num_successful_steps, num_unsuccessful_steps, final_cost (None: not pinned), reached (the
set of branches the run went through: the names of BRANCHES)."""
import numpy as np

import step_check as sc
import dogleg_reference as dr

LD = np.longdouble
DBL_MAX = float(np.finfo(np.float64).max)
DEFAULTS = dict(dr.DEFAULTS)
CONVERGENCE, NO_CONVERGENCE, FAILURE = "CONVERGENCE", "NO_CONVERGENCE", "FAILURE"
BRANCHES = ("initial-evaluation-failed", "evaluation-after-accept-failed", "candidate-failed", "invalid-step", "too-many-invalid-steps",
            "accepted", "rejected")
MSG_INITIAL = "Initial residual and Jacobian evaluation failed."
MSG_EVALUATION = "Residual and Jacobian evaluation failed."
MSG_INVALID = "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d"


class CallableModel(sc._Model):
    """Host-callback residual blocks: blocks = [(f, [offset of each parameter block in x], [their sizes])] with
    f(params, want_jacobians) -> (ok, residuals [k], [Jacobian [k, size] per parameter block] or None)."""

    def __init__(self, n, blocks):
        self.n = int(n)
        self.blocks = blocks
        self.free = np.ones(self.n, dtype=bool)
        self.kind = np.zeros(self.n, dtype=np.int8)

    def _params(self, x, offs, sizes):
        return [np.array(x[o:o + s], dtype=np.float64) for o, s in zip(offs, sizes)]

    def failed(self, x, jac):
        """Does a block report failure at x (for an evaluation with / without Jacobians)?"""
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            return any(not f(self._params(x, offs, sizes), jac)[0] for f, offs, sizes in self.blocks)

    def chunks(self, x):
        x = np.asarray(x, dtype=np.float64)
        for f, offs, sizes in self.blocks:
            with np.errstate(all="ignore"):
                _, r, J = f(self._params(x, offs, sizes), True)
            yield (np.asarray(r, dtype=LD)[None, :],
                   [(np.asarray(J[q], dtype=LD)[None, :, :], np.array([offs[q]], dtype=np.int64)) for q in range(len(offs))])


def _evaluate(model, x, s, T, jac):
    """(cost, lin) at x with the columns scaled by s, or None where the evaluation fails (the module's docstring)."""
    if hasattr(model, "failed") and model.failed(x, jac):
        return None
    with np.errstate(all="ignore"):
        lin = dr._linearize(model, x, s, T)
        for r, terms in lin:
            if not np.all(np.isfinite(r)) or (jac and not all(np.all(np.isfinite(J)) for J, _ in terms)):
                return None
        cost = float(sum(np.sum(r * r) for r, _ in lin) / 2)
    return (cost, lin) if np.isfinite(cost) else None


def solve(model, x0, options=None, dtype=np.float64, schur=None):
    T = LD if dtype is LD else np.float64
    o = dict(DEFAULTS)
    o.update(options or {})
    n = model.n
    x = np.array(x0, dtype=np.float64)
    out = dict(x=x, log=[], termination=NO_CONVERGENCE, message="", num_successful_steps=0, num_unsuccessful_steps=0, final_cost=None, reached=set())

    def done(termination, message, x, final_cost):
        out.update(x=x, termination=termination, message=message, final_cost=final_cost)
        out["reached"] = frozenset(out["reached"])
        return out

    ev = _evaluate(model, x, np.ones(n, dtype=T), T, True)
    if ev is None:
        out["reached"].add("initial-evaluation-failed")
        return done(FAILURE, MSG_INITIAL, x, None)
    c, lin = ev
    s = np.ones(n, dtype=T)
    if o["jacobi_scaling"]:
        s = (1 / (1 + np.sqrt(dr._colsq_and_gradient(lin, n, T)[0]))).astype(T)
        c, lin = _evaluate(model, x, s, T, True)

    def reductions(lin, x):
        with np.errstate(all="ignore"):
            colsq, gs = dr._colsq_and_gradient(lin, n, T)
        return colsq, gs, float(np.max(np.abs(gs / s))), float(np.sqrt(np.sum(x.astype(T) ** 2)))

    colsq, gs, gmax, xnorm = reductions(lin, x)
    radius = T(o["initial_trust_region_radius"])
    decrease_factor = 2.0
    radius_exact = True   # every update so far was a division by a power of two or the multiplication by 3: no rounding of rho in it

    def entry(cost_change=0.0, step_norm=0.0, rho=0.0, valid=1, success=1, **extra):
        e = dict(cost=c, cost_change=float(cost_change), gradient_max_norm=gmax, step_norm=float(step_norm), relative_decrease=float(rho),
                 trust_region_radius=float(radius), step_is_valid=valid, step_is_successful=success, radius_exact=radius_exact)
        e.update(extra)
        out["log"].append(e)

    entry()
    iteration = invalid = 0
    while True:
        if iteration >= o["max_num_iterations"]:
            return done(NO_CONVERGENCE, "Maximum number of iterations reached. Number of iterations: %d." % iteration, x, c)
        if gmax <= o["gradient_tolerance"]:
            return done(CONVERGENCE, "Gradient tolerance reached. Gradient max norm: %e <= %e" % (gmax, o["gradient_tolerance"]), x, c)
        if radius < o["min_trust_region_radius"]:
            return done(CONVERGENCE, "Minimum trust region radius reached. Trust region radius: %e <= %e" % (radius, o["min_trust_region_radius"]), x, c)
        iteration += 1
        ok = True
        with np.errstate(all="ignore"):
            D2 = np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])) / radius
            try:
                y = dr._gauss_newton_schur(lin, schur[0], schur[1], D2, gs, T) if schur else dr._gauss_newton_dense(lin, n, D2, gs, T)
                ok = bool(np.all(np.isfinite(y)))
            except (dr.NotPositiveDefinite, np.linalg.LinAlgError):
                ok = False
            if ok:
                step = -y
                m = dr._times(lin, step)
                mcc = -sum(np.sum(mm * (r + mm / 2)) for mm, (r, _) in zip(m, lin))
                ok = bool(mcc > 0)
        if not ok:
            invalid += 1
            out["reached"].add("invalid-step")
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                entry(valid=0, success=0)
                out["reached"].add("too-many-invalid-steps")
                return done(FAILURE, MSG_INVALID % o["max_num_consecutive_invalid_steps"], x, c)
            radius = radius / T(decrease_factor)
            decrease_factor *= 2.0
            entry(valid=0, success=0)
            continue
        invalid = 0
        x_new = (x.astype(T) + step * s).astype(np.float64)
        cand = _evaluate(model, x_new, s, T, False)
        new_cost = DBL_MAX if cand is None else cand[0]
        extra = dict(model_cost_change=float(mcc), candidate=x_new, candidate_failed=cand is None, previous=x)
        if cand is None:
            out["reached"].add("candidate-failed")
        cost_change = c - new_cost
        step_norm = float(np.sqrt(np.sum((x.astype(T) - x_new.astype(T)) ** 2)))
        if step_norm <= o["parameter_tolerance"] * (xnorm + o["parameter_tolerance"]):
            entry(cost_change, step_norm, 0.0, 1, 0, **extra)
            return done(CONVERGENCE, "Parameter tolerance reached. Relative step_norm: %e <= %e." % (step_norm / (xnorm + o["parameter_tolerance"]), o["parameter_tolerance"]), x, c)
        if abs(cost_change) <= o["function_tolerance"] * c:
            entry(cost_change, step_norm, 0.0, 1, 0, **extra)
            return done(CONVERGENCE, "Function tolerance reached. |cost_change|/cost: %e <= %e" % (abs(cost_change) / c, o["function_tolerance"]), x, c)
        rho = cost_change / float(mcc)
        if rho > o["min_relative_decrease"]:
            ev = _evaluate(model, x_new, s, T, True)
            if ev is None:
                out["reached"].add("evaluation-after-accept-failed")
                return done(FAILURE, MSG_EVALUATION, x_new, None)
            x = x_new
            c, lin = ev
            colsq, gs, gmax, xnorm = reductions(lin, x)
            shrink = 1 - (2 * T(rho) - 1) ** 3
            radius_exact = radius_exact and bool(shrink < T(1) / 3)   # (else the new radius carries the rounding of rho)
            radius = min(T(o["max_trust_region_radius"]), radius / max(T(1) / 3, shrink))
            decrease_factor = 2.0
            out["num_successful_steps"] += 1
            out["reached"].add("accepted")
            entry(cost_change, step_norm, rho, 1, 1, **extra)
        else:
            radius = radius / T(decrease_factor)
            decrease_factor *= 2.0
            out["num_unsuccessful_steps"] += 1
            out["reached"].add("rejected")
            entry(cost_change, step_norm, rho, 1, 0, **extra)


def discrete(run):
    """The discrete fields of a run (the reference's dict, or a device run brought to the same shape: failure_cases.device_run)."""
    msg = run["message"]   # (a FAILURE's message is compared whole, a figure-carrying one up to its figure)
    return dict(termination=run["termination"], message_prefix=msg if run["termination"] == FAILURE else msg.split(":")[0], num_logged=len(run["log"]),
                num_successful_steps=run["num_successful_steps"], num_unsuccessful_steps=run["num_unsuccessful_steps"],
                valid=[int(bool(e["step_is_valid"])) for e in run["log"]], successful=[int(bool(e["step_is_successful"])) for e in run["log"]])
