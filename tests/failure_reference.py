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

Option zero_columns_in_ieee_double (case i of tests/failure_cases.py only; absent, nothing changes): a column of the scaled Jacobian
that is exactly zero, with a zero gradient entry, has min_lm_diagonal / radius on its diagonal and nothing else in its row.  That
quotient is formed in IEEE double in BOTH precisions of the reference — where it underflows to 0 the system is not positive definite
and the solve is not valid; long double would not underflow there, and the underflow is what the case is about — and where it is
positive the unknown is 0 whatever the value (the row is decoupled and its right-hand side is 0), so the solve proceeds with a unit
diagonal there: a subnormal pivot never enters the reference's own arithmetic.  Each entry then carries radius_used,
radius_used_exact, zero_columns, zero_quotient and zero_quotient_over_half_ulp (the exact quotient over 2^-1075).  cost_of: the cost
where a robust loss makes it something else than 1/2 sum of the squared corrected residuals.

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


def _evaluate(model, x, s, T, jac, cost_of=None):
    """(cost, lin) at x with the columns scaled by s, or None where the evaluation fails (the module's docstring).  cost_of: x -> the
    cost, where 1/2 sum r^2 of the model's residuals is not it (a robust loss: the model's residuals are the corrected ones, whose
    squares sum to something else than sum rho(|r|^2))."""
    if hasattr(model, "failed") and model.failed(x, jac):
        return None
    with np.errstate(all="ignore"):
        lin = dr._linearize(model, x, s, T)
        for r, terms in lin:
            if not np.all(np.isfinite(r)) or (jac and not all(np.all(np.isfinite(J)) for J, _ in terms)):
                return None
        cost = float(sum(np.sum(r * r) for r, _ in lin) / 2) if cost_of is None else float(cost_of(x))
    return (cost, lin) if np.isfinite(cost) else None


def _zero_column_quotient(colsq, gs, min_lm_diagonal, radius):
    """The columns of the scaled Jacobian that are exactly zero (with them their gradient entries), min_lm_diagonal / radius formed in
    IEEE double whatever the precision of the run — where it underflows to 0 the pivot of such a column is 0 and the system is not
    positive definite: that underflow is what case i is about, and long double has none there — and the exact quotient in units of
    2^-1075, half the smallest subnormal double: it rounds to 0 (ties to even) exactly where that figure is <= 1."""
    zero = (colsq == 0) & (gs == 0)
    with np.errstate(under="ignore"):
        quotient = float(np.float64(min_lm_diagonal) / np.float64(radius))
    return zero, quotient, float(LD(min_lm_diagonal) / LD(radius) / LD(2) ** -1075)


def solve(model, x0, options=None, dtype=np.float64, schur=None, cost_of=None, defect=None):
    """defect (tests/test_termination_cpu.py: what the termination brackets must reject; absent, nothing changes): a dict of
    xnorm (x -> the norm the parameter test uses instead of |x|), gradient_strict (< in the gradient test), radius_not_strict (<= in
    the radius test), function_first (the function test before the parameter test), after_acceptance (a tolerance exit returns the
    candidate), no_exit_entry (a tolerance exit logs nothing), exit_entry_successful (its entry is marked successful)."""
    T = LD if dtype is LD else np.float64
    defect = defect or {}
    o = dict(DEFAULTS)
    o.update(options or {})
    n = model.n
    x = np.array(x0, dtype=np.float64)
    out = dict(x=x, log=[], termination=NO_CONVERGENCE, message="", num_successful_steps=0, num_unsuccessful_steps=0, final_cost=None, reached=set())

    def done(termination, message, x, final_cost):
        out.update(x=x, termination=termination, message=message, final_cost=final_cost)
        out["reached"] = frozenset(out["reached"])
        return out

    ev = _evaluate(model, x, np.ones(n, dtype=T), T, True, cost_of)
    if ev is None:
        out["reached"].add("initial-evaluation-failed")
        return done(FAILURE, MSG_INITIAL, x, None)
    c, lin = ev
    s = np.ones(n, dtype=T)
    if o["jacobi_scaling"]:
        s = (1 / (1 + np.sqrt(dr._colsq_and_gradient(lin, n, T)[0]))).astype(T)
        c, lin = _evaluate(model, x, s, T, True, cost_of)

    def reductions(lin, x):
        with np.errstate(all="ignore"):
            colsq, gs = dr._colsq_and_gradient(lin, n, T)
        xnorm = float(defect["xnorm"](x)) if "xnorm" in defect else float(np.sqrt(np.sum(x.astype(T) ** 2)))
        return colsq, gs, float(np.max(np.abs(gs / s))), xnorm

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
        if gmax < o["gradient_tolerance"] if defect.get("gradient_strict") else gmax <= o["gradient_tolerance"]:
            return done(CONVERGENCE, "Gradient tolerance reached. Gradient max norm: %e <= %e" % (gmax, o["gradient_tolerance"]), x, c)
        if radius <= o["min_trust_region_radius"] if defect.get("radius_not_strict") else radius < o["min_trust_region_radius"]:
            return done(CONVERGENCE, "Minimum trust region radius reached. Trust region radius: %e <= %e" % (radius, o["min_trust_region_radius"]), x, c)
        iteration += 1
        ok = True
        with np.errstate(all="ignore"):
            D2 = np.clip(colsq, T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"])) / radius
            zero_ok, info = True, {}
            if o.get("zero_columns_in_ieee_double"):
                zero, quotient, ratio = _zero_column_quotient(colsq, gs, o["min_lm_diagonal"], radius)
                info = dict(radius_used=float(radius), radius_used_exact=radius_exact, zero_columns=int(np.count_nonzero(zero)),
                                   zero_quotient=quotient, zero_quotient_over_half_ulp=ratio)
                zero_ok = not zero.any() or quotient > 0.0
                D2[zero] = 1   # (a decoupled unknown with right-hand side 0: y_j = 0 under any positive diagonal)
            try:
                if not zero_ok:
                    raise dr.NotPositiveDefinite()
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
                entry(valid=0, success=0, **info)
                out["reached"].add("too-many-invalid-steps")
                return done(FAILURE, MSG_INVALID % o["max_num_consecutive_invalid_steps"], x, c)
            radius = radius / T(decrease_factor)
            decrease_factor *= 2.0
            entry(valid=0, success=0, **info)
            continue
        invalid = 0
        x_new = (x.astype(T) + step * s).astype(np.float64)
        cand = _evaluate(model, x_new, s, T, False, cost_of)
        new_cost = DBL_MAX if cand is None else cand[0]
        extra = dict(info, model_cost_change=float(mcc), candidate=x_new, candidate_failed=cand is None, previous=x)
        if cand is None:
            out["reached"].add("candidate-failed")
        cost_change = c - new_cost
        step_norm = float(np.sqrt(np.sum((x.astype(T) - x_new.astype(T)) ** 2)))
        def tolerance_exit(message):
            if not defect.get("no_exit_entry"):
                entry(cost_change, step_norm, 0.0, 1, 1 if defect.get("exit_entry_successful") else 0, **extra)
            return done(CONVERGENCE, message, x_new if defect.get("after_acceptance") else x, c)

        by_parameter = step_norm <= o["parameter_tolerance"] * (xnorm + o["parameter_tolerance"])
        by_function = abs(cost_change) <= o["function_tolerance"] * c
        if by_parameter and not (defect.get("function_first") and by_function):
            return tolerance_exit("Parameter tolerance reached. Relative step_norm: %e <= %e." % (step_norm / (xnorm + o["parameter_tolerance"]), o["parameter_tolerance"]))
        if by_function:
            return tolerance_exit("Function tolerance reached. |cost_change|/cost: %e <= %e" % (abs(cost_change) / c, o["function_tolerance"]))
        rho = cost_change / float(mcc)
        if rho > o["min_relative_decrease"]:
            ev = _evaluate(model, x_new, s, T, True, cost_of)
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
