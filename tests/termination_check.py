"""Every exit of the trust-region loop (SolverBase::step: iteration limit, gradient tolerance, minimum trust-region radius,
parameter tolerance, function tolerance), bracketed at its threshold from a runner's OWN log.  numpy only: neither skeres_amd's
native library nor the oracle is imported here.

A runner is run(options) -> dict with the fields failure_cases.device_run and failure_reference.solve share: x, log, termination,
message, num_successful_steps, num_unsuccessful_steps, final_cost; options holds max_num_iterations and the four thresholds
(gradient_tolerance, parameter_tolerance, function_tolerance, min_trust_region_radius), everything else is the case's.  Optional
fields: xs (x after every logged iteration: it spares the runs that would fetch them) and idempotent (the stepping API was stepped
once more after the exit, reported done again and changed nothing).

Nothing here compares a trajectory with a reference trajectory.  The baseline is the runner's run with all four thresholds 0 and
max_num_iterations = K; runs with max_num_iterations = k give x_k, and their cost, step_norm, gradient_max_norm and
trust_region_radius must be a bitwise prefix of the baseline's.  Each exit then gets a k at which its quantity is a running minimum
by a factor of two (so it cannot fire earlier), an "in" threshold at which the run must end for that reason at that iteration, and
an "out" threshold, an ulp or so away, at which it must not.  The quantities: gradient_max_norm_k; |cost_change_k| / cost_{k-1}; and
for the parameter exit the tolerance p_k at which its test flips (below) — step_norm_k / |x_{k-1}| wherever that is small, and still
what decides where it is not (a start at the origin: p_1 = sqrt(step_norm_1)).

    gradient    in  gradient_tolerance = gmax_k exactly                   out nextafter(gmax_k, 0)
    radius      in  min_trust_region_radius = nextafter(radius_k, inf)    out radius_k exactly (the test is strict)
    function    f = |cost_change_k| / cost_{k-1} in double: in f (1 + 2^-50), out f (1 - 2^-50) — the quotient and the solver's product
                function_tolerance * cost round once each, at most 2 ulp together; the margin is 4 ulp
    parameter   xn = |x_{k-1}| in long double from the runner's own x_{k-1}, sn the logged step_norm_k, p the positive root of
                p (xn + p) = sn: in p (1 + delta), out p (1 - delta), delta = (n + 8) 2^-53 with n the ambient parameter count — a sum
                of n squares in any order is within n u of exact, its root within half of that, the rest covers the rounding of p,
                of the product and of the sum.  This is the one place where a value the solver never shows (its |x|) is held.

The order of the tests, three runs: parameter and function thresholds both "in" at the first k at which both quantities are running
minima by a quarter (the parameter's message; a case whose trajectory has no such k leaves this run to the others and says so);
max_num_iterations = k with gradient_tolerance = gmax_k (the limit's message); gradient_tolerance = gmax_k with a
min_trust_region_radius above radius_k (the gradient's message).  The last one needs a k at which BOTH tests hold for the first
time: the radius test holds at k and at no j < k only where radius_k is below every earlier radius, which the k of the gradient
bracket seldom is (accepted steps grow the radius) — so it is run at the largest k <= K - 1 at which gmax_k and radius_k are both
strictly below every earlier value (k = 0 always is), with min_trust_region_radius = min(2 radius_k, the smallest earlier radius).
"""
import re

import numpy as np

LD = np.longdouble
ZERO = dict(gradient_tolerance=0.0, parameter_tolerance=0.0, function_tolerance=0.0, min_trust_region_radius=0.0)
PREFIX_FIELDS = ("cost", "step_norm", "gradient_max_norm", "trust_region_radius")
ENTRY_FIELDS = PREFIX_FIELDS + ("cost_change", "relative_decrease")
CONVERGENCE, NO_CONVERGENCE = "CONVERGENCE", "NO_CONVERGENCE"
MSG_LIMIT = "Maximum number of iterations reached. Number of iterations: %d."
MSG_GRADIENT = "Gradient tolerance reached. Gradient max norm: %e <= %e"
MSG_RADIUS = "Minimum trust region radius reached. Trust region radius: %e <= %e"
MSG_PARAMETER = "Parameter tolerance reached. Relative step_norm: %e <= %e."
MSG_FUNCTION = "Function tolerance reached. |cost_change|/cost: %e <= %e"
EXITS = ("gradient", "radius", "function", "parameter")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def delta(n):
    return (n + 8) * 2.0 ** -53


def xnorm(x):
    """|x| in long double."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    return np.sqrt(np.sum(x * x))


def parameter_threshold(xn, sn):
    """The p with p (xn + p) = sn, in long double: (-xn + sqrt(xn^2 + 4 sn)) / 2 written without its cancellation (p / xn is 1e-4 and
    less: the difference would lose that many of long double's digits, more than delta leaves)."""
    xn, sn = LD(xn), LD(sn)
    return 2 * sn / (xn + np.sqrt(xn * xn + 4 * sn))


def _entries_equal(a, b, fields=ENTRY_FIELDS):
    return (all(same(a[f], b[f]) for f in fields) and bool(a["step_is_valid"]) == bool(b["step_is_valid"])
            and bool(a["step_is_successful"]) == bool(b["step_is_successful"]))


def _counters(log, k):
    """(successful, unsuccessful) steps among log[1..k]: a valid step that was not accepted is unsuccessful, an invalid one neither."""
    ok = sum(1 for e in log[1:k + 1] if e["step_is_successful"])
    no = sum(1 for e in log[1:k + 1] if e["step_is_valid"] and not e["step_is_successful"])
    return ok, no


def _e_units(text):
    """A %e figure as (its seven digits as an integer, its exponent)."""
    m = re.fullmatch(r"(-?)(\d)\.(\d{6})e([+-]\d+)", text)
    assert m, text
    return int(m.group(2) + m.group(3)), int(m.group(4))


def _e_within_one_unit(a, b):
    (ua, ea), (ub, eb) = _e_units(a), _e_units(b)
    if ea == eb:
        return abs(ua - ub) <= 1
    return {(ua, ea), (ub, eb)} == {(9999999, min(ea, eb)), (1000000, max(ea, eb))} and abs(ea - eb) == 1


class Brackets:
    """The brackets of one case on one runner.  n: the ambient parameter count; K: the baseline's iterations."""

    def __init__(self, run, K, n, show=None):
        self.run, self.K, self.n, self.show = run, int(K), int(n), show
        self.solves = 0
        self._prefix = {}
        self.base = self._solve(max_num_iterations=self.K)
        self._prefix[self.K] = self.base
        self.log = self.base["log"]
        assert self.base["termination"] == NO_CONVERGENCE and self.base["message"] == MSG_LIMIT % self.K, (self.base["termination"], self.base["message"])
        assert len(self.log) == self.K + 1, len(self.log)
        assert all(np.isfinite(e[f]) for e in self.log for f in ENTRY_FIELDS)

    def _solve(self, **o):
        opts = dict(ZERO, max_num_iterations=self.K)
        opts.update(o)
        self.solves += 1
        r = self.run(opts)
        if self.show:
            print(self.show, {k: (v if isinstance(v, int) else "%.17g" % v) for k, v in opts.items()}, "->", r["termination"], repr(r["message"]), "logged", len(r["log"]), flush=True)
        return r

    # ---- the baseline and its prefixes -----------------------------------------------------------------------------------------
    def prefix(self, k):
        """The run with max_num_iterations = k and no threshold: x_k; its log a bitwise prefix of the baseline's."""
        if k not in self._prefix:
            r = self._solve(max_num_iterations=k)
            assert r["termination"] == NO_CONVERGENCE and r["message"] == MSG_LIMIT % k, (k, r["termination"], r["message"])
            self._assert_prefix(r, k)
            xs = self.base.get("xs")
            if xs is not None:
                assert same(r["x"], xs[k]), "x_%d of the baseline's stepping differs from the run of %d iterations" % (k, k)
            self._prefix[k] = r
        return self._prefix[k]

    def _assert_prefix(self, r, k, upto=None):
        """log[0..upto] (default k) of run r bitwise the baseline's."""
        upto = k if upto is None else upto
        assert len(r["log"]) > upto, (len(r["log"]), upto)
        for j in range(upto + 1):
            for f in PREFIX_FIELDS:
                assert same(r["log"][j][f], self.log[j][f]), "%s of iteration %d: %.17g, the baseline's %.17g" % (f, j, r["log"][j][f], self.log[j][f])
            assert _entries_equal(r["log"][j], self.log[j]), (j, r["log"][j], self.log[j])

    def x(self, k):
        xs = self.base.get("xs")
        return np.asarray(xs[k] if xs is not None else self.prefix(k)["x"], dtype=np.float64)

    # ---- the quantities and the choice of k ------------------------------------------------------------------------------------
    def quantity(self, exit, k):
        """The quantity of the exit at iteration k, or None where the exit's test is not reached there (an invalid step)."""
        e = self.log[k]
        if exit == "gradient":
            return float(e["gradient_max_norm"])
        if k == 0 or not e["step_is_valid"]:
            return None
        if exit == "parameter":   # (the tolerance at which the test flips: step_norm / |x| wherever that is small, sqrt(step_norm) at |x| = 0)
            return float(parameter_threshold(xnorm(self.x(k - 1)), e["step_norm"]))
        if exit == "function":
            return abs(e["cost_change"]) / self.log[k - 1]["cost"]
        raise KeyError(exit)

    def is_running_minimum(self, exit, k, factor=2.0):
        q = self.quantity(exit, k)
        if q is None or not q > 0.0:
            return False
        first = 0 if exit == "gradient" else 1
        earlier = [self.quantity(exit, j) for j in range(first, k)]
        return all(v is None or factor * q <= v for v in earlier)

    def choose(self, exit, also=None, factor=2.0):
        """The first k >= 2 (gradient: k <= K - 1, its "out" run logs iteration k + 1) at which the exit's quantity is a running
        minimum by `factor` (also: a second exit for which it must be one too); the radius exit: the first k at which the
        radius is strictly below every earlier one, else 0.  The case fails where there is none."""
        if exit == "radius":
            radii = [e["trust_region_radius"] for e in self.log]
            for k in range(1, self.K + 1):
                if radii[k] < min(radii[:k]):
                    return k
            return 0
        last = self.K - 1 if exit == "gradient" else self.K
        for k in range(2, last + 1):
            if self.is_running_minimum(exit, k, factor) and (also is None or self.is_running_minimum(also, k, factor)):
                return k
        raise AssertionError("no k <= %d at which the %s quantity%s is a running minimum by a factor of %g: %s" % (
            last, exit, " (and the %s one)" % also if also else "", factor, [self.quantity(exit, j) for j in range(self.K + 1)]))

    def thresholds(self, exit, k):
        """(in, out) of the exit at k."""
        e = self.log[k]
        if exit == "gradient":
            g = float(e["gradient_max_norm"])
            return g, float(np.nextafter(g, 0.0))
        if exit == "radius":
            r = float(e["trust_region_radius"])
            return float(np.nextafter(r, np.inf)), r
        if exit == "function":
            f = abs(e["cost_change"]) / self.log[k - 1]["cost"]
            return f * (1 + 2.0 ** -50), f * (1 - 2.0 ** -50)
        p = parameter_threshold(xnorm(self.prefix(k - 1)["x"]), e["step_norm"])
        d = LD(delta(self.n))
        return float(p * (1 + d)), float(p * (1 - d))

    # ---- what a run must leave behind --------------------------------------------------------------------------------------------
    def _assert_idempotent(self, r):
        assert r.get("idempotent", True) is True, "a further step() after the exit changed something or did not report done"

    def assert_limit(self, r, k, entry=True):
        """r ended at the iteration limit k; entry: log[k] is the baseline's, bitwise (k <= K)."""
        assert r["termination"] == NO_CONVERGENCE and r["message"] == MSG_LIMIT % k, (r["termination"], r["message"], k)
        assert len(r["log"]) == k + 1, (len(r["log"]), k)
        if entry and k <= self.K:
            self._assert_prefix(r, k)
            assert same(r["x"], self.x(k)) and same(r["final_cost"], self.log[k]["cost"])
        else:
            self._assert_prefix(r, k - 1)
        self._assert_idempotent(r)

    def assert_start_exit(self, r, k, message):
        """r ended before iteration k + 1 was tried (gradient, radius): everything up to k as the baseline has it."""
        assert r["termination"] == CONVERGENCE, (r["termination"], r["message"])
        assert r["message"] == message, (r["message"], message)
        assert len(r["log"]) == k + 1, (len(r["log"]), k)
        self._assert_prefix(r, k)
        assert same(r["x"], self.prefix(k)["x"]), "x is not x_%d" % k
        assert same(r["final_cost"], self.log[k]["cost"]), (r["final_cost"], self.log[k]["cost"])
        assert (r["num_successful_steps"], r["num_unsuccessful_steps"]) == _counters(self.log, k)
        self._assert_idempotent(r)

    def assert_tolerance_exit(self, r, k, exit, tolerance):
        """r ended inside iteration k by the parameter or the function tolerance."""
        assert r["termination"] == CONVERGENCE, (r["termination"], r["message"])
        e = self.log[k]
        if exit == "function":
            message = MSG_FUNCTION % (abs(e["cost_change"]) / self.log[k - 1]["cost"], tolerance)
            assert r["message"] == message, (r["message"], message)
        else:
            ratio = float(LD(e["step_norm"]) / (xnorm(self.prefix(k - 1)["x"]) + LD(tolerance)))
            message = MSG_PARAMETER % (ratio, tolerance)
            m = re.fullmatch(r"Parameter tolerance reached\. Relative step_norm: (\S+) <= (\S+)\.", r["message"])
            assert m, (r["message"], message)
            assert m.group(2) == "%e" % tolerance and _e_within_one_unit(m.group(1), "%e" % ratio), (r["message"], message)
        assert len(r["log"]) == k + 1, (len(r["log"]), k)
        self._assert_prefix(r, k - 1)
        last = r["log"][k]
        assert same(last["cost_change"], e["cost_change"]) and same(last["step_norm"], e["step_norm"]), (last, e)
        assert bool(last["step_is_valid"]) and not bool(last["step_is_successful"]), last
        assert same(r["x"], self.prefix(k - 1)["x"]), "x is not x_%d" % (k - 1)
        assert same(r["final_cost"], self.log[k - 1]["cost"]), (r["final_cost"], self.log[k - 1]["cost"])
        assert (r["num_successful_steps"], r["num_unsuccessful_steps"]) == _counters(self.log, k - 1)
        self._assert_idempotent(r)

    # ---- the brackets ------------------------------------------------------------------------------------------------------------
    def gradient(self):
        k = self.choose("gradient")
        t_in, t_out = self.thresholds("gradient", k)
        self.assert_start_exit(self._solve(gradient_tolerance=t_in, max_num_iterations=k + 1), k, MSG_GRADIENT % (t_in, t_in))
        self.assert_limit(self._solve(gradient_tolerance=t_out, max_num_iterations=k + 1), k + 1)
        return dict(exit="gradient", k=k, threshold=t_in)

    def radius(self):
        k = self.choose("radius")
        t_in, t_out = self.thresholds("radius", k)
        self.assert_start_exit(self._solve(min_trust_region_radius=t_in), k, MSG_RADIUS % (t_out, t_in))
        self.assert_limit(self._solve(min_trust_region_radius=t_out, max_num_iterations=k + 1), k + 1, entry=k + 1 <= self.K)
        return dict(exit="radius", k=k, threshold=t_in)

    def function(self):
        k = self.choose("function")
        t_in, t_out = self.thresholds("function", k)
        self.assert_tolerance_exit(self._solve(function_tolerance=t_in), k, "function", t_in)
        self.assert_limit(self._solve(function_tolerance=t_out, max_num_iterations=k), k)
        return dict(exit="function", k=k, threshold=t_in)

    def parameter(self):
        k = self.choose("parameter")
        t_in, t_out = self.thresholds("parameter", k)
        assert t_out < t_in
        self.assert_tolerance_exit(self._solve(parameter_tolerance=t_in), k, "parameter", t_in)
        self.assert_limit(self._solve(parameter_tolerance=t_out, max_num_iterations=k), k)
        return dict(exit="parameter", k=k, threshold=t_in, delta=delta(self.n))

    def limit(self):
        """max_num_iterations = k with gradient_tolerance = gmax_k, at the gradient bracket's k: the limit wins."""
        k = self.choose("gradient")
        self.assert_limit(self._solve(gradient_tolerance=self.thresholds("gradient", k)[0], max_num_iterations=k), k)
        return dict(exit="limit", k=k, threshold=self.thresholds("gradient", k)[0])

    def order(self, parameter_before_function=True):
        """parameter_before_function = False: a case whose trajectory has no k that serves both (it says so) runs the other two."""
        k = p_in = f_in = None
        if parameter_before_function:
            # at the first k whose two quantities are both running minima by a quarter: the two exits' own k seldom coincide, and
            # thresholds taken from the runner's own log need no more room than that
            k = self.choose("parameter", also="function", factor=1.25)
            p_in, f_in = self.thresholds("parameter", k)[0], self.thresholds("function", k)[0]
            self.assert_tolerance_exit(self._solve(parameter_tolerance=p_in, function_tolerance=f_in), k, "parameter", p_in)
        # the limit before the gradient test
        kl = self.limit()["k"]
        # the gradient test before the radius test (the module's docstring: where both hold for the first time)
        g = [e["gradient_max_norm"] for e in self.log]
        r = [e["trust_region_radius"] for e in self.log]
        kg = max(j for j in range(self.K) if j == 0 or (g[j] < min(g[:j]) and r[j] < min(r[:j])))
        min_radius = min([2 * r[kg]] + r[:kg])
        assert r[kg] < min_radius
        self.assert_start_exit(self._solve(gradient_tolerance=g[kg], min_trust_region_radius=min_radius, max_num_iterations=kg + 1), kg, MSG_GRADIENT % (g[kg], g[kg]))
        return dict(exit="order", k=(k, kl, kg), threshold=(p_in, f_in, min_radius))

    def all(self):
        return [self.gradient(), self.radius(), self.function(), self.parameter(), self.order()]
