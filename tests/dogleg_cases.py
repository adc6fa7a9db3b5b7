"""The cases of the dogleg tests and their reference trajectories (tests/dogleg_reference.py), computed once per process.

Every bundle-adjustment case holds cameras 0 and 1 constant: a Gauss-Newton step at mu = 1e-8 amplifies rounding in the seven
gauge directions of a free problem (tests/test_gpu_step_check.py: test_rejected_step_then_accepted_steps says the same of
near-undamped LM).  Seeds, perturbations and the iterations compared (kmax) were chosen with the reference alone, in double and in
long double, so that the two agree ten times inside the tolerances of the device comparison; tests/test_dogleg_cpu.py asserts
that, and what every case is there to exercise."""
import functools

import numpy as np

from skeres_amd import bal
import step_check as sc
import dogleg_reference as dr

LD = np.longdouble
# the project's tolerances for oracle comparisons (README, round 3): relative, per iteration
TOL = {"cost": 1e-10, "step_norm": 1e-8, "gradient_max_norm": 1e-8, "trust_region_radius": 1e-8, "relative_decrease": 1e-8}
DEFAULT_PERTURB = (1e-2, 1e-1, 1e-1)
CONST_CAMS = (0, 1)

CASES = {
    # one partial workgroup; every step a Gauss-Newton step inside the region
    "small": dict(shape=(6, 40, 200), seed=1, perturb=DEFAULT_PERTURB, kmax=3),
    # the same from radius 1: truncated Cauchy steps, then an interpolated one
    "small-radius-1": dict(shape=(6, 40, 200), seed=1, perturb=DEFAULT_PERTURB, kmax=6, options=dict(initial_trust_region_radius=1.0)),
    # iteration 5 is rejected, 6 re-interpolates and is rejected, 7 re-interpolates and is accepted
    "rejecting": dict(shape=(16, 600, 2600), seed=4, perturb=(0.03, 0.3, 0.5), kmax=7),
    # several workgroups; the smallest size at which the existing tests force plans
    "plans": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=2),
    "plans-jacobi-off": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=2, options=dict(jacobi_scaling=False)),
    # a robust loss, the intrinsics held by a subset parameterization, a constant point
    "robust": dict(shape=(16, 600, 2600), seed=11, perturb=DEFAULT_PERTURB, kmax=4, loss=("huber", 1.0), subset=True, const_pts=(5,)),
    # The three above take Gauss-Newton steps far inside the region (|p| <= 859 against 1e4): a = 0, b = 1, and neither the vector
    # norms nor the Cauchy direction reach anything a test compares.  From radius 1 each takes five truncated Cauchy steps (the
    # radius tripling), then an interpolated one, so that retained points (counted once, as points), diag far from 1 (Jacobi
    # scaling off) and held coordinates (a zero entry of the Cauchy direction) decide the trajectory; "robust-radius-1" goes on to
    # a Gauss-Newton step.
    "plans-radius-1": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=6, options=dict(initial_trust_region_radius=1.0)),
    "plans-jacobi-off-radius-1": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=6,
                                      options=dict(jacobi_scaling=False, initial_trust_region_radius=1.0)),
    "robust-radius-1": dict(shape=(16, 600, 2600), seed=11, perturb=DEFAULT_PERTURB, kmax=7, loss=("huber", 1.0), subset=True, const_pts=(5,),
                            options=dict(initial_trust_region_radius=1.0)),
    # The mu loop (mu *= 10 while the damped system is not positive definite), which no case above reaches: the silent co-axial
    # component of tests/failure_cases.py (case i there) appended to "plans".  Its free, exactly zero point columns have the diagonal
    # min_lm_diagonal / (1 / mu) = 2^-1075 R* mu with R* = 2^12, which rounds to 0 — a zero pivot — exactly where R* mu <= 1: iteration 1
    # fails at mu = 1e-8 .. 1e-4 (R* mu <= 0.41) and factors at 1e-3 (4.1); an accepted step sets mu = 2 mu / 10, so iteration 2 fails at
    # 2e-4 (0.82) and factors at 2e-3, iteration 3 factors at 4e-4 (1.64) at once, iteration 4 fails at 8e-5 and factors at 8e-4: every
    # decision at least 18 % from the threshold, where the roundings of mu and of 1 / mu are 1e-16.  No camera is held here: a held
    # coordinate is inert, its diagonal under this min_lm_diagonal is subnormal, and wave_potrf32 takes the rcp of a camera pivot
    # (tests/failure_cases.py says more); at mu >= 4e-4 the damping keeps the gauge directions far above rounding.
    "i-dogleg": dict(shape=(150, 3000, 14000), seed=5, perturb=(1e-3, 1e-2, 1e-2), kmax=4, silent="middle", const_cams=(),
                     options=dict(min_lm_diagonal=2.0 ** (12 - 1075), zero_columns_in_ieee_double=True),
                     solves=(6, 2, 1, 2), mus=(1e-3, 2e-3, 4e-4, 8e-4)),
}
REFERENCE_ONLY_OPTIONS = ("zero_columns_in_ieee_double",)


@functools.lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    prob = bal.generate(*c["shape"], seed=c["seed"], perturb=c["perturb"])
    if c.get("silent"):
        prob = silent_component(name)[0]
    return prob


@functools.lru_cache(maxsize=None)
def silent_component(name):
    """(the problem with the silent component appended, the columns of x that belong to the component)."""
    import failure_cases as fc   # (imports this module: not at the top)
    c = CASES[name]
    prob, comp = fc._with_silent_component(bal.generate(*c["shape"], seed=c["seed"], perturb=c["perturb"]), c["silent"])
    nc = 9 * prob.num_cameras
    return prob, [9 * a + k for a in comp["cameras"] for k in range(9)] + [nc + 3 * q + k for q in comp["on_axis"] + comp["off_axis"] for k in range(3)]


def masks(name):
    c, prob = CASES[name], problem(name)
    cam_mask = np.full(prob.num_cameras, 0b111000000 if c.get("subset") else 0, dtype=np.int32)
    cam_mask[list(c.get("const_cams", CONST_CAMS))] = 0x1ff
    pt_mask = np.zeros(prob.num_points, dtype=np.int32)
    pt_mask[list(c.get("const_pts", ()))] = 7
    return cam_mask, pt_mask


def model(name):
    cam_mask, pt_mask = masks(name)
    return sc.BalModel(problem(name), loss=CASES[name].get("loss"), cam_mask=cam_mask, pt_mask=pt_mask)


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False):
    """(x, log) of the reference on case `name`; shared by the tests, not to be modified."""
    c, prob = CASES[name], problem(name)
    o = dict(c.get("options", {}))
    o["max_num_iterations"] = c["kmax"]
    return dr.solve(model(name), dr.bal_cost(prob, c.get("loss")), prob.parameters, o, dtype=LD if long_double else np.float64,
                    schur=(prob.num_cameras, prob.num_points))


# The dense Jacobian path: EX/Powell.scala (ten Gauss-Newton steps) and EX/CurveFitting.scala (from m = c = 0 the Gauss-Newton step
# is rejected ten times, the radius halving down to it; the eleventh candidate, a truncated Cauchy step, is rejected too and the
# twelfth accepted: eleven candidates from one factorisation).
DENSE_CASES = {"powell": dict(kmax=10), "curve-fitting": dict(kmax=14)}


def dense_problem(name):
    """(block sizes, [(functor, consts, parameter blocks, loss)], x0)."""
    import oracle
    if name == "powell":
        blocks = [(oracle.POWELL_F1, [], [0, 1], None), (oracle.POWELL_F2, [], [2, 3], None), (oracle.POWELL_F3, [], [1, 2], None),
                  (oracle.POWELL_F4, [], [0, 3], None)]
        return [1, 1, 1, 1], blocks, np.array([3.0, -1.0, 0.0, 1.0])
    from helpers import curve_fitting_data
    return [1, 1], [(oracle.EXPONENTIAL, [xv, yv], [0, 1], None) for xv, yv in curve_fitting_data()], np.zeros(2)


@functools.lru_cache(maxsize=None)
def dense_reference(name, long_double=False):
    sizes, blocks, x0 = dense_problem(name)
    m = sc.BlocksModel(sizes, blocks)
    return dr.solve(m, dr.blocks_cost(m), x0, dict(max_num_iterations=DENSE_CASES[name]["kmax"]), dtype=LD if long_double else np.float64)


def close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def compare_logs(log, ref, kmax, tol=TOL, factor=1.0, show=None):
    """Asserts the accepted / rejected pattern and every compared field of iterations 0..kmax; prints each figure first when asked to."""
    assert len(log) == len(ref) == kmax + 1, (len(log), len(ref))
    for k in range(kmax + 1):
        if show:
            print("%s k=%d" % (show, k), " ".join("%s %.17g / %.17g" % (f, log[k][f], ref[k][f]) for f in tol), flush=True)
    for k in range(kmax + 1):
        assert bool(log[k]["step_is_valid"]) == bool(ref[k]["step_is_valid"]), k
        assert bool(log[k]["step_is_successful"]) == bool(ref[k]["step_is_successful"]), k
        for f, t in tol.items():
            assert close(log[k][f], ref[k][f], t * factor), (k, f, log[k][f], ref[k][f])
