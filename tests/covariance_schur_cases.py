"""The cases of the covariance tests with the Schur elimination (tests/test_covariance_schur_cpu.py, tests/test_gpu_covariance_schur.py):
covariance_cases.CASES unchanged, and two bundle-adjustment shapes built by hand as covariance_cases._bal_duplicate builds its
BalProblem (cameras on the trajectory of skeres_amd.bal.generate, observations projected by bal.snavely_project plus noise).

    bal-landmark   70 cameras (0 and 1 constant), 120 points in sliding windows of 4 to 6 cameras (point p: 4 + p % 3 cameras from
                   camera 37 p mod 70 on, wrapping round, so every camera sees 7 to 9 of them) and point 120, the landmark, seen by all
                   70: N = 68 * 9 + 121 * 3 = 975.  Every camera has more neighbours than any window point, so E is the 121 points
                   (the landmark last, once its 68 cameras are in F) and n_F = 612.  The landmark's (e, e) pair has 70 terms: two
                   parts; its diagonal block sums 68^2 tile products.  kappa_2 of the scaled normal matrix: 6.3e5, found with the
                   reference alone (chain: 8.9e5).
    bal-wide       8 cameras (0 and 1 constant), 11 000 points seen by 3 cameras each: N = 54 + 33 000 = 33 054 columns, which the
                   dense route refuses; n_F = 54.  Its reference is the elimination restatement alone."""
import functools

import numpy as np

from skeres_amd import bal
import covariance_cases as vc
import covariance_reference as cv
import covariance_schur_reference as sr

LD = np.longdouble
LANDMARK_CAMERAS, LANDMARK_POINTS = 70, 120
WIDE_CAMERAS, WIDE_POINTS = 8, 11000


def _hand_bal(C, tracks, seed):
    """A BalProblem of C cameras and one point per track (its cameras), geometry as bal.generate's."""
    rng = np.random.default_rng(seed)
    P = len(tracks)
    cam_x = 0.02 * np.arange(C) + rng.normal(0, 0.02, C)
    centers = np.stack([cam_x, rng.normal(0, 0.3, C), 6.0 + rng.normal(0, 0.3, C)], axis=1)
    cams = np.zeros((C, 9))
    cams[:, 0:3] = rng.normal(0, 0.08, (C, 3))
    cams[:, 6] = rng.uniform(400, 1200, C)
    cams[:, 7] = rng.normal(0, 3e-7, C)
    cams[:, 8] = rng.normal(0, 6e-13, C)
    cams[:, 3:6] = -bal._rotate(cams[:, 0:3], centers)[0]
    cam_idx = np.concatenate([np.asarray(t, dtype=np.int64) for t in tracks])
    pt_idx = np.repeat(np.arange(P, dtype=np.int64), [len(t) for t in tracks])
    px = np.array([np.mean(cam_x[np.asarray(t)]) for t in tracks]) + rng.normal(0, 0.5, P)
    pts = np.stack([px, rng.normal(0, 1.0, P), np.clip(rng.normal(0, 1.0, P), -3, 3)], axis=1)
    proj, depth = bal.snavely_project(cams[cam_idx], pts[pt_idx])
    assert (depth < 0).all()
    obs = proj + rng.normal(0, 0.5, proj.shape)
    cams0, pts0 = cams.copy(), pts + rng.uniform(-1e-2, 1e-2, (P, 3))
    cams0[:, 0:3] += rng.uniform(-1e-3, 1e-3, (C, 3))
    cams0[:, 3:6] += rng.uniform(-1e-2, 1e-2, (C, 3))
    return bal.BalProblem(C, P, cam_idx.astype(np.int32), pt_idx.astype(np.int32), np.ascontiguousarray(obs), np.concatenate([cams0.ravel(), pts0.ravel()]))


def _bal_landmark():
    C, P = LANDMARK_CAMERAS, LANDMARK_POINTS
    tracks = [[(37 * p + j) % C for j in range(4 + p % 3)] for p in range(P)] + [list(range(C))]
    prob = _hand_bal(C, tracks, seed=5)
    cam, pt, landmark = (lambda i: i), (lambda p: C + p), C + P
    return vc._bal_case("bal-landmark", prob, pairs=[(landmark, landmark), (landmark, pt(17)), (landmark, cam(5)), (cam(5), cam(40)), (cam(0), cam(0))])


def _bal_wide():
    C, P = WIDE_CAMERAS, WIDE_POINTS
    rng = np.random.default_rng(9)
    tracks = [sorted(rng.choice(C, size=3, replace=False).tolist()) for _ in range(P)]
    prob = _hand_bal(C, tracks, seed=6)
    cam, pt = (lambda i: i), (lambda p: C + p)
    return vc._bal_case("bal-wide", prob, pairs=[(cam(2), cam(2)), (cam(2), cam(5)), (cam(7), cam(7)), (cam(3), pt(100)), (pt(10999), cam(6)), (pt(0), pt(0)),
                                                 (pt(5000), pt(77))])


CASES = dict(vc.CASES)
CASES.update({"bal-landmark": _bal_landmark, "bal-wide": _bal_wide})
DENSE = sorted(set(CASES) - {"bal-wide"})          # the cases the dense route takes


@functools.lru_cache(maxsize=None)
def case(name):
    return vc.case(name) if name in vc.CASES else CASES[name]()


@functools.lru_cache(maxsize=None)
def problem_order(name):
    """Per block of the case its index in the device problem's own order (first mention): the tie-break of the greedy visit."""
    c = case(name)
    problem, params, keep = c.build()
    order = [problem.parameterBlockIndex(h) for h in vc.handles(c, params)]
    assert sorted(order) == list(range(len(order)))
    return tuple(order)


@functools.lru_cache(maxsize=None)
def model_coo(name, with_loss=True):
    """The independent reference's Jacobian in long double; shared, not to be modified."""
    c = case(name)
    return sr.model_coo(c.model(with_loss), c.x, c.blocks, LD)


@functools.lru_cache(maxsize=None)
def reference(name, long_double=False, with_loss=True):
    """The restatement of the route on the reference's own Jacobian (with kappa_2 in the long-double run); shared."""
    c = case(name)
    T = LD if long_double else np.float64
    return sr.eliminate(model_coo(name, with_loss), c.blocks, c.x, c.offsets, c.pairs, T, kappa=long_double, order=problem_order(name))


@functools.lru_cache(maxsize=None)
def self_deviation(name, with_loss=True):
    """D: the float64 restatement of this route against its long-double run, in the metric."""
    return cv.deviation(reference(name, False, with_loss), reference(name, True, with_loss), case(name).pairs)


def tolerance(name, with_loss=True):
    """The bound of the inversion test: max(16 D, 64 u)."""
    return max(16 * self_deviation(name, with_loss), 64 * cv.U)


def options(on=True):
    import skeres_amd as sk
    o = sk.Covariance.Options()
    o.schurElimination(on)
    return o
