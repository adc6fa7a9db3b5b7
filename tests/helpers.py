"""Shared helpers for the parity tests."""
import numpy as np

import skeres_amd as sk


def bal_problem_to_sk(prob, x0=None, loss=None):
    """Build a skeres_amd Problem the way EX/SimpleBundleAdjuster.scala:134-145 does,
    through the bulk addResidualBlocks call.  Returns (problem, params DoubleArray, loss)."""
    x0 = prob.parameters if x0 is None else x0
    params = sk.RichDoubleArray.fromArray(x0)
    problem = sk.Problem()
    loss = loss if loss is not None else sk.PredefinedLossFunctions.trivialLoss()
    offs = np.stack([9 * prob.camera_index.astype(np.int64),
                     9 * prob.num_cameras + 3 * prob.point_index.astype(np.int64)], axis=1)
    problem.addResidualBlocks(sk.SnavelyReprojectionError.FUNCTOR_ID, prob.observations, loss, params, offs)
    return problem, params, loss


def solve_bal_gpu(prob, x0=None, loss=None, **opts):
    problem, params, loss = bal_problem_to_sk(prob, x0, loss)
    options = sk.Solver.Options()
    options.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
    for k, v in opts.items():
        getattr(options, k)(*v) if isinstance(v, tuple) else getattr(options, k)(v)
    summary = sk.Solver.Summary()
    sk.ceres.solve(options, problem, summary)
    return params.toArray(prob.num_parameters), summary


CURVE_DATA = None


def curve_fitting_data():
    """The 67 (x, y) samples of EX/CurveFitting.scala:22-90 (tests/golden/curve_fitting_data.txt)."""
    global CURVE_DATA
    if CURVE_DATA is None:
        import os
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curve_fitting_data.txt")
        CURVE_DATA = np.loadtxt(path)
    return CURVE_DATA


def robust_curve_fitting_data():
    """The 67 (x, y) samples of EX/RobustCurveFitting.scala:21-90 (tests/golden/robust_curve_fitting_data.txt)."""
    import os
    return np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_curve_fitting_data.txt"))


def sk_loss(spec):
    """oracle-style loss tuple -> skeres_amd LossFunction (None -> None)."""
    L = sk.PredefinedLossFunctions
    if spec is None:
        return None
    kind = spec[0]
    if kind == "composed":
        return L.composedLoss(sk_loss(spec[1]), sk_loss(spec[2]))
    if kind == "scaled":
        return L.scaledLoss(sk_loss(spec[1]), spec[2])
    if kind == "tolerant":
        return L.tolerantLoss(spec[1], spec[2])
    return {"huber": L.huberLoss, "softlone": L.softLOneLoss, "cauchy": L.cauchyLoss, "tukey": L.tukeyLoss}[kind](spec[1])


def bal_from_tracks(num_cameras, tracks, seed=7, sigma_px=0.5, perturb=(1e-2, 1e-1, 1e-1)):
    """A BalProblem from an explicit list of cameras per track (tracks[p] = the cameras that observe point p; a camera listed
    twice is two residual blocks on one (camera, point) pair).  Truth, projection, noise and perturbation as bal.generate
    draws them: cameras on a trajectory along +x looking down -z, each point near the centroid of its cameras."""
    from skeres_amd import bal
    C, P = int(num_cameras), len(tracks)
    rng = np.random.default_rng(seed)
    cam_x = 0.02 * np.arange(C) + rng.normal(0, 0.02, C)
    centers = np.stack([cam_x, rng.normal(0, 0.3, C), 6.0 + rng.normal(0, 0.3, C)], axis=1)
    aa = rng.normal(0, 0.08, (C, 3))
    cams = np.zeros((C, 9))
    cams[:, 0:3] = aa
    cams[:, 6] = rng.uniform(400, 1200, C)
    cams[:, 7] = rng.normal(0, 3e-7, C)
    cams[:, 8] = rng.normal(0, 6e-13, C)
    Rc, _ = bal._rotate(aa, centers)
    cams[:, 3:6] = -Rc
    cam_idx = np.concatenate([np.asarray(t, dtype=np.int64) for t in tracks])
    pt_idx = np.repeat(np.arange(P, dtype=np.int64), [len(t) for t in tracks])
    assert cam_idx.min() >= 0 and cam_idx.max() < C
    px = np.array([cam_x[np.asarray(t)].mean() for t in tracks]) + rng.normal(0, 0.5, P)
    pts = np.stack([px, rng.normal(0, 1.0, P), np.clip(rng.normal(0, 1.0, P), -3, 3)], axis=1)
    proj, depth = bal.snavely_project(cams[cam_idx], pts[pt_idx])
    assert (depth < 0).all(), "a point behind one of its cameras"
    N = len(cam_idx)
    obs = proj + rng.normal(0, sigma_px, (N, 2))
    cams0 = cams.copy()
    cams0[:, 0:3] += rng.uniform(-perturb[0], perturb[0], (C, 3))
    cams0[:, 3:6] += rng.uniform(-perturb[1], perturb[1], (C, 3))
    pts0 = pts + rng.uniform(-perturb[2], perturb[2], (P, 3))
    order = rng.permutation(N)
    return bal.BalProblem(C, P, cam_idx[order].astype(np.int32), pt_idx[order].astype(np.int32), np.ascontiguousarray(obs[order]),
                          np.concatenate([cams0.ravel(), pts0.ravel()]))


def structural_edges_tracks():
    """Tracks of a 270-camera problem with the structural edges of the Schur assembly: camera pairs that share exactly 1, 2, 31,
    32 (kLongSegment) and 33 .. 38 points (long pairs of 32 + r, r = 0..6, the seven lane groups), points seen by exactly two
    cameras, one track seen by 260 cameras (> 256), a camera with one observation (269), runs of two and three residual blocks
    on one (camera, point) pair on neighbouring cameras, and P, N that are not multiples of 64."""
    C = 270
    shares = [1, 2, 31, 32, 33, 34, 35, 36, 37, 38]
    pairs = [(20 + 10 * i, 21 + 10 * i) for i in range(len(shares))]
    tracks = []
    for (a, b), m in zip(pairs, shares):
        tracks += [[a, b]] * m
    excluded = {a for a, _ in pairs}
    tracks.append([c for c in range(C) if c not in excluded])     # 260 cameras; the only observation of camera 269
    # background: cameras c, c+2, c+4 (never both cameras of a designed pair, which are neighbours)
    for c in range(0, 265):
        tracks += [[c, c + 2, c + 4]] * 3
    tracks += [[150, 150, 152, 154], [151, 151, 153, 155], [152, 152, 152, 154], [153, 153, 153, 155, 157]]
    tracks.append([7, 9])
    return C, tracks
