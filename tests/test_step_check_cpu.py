"""tests/step_check.py on the CPU: the backward error of a step is right (the independent fixture), the oracle's accepted steps
sit below its tolerance TAU (calibration), and a step of a deliberately wrong system lands at least 100 TAU above it (teeth)."""
import json
import os

import numpy as np
import pytest

import oracle
from skeres_amd import bal
import step_check as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _oracle(built):
    oracle.lib()


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63


def test_independent_fixture_step_is_at_the_rounding_floor():
    """tests/golden/lm_step.json (SymPy at 40 digits, refinement residual 5e-19, no code of the oracle or the product): its delta
    solves the damped normal equations the helper forms — sign, scale, D^2 and radius conventions pinned."""
    g = json.load(open(os.path.join(GOLDEN, "lm_step.json")))
    C, P, N = g["shape"]
    prob = bal.BalProblem(C, P, np.array(g["camera_index"], dtype=np.int32), np.array(g["point_index"], dtype=np.int32),
                          np.array(g["observations"]), np.array(g["x0"]))
    x0 = prob.parameters
    x1 = x0 + np.array(g["delta"])
    log = [{"trust_region_radius": g["initial_radius"], "gradient_max_norm": g["gradient_max_norm"]},
           {"cost_change": g["initial_cost"] - g["candidate_cost"], "relative_decrease": g["relative_decrease"], "step_is_successful": 1}]
    e = sc.backward_error(sc.BalModel(prob), x0, x0, x1, log, 1)
    assert e["eta"] <= sc.TAU / 100, e
    assert abs(e["mcc"] - g["model_cost_change"]) <= 1e-12 * g["model_cost_change"], e
    assert abs(e["gmax"] - g["gradient_max_norm"]) <= 1e-12 * g["gradient_max_norm"], e


def _oracle_steps(prob, kmax, loss=None, cam_mask=None, pt_mask=None, **opts):
    """x_0 .. x_kmax and the logs of oracle.solve_bal with max_num_iterations = k."""
    xs, logs = [prob.parameters.copy()], [None]
    for k in range(1, kmax + 1):
        o = oracle.default_options(linear_solver_type=oracle.DENSE_SCHUR, max_num_iterations=k, num_threads=4, **opts)
        x, so = oracle.solve_bal(prob.num_cameras, prob.num_points, prob.camera_index, prob.point_index, prob.observations,
                                 prob.parameters, o, loss=loss, cam_mask=cam_mask, pt_mask=pt_mask)
        xs.append(x)
        logs.append(sc.log_of(so))
    return xs, logs


CALIBRATION = [
    ("6-cameras", (6, 40, 200, 1), {}),
    ("16-cameras", (16, 600, 2600, 11), {}),
    ("49-cameras", (49, 7776, 31843, 49), {}),
    ("150-cameras", (150, 3000, 14000, 5), {}),
    ("tolerant-loss", (16, 600, 2600, 11), {"loss": ("tolerant", 4.0, 1.0)}),
    ("constant-blocks", (60, 2500, 12000, 13), {"masks": True}),
    ("rejected-step", (16, 600, 2600, 4), {"perturb": (0.1, 1.0, 2.0), "min_relative_decrease": 0.65}),
    ("clamped-diagonal", (150, 3000, 14000, 5), {"min_lm_diagonal": 0.5}),
]


@pytest.mark.parametrize("name,shape,extra", CALIBRATION, ids=[c[0] for c in CALIBRATION])
def test_oracle_steps_pass_at_tau(name, shape, extra):
    """Calibration: every accepted step of the oracle for k = 1..4 has eta <= max(TAU, 4 floor), the helper's model cost change
    and gradient norm agree with the oracle's log (observed eta: profiles/step_backward_error.txt)."""
    C, P, N, seed = shape
    extra = dict(extra)
    prob = bal.generate(C, P, N, seed=seed, **({"perturb": extra.pop("perturb")} if "perturb" in extra else {}))
    loss = extra.pop("loss", None)
    cam_mask = pt_mask = None
    if extra.pop("masks", False):
        cam_mask = np.full(C, 0b111000000, dtype=np.int32)   # intrinsics held by a subset parameterization
        cam_mask[[0, C // 2]] = 0x1ff                         # two constant cameras
        pt_mask = np.zeros(P, dtype=np.int32)
        pt_mask[[3, 40]] = 7                                  # two constant points
    xs, logs = _oracle_steps(prob, 4, loss=loss, cam_mask=cam_mask, pt_mask=pt_mask, **extra)
    model = sc.BalModel(prob, loss=loss, cam_mask=cam_mask, pt_mask=pt_mask)
    s = sc.jacobi_scale(model, prob.parameters)
    accepted = 0
    for k in range(1, 5):
        log = logs[k]
        if len(log) <= k:
            break
        assert k == 1 or [it["cost"] for it in log[:k]] == [it["cost"] for it in logs[k - 1][:k]]
        if not log[k]["step_is_successful"]:
            assert np.array_equal(xs[k], xs[k - 1])
            continue
        e = sc.check(model, prob.parameters, xs[k - 1], xs[k], log, k, scale=s, min_lm_diagonal=extra.get("min_lm_diagonal", 1e-6))
        assert e["eta"] <= sc.TAU, (k, e)
        # the default min_lm_diagonal (1e-6) clamps no column here (||J_s,j||^2 >= 0.24); 0.5 clamps some and not others
        assert (0 < e["clamped"] < e["free"]) if "min_lm_diagonal" in extra else e["clamped"] == 0, e
        accepted += 1
    assert accepted >= 3
    if name == "rejected-step":   # step 3 rejected, step 4 solves the same J with a new D
        assert [bool(logs[k][k]["step_is_successful"]) for k in range(1, 5)] == [True, True, False, True]


def test_oracle_steps_of_the_dense_paths_pass_at_tau():
    """The general dense path (oracle.evaluate per residual block): curve fitting, and BAL blocks through DENSE_QR with the
    intrinsics held by a subset parameterization."""
    from helpers import curve_fitting_data
    data = curve_fitting_data()
    blocks = [(oracle.EXPONENTIAL, [x, y], [0, 1]) for x, y in data]   # (EX/CurveFitting.scala: two 1-parameter blocks)
    xs = [np.zeros(2)]
    accepted = 0
    for k in range(1, 9):   # (its first steps from m = c = 0 are rejected)
        x, so = oracle.solve([1, 1], [0.0, 0.0], blocks, oracle.default_options(linear_solver_type=oracle.DENSE_QR, max_num_iterations=k))
        xs.append(x)
        log = sc.log_of(so)
        if log[k]["step_is_successful"]:
            e = sc.check(sc.BlocksModel([1, 1], [b + (None,) for b in blocks]), np.zeros(2), xs[k - 1], x, log, k)
            assert e["eta"] <= sc.TAU
            accepted += 1
    assert accepted >= 2
    prob = bal.generate(5, 30, 130, seed=2)
    C, P = prob.num_cameras, prob.num_points
    sizes = [9] * C + [3] * P
    rb = [(oracle.SNAVELY, list(prob.observations[o]), [int(prob.camera_index[o]), C + int(prob.point_index[o])]) for o in range(prob.num_observations)]
    params = [("subset", [6, 7, 8])] * C + [None] * P
    xs = [prob.parameters]
    for k in (1, 2, 3):
        x, so = oracle.solve_param(sizes, prob.parameters, rb, params, oracle.default_options(linear_solver_type=oracle.DENSE_QR, max_num_iterations=k))
        xs.append(x)
        log = sc.log_of(so)
        if log[k]["step_is_successful"]:
            e = sc.check(sc.BlocksModel(sizes, [b + (None,) for b in rb], params), prob.parameters, xs[k - 1], x, log, k)
            assert e["eta"] <= sc.TAU


# ---------------------------------------------------------------------------
# teeth: exact steps of wrong systems
# ---------------------------------------------------------------------------
class _Schur:
    """The damped normal equations of a small BAL problem at x, as dense doubles, with the Schur complement kept per point so
    that one term can be planted wrong."""

    def __init__(self, prob, s, x, radius, min_lm_diagonal=1e-6):
        C, P, N = prob.num_cameras, prob.num_points, prob.num_observations
        self.C, self.P = C, P
        r, F, E, _ = oracle.bal_evaluate(C, P, prob.camera_index, prob.point_index, prob.observations, x)
        n = 9 * C + 3 * P
        J = np.zeros((2 * N, n))
        for o in range(N):
            c, p = int(prob.camera_index[o]), int(prob.point_index[o])
            J[2 * o:2 * o + 2, 9 * c:9 * c + 9] += F[o]
            J[2 * o:2 * o + 2, 9 * C + 3 * p:9 * C + 3 * p + 3] += E[o]
        self.obs_rows = (F * s[9 * prob.camera_index[:, None] + np.arange(9)][:, None, :],
                         E * s[9 * C + 3 * prob.point_index[:, None] + np.arange(3)][:, None, :])
        Js = J * s
        self.D2 = np.clip((Js * Js).sum(0), min_lm_diagonal, 1e32) / radius
        self.A = Js.T @ Js + np.diag(self.D2)
        self.b = Js.T @ r.ravel()
        self.s = s
        nc = 9 * C
        self.U, self.W = self.A[:nc, :nc], self.A[:nc, nc:]
        self.Vinv = [np.linalg.inv(self.A[nc + 3 * p:nc + 3 * p + 3, nc + 3 * p:nc + 3 * p + 3]) for p in range(P)]

    def term(self, p):
        """W_p V_p^-1 W_p^T: point p's share of the Schur complement."""
        Wp = self.W[:, 3 * p:3 * p + 3]
        return Wp @ self.Vinv[p] @ Wp.T

    def reduced(self):
        nc = 9 * self.C
        S = self.U.copy()
        rhs = self.b[:nc].copy()
        for p in range(self.P):
            Wp = self.W[:, 3 * p:3 * p + 3]
            S -= self.term(p)
            rhs -= Wp @ (self.Vinv[p] @ self.b[nc + 3 * p:nc + 3 * p + 3])
        return S, rhs

    def solve(self, S=None, rhs=None, zero_yc_point=None):
        nc = 9 * self.C
        S0, rhs0 = self.reduced()
        S = S0 if S is None else S
        rhs = rhs0 if rhs is None else rhs
        yc = np.linalg.solve(S, rhs)
        y = np.empty(nc + 3 * self.P)
        y[:nc] = yc
        for p in range(self.P):
            Wp = self.W[:, 3 * p:3 * p + 3]
            yp = yc if p != zero_yc_point else np.zeros_like(yc)
            y[nc + 3 * p:nc + 3 * p + 3] = self.Vinv[p] @ (self.b[nc + 3 * p:nc + 3 * p + 3] - Wp.T @ yp)
        return y


def _blk(i):
    return slice(9 * i, 9 * i + 9)


def _shared(prob, i, j):
    a = set(prob.point_index[prob.camera_index == i].tolist())
    return sorted(a & set(prob.point_index[prob.camera_index == j].tolist()))


@pytest.fixture(scope="module")
def teeth_problem():
    """8 cameras, 150 points, one (camera, point) pair observed twice; the oracle's first two steps and logs."""
    prob = bal.generate(8, 150, 700, seed=3)
    o = 17
    dup = bal.BalProblem(8, 150, np.r_[prob.camera_index, prob.camera_index[o]].astype(np.int32),
                         np.r_[prob.point_index, prob.point_index[o]].astype(np.int32),
                         np.vstack([prob.observations, prob.observations[o] + [0.4, -0.3]]), prob.parameters.copy())
    xs, logs = _oracle_steps(dup, 2)
    assert logs[1][1]["step_is_successful"] and logs[2][2]["step_is_successful"]
    model = sc.BalModel(dup)
    s = np.asarray(sc.jacobi_scale(model, dup.parameters), dtype=np.float64)
    return dup, xs, logs, model, s, o


DEFECTS = ["none", "pair-missing-one-point", "long-pair-missing-a-lane-group", "stale-block", "duplicate-cross-term-missing",
           "retained-point-without-D2", "retained-point-D2-of-the-next-radius", "point-back-substituted-with-yc-0",
           "jacobi-scale-at-x_k-1", "S-in-float32"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_wrong_system_is_far_above_tau(teeth_problem, defect):
    """The exact step of a deliberately wrong system, one per failure mode of the device's Schur assembly and solve, lands at
    least 100 TAU above the tolerance ("none": the same construction without a defect stays below TAU)."""
    prob, xs, logs, model, s, odup = teeth_problem
    C = prob.num_cameras
    k = 2 if defect in ("stale-block", "jacobi-scale-at-x_k-1") else 1
    log = logs[k]
    radius = log[k - 1]["trust_region_radius"]
    sys_ = _Schur(prob, s, xs[k - 1], radius)
    S, rhs = sys_.reduced()
    s_step = s
    y = None
    kw = {}
    # the pair of cameras sharing the most points (a long segment: >= 32 + 1)
    pairs = [(len(_shared(prob, i, j)), i, j) for i in range(C) for j in range(i)]
    nsh, pi, pj = max(pairs)
    assert nsh >= 33
    if defect == "none":
        y = sys_.solve()
    elif defect == "pair-missing-one-point":
        small = min((p for p in pairs if p[0] >= 2))
        _, i, j = small
        p = _shared(prob, i, j)[0]
        T = sys_.term(p)
        S[_blk(i), _blk(j)] += T[_blk(i), _blk(j)]
        S[_blk(j), _blk(i)] += T[_blk(j), _blk(i)]
    elif defect == "long-pair-missing-a-lane-group":
        for p in _shared(prob, pi, pj)[3::7]:   # lane group 3 of 7
            T = sys_.term(p)
            S[_blk(pi), _blk(pj)] += T[_blk(pi), _blk(pj)]
            S[_blk(pj), _blk(pi)] += T[_blk(pj), _blk(pi)]
    elif defect == "stale-block":
        S_prev, _ = _Schur(prob, s, xs[k - 2], logs[k - 1][k - 2]["trust_region_radius"]).reduced()
        S[_blk(pi), _blk(pj)] += S_prev[_blk(pi), _blk(pj)]
        S[_blk(pj), _blk(pi)] += S_prev[_blk(pj), _blk(pi)]
    elif defect == "duplicate-cross-term-missing":
        c, p = int(prob.camera_index[odup]), int(prob.point_index[odup])
        o1, o2 = odup, prob.num_observations - 1
        Fs, Es = sys_.obs_rows
        W1, W2 = Fs[o1].T @ Es[o1], Fs[o2].T @ Es[o2]
        S[_blk(c), _blk(c)] += W1 @ sys_.Vinv[p] @ W2.T + W2 @ sys_.Vinv[p] @ W1.T
    elif defect in ("retained-point-without-D2", "retained-point-D2-of-the-next-radius"):
        q = int(np.argmax(np.bincount(prob.point_index, minlength=prob.num_points)))   # the widest track
        rows = slice(9 * C + 3 * q, 9 * C + 3 * q + 3)
        A = sys_.A.copy()
        factor = -1.0 if defect == "retained-point-without-D2" else radius / log[k]["trust_region_radius"] - 1.0
        assert factor != 0.0
        A[rows, rows] += factor * np.diag(sys_.D2[rows])
        y = np.linalg.solve(A, sys_.b)
    elif defect == "point-back-substituted-with-yc-0":
        y = sys_.solve(zero_yc_point=int(prob.point_index[0]))
    elif defect == "jacobi-scale-at-x_k-1":
        # D^2 = clamp(||J_s,j||^2) / radius makes the step independent of s wherever the clamp does not bind (the scale cancels),
        # so a wrong scale shows only in clamped columns: here every column is clamped (||J_s,j|| < 1 < sqrt(min_lm_diagonal))
        s_step = np.asarray(sc.jacobi_scale(model, xs[k - 1]), dtype=np.float64)
        y = _Schur(prob, s_step, xs[k - 1], radius, min_lm_diagonal=1.0).solve()
        kw["min_lm_diagonal"] = 1.0
    elif defect == "S-in-float32":
        S = S.astype(np.float32).astype(np.float64)
    if y is None:
        y = sys_.solve(S, rhs)
    x_next = xs[k - 1] + (-y) * s_step
    e = sc.backward_error(model, prob.parameters, xs[k - 1], x_next, log, k, **kw)
    print(defect, "eta %.3e floor %.3e" % (e["eta"], e["floor"]))
    if defect == "none":
        assert e["eta"] <= sc.TAU, e
    else:
        assert e["eta"] >= 100 * sc.TAU, e
