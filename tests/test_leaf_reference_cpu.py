"""tests/leaf_reference.py against its own definitions, the committed fixture against a fresh run of it, the CPU oracle against
the fixture under the same compare() the GPU test uses, and compare() against planted defects: each of them must miss its
bound by a factor of 100 or more.  No GPU."""
import numpy as np
import pytest

import oracle
import leaf_cases as lc
import leaf_reference as lr


class OracleBackend:
    def rotation(self, op, a, row_major, K):
        return oracle.rotation_apply(op, a, row_major, K)

    def loss(self, spec, s):
        return np.array([oracle.loss_evaluate(spec, v) for v in s])

    @staticmethod
    def spec(key):
        if key[0] == "h":
            return ("homogeneous",)
        if key[0] == "q":
            return ("quaternion",)
        return ("subset", [int(c) for c in key.split("_")[1]])

    def param(self, key, x, d, rows):
        p = self.spec(key)
        return (np.array([oracle.parameterization_plus(p, x[i], d[i]) for i in range(len(x))]),
                np.array([oracle.parameterization_jacobian(p, x[i]) for i in rows]).reshape(len(rows), x.shape[1], d.shape[1]))

    def correct(self, spec, r, J):
        rt, Jt, rho = oracle.loss_correct(spec, r, J)
        return rt, Jt, 0.5 * rho

    def functor(self, fid, c, p, want_jac):
        blocks = np.split(p, np.cumsum(lc.FUNCTORS[fid][1])[:-1])
        ok, r, j = oracle.evaluate(fid, c, blocks, want_jacobians=want_jac)
        assert ok
        return r, (np.concatenate(j, axis=1) if want_jac else None)


@pytest.fixture(scope="module")
def ref():
    return lr.load()


def test_oracle_meets_the_reference_on_every_case(ref):
    oracle.build()
    tally = lr.run_all(OracleBackend(), ref, lr.Tally())
    assert tally.count == lr.expected_count(ref)  # nothing skipped or filtered
    with pytest.raises(ValueError):  # the one input without a reference value
        oracle.rotation_apply(lc.Q2R, lc.ZERO_QUATERNION_RAISES, True)


def test_oracle_corrector_has_its_defining_properties():
    tally = lr.Tally()
    assert lr.run_corrector(OracleBackend(), tally) == {True, False}  # with and without the alpha branch
    assert tally.count == 3 * len(lc.corrector_inputs())


def test_fixture_is_reproducible_bit_for_bit(ref):
    pytest.importorskip("mpmath")
    pytest.importorskip("sympy")
    fresh = lr.generate()
    assert sorted(fresh) == sorted(ref)
    for k in fresh:
        assert fresh[k].dtype == ref[k].dtype == np.float64 and fresh[k].tobytes() == ref[k].tobytes(), k


# ---- the reference's own properties, at 1e-40 --------------------------------------------------------------------------------
TOL = 1e-40


def _close(a, b, scale=1):
    return all(abs(x - y) <= TOL * scale for x, y in zip(a, b))


def test_rotation_reference_properties():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = lr.DPS
    for a64 in lc.rotation_inputs()[lc.AA2Q]:
        a = lr.vec(a64)
        R = lr.exp_so3(a)
        RRt = [[lr.dot(R[i], R[j]) for j in range(3)] for i in range(3)]
        assert _close(lr.flat(RRt), [1, 0, 0, 0, 1, 0, 0, 0, 1])                                  # orthogonal
        assert abs(lr.dot(R[0], lr.cross(R[1], R[2])) - 1) <= TOL                                 # det = 1
        q = lr.quaternion_of_angle_axis(a)
        assert abs(lr.dot(q, q) - 1) <= TOL
        assert _close(lr.flat(lr.scaled_rotation(q)), lr.flat(R))                                 # q p q* is exp([a]x) p
        theta = lr.norm(a)
        back = lr.log_quaternion(q, q[0] < 0)
        if theta <= mp.pi:                                                                        # the principal logarithm
            assert _close(back, a)
        else:                                                                                     # the short way round
            assert _close(back, [x * (theta - 2 * mp.pi) / theta for x in a])
        assert lr.norm(back) <= mp.pi + TOL
    for R64 in lc.rotation_inputs()[lc.R2Q]:
        R = lr.unflat(lr.vec(R64))
        q = lr.quaternion_of_matrix(R, lr.matrix_sign_index(R))
        # the input is a rounded rotation matrix: q reproduces it as far as it is one (1e-15), exactly when it is exact
        exact = all(v in (0.0, 1.0, -1.0) for v in R64)
        assert _close(lr.flat(lr.scaled_rotation(q)), lr.flat(R), 1 if exact else 1e25)
        aa = lr.log_quaternion(q, q[0] < 0)
        assert _close(lr.flat(lr.exp_so3(aa)), [v / lr.dot(q, q) for v in lr.flat(lr.scaled_rotation(q))])  # exp(log) = id
    # Euler angles: (pitch, roll, yaw) turn about x, y, z
    assert _close(lr.matvec(lr.euler_matrix(lr.vec([90, 0, 0])), lr.vec([0, 1, 0])), [0, 0, 1])
    assert _close(lr.matvec(lr.euler_matrix(lr.vec([0, 90, 0])), lr.vec([0, 0, 1])), [1, 0, 0])
    assert _close(lr.matvec(lr.euler_matrix(lr.vec([0, 0, 90])), lr.vec([1, 0, 0])), [0, 1, 0])
    # Hamilton: i j = k, and the product of rotations is the rotation of the product
    assert lr.qmul([0, 1, 0, 0], [0, 0, 1, 0]) == [0, 0, 0, 1]


def test_loss_reference_properties():
    mp = pytest.importorskip("mpmath")
    pytest.importorskip("sympy")
    mp.mp.dps = lr.DPS
    at0 = {("huber", 1.3): 1, ("softlone", 0.7): 1, ("cauchy", 0.5): 1, ("tukey", 2.0): mp.mpf(1) / 2,
           ("tolerant", 1.5, 0.4): 1 / (1 + mp.exp(mp.mpf(1.5) / mp.mpf(0.4))), ("scaled", None, 0.25): mp.mpf(0.25),
           ("scaled", ("cauchy", 0.8), 2.5): mp.mpf(2.5)}
    for spec in lc.LOSS_SPECS:
        r0 = lr.loss_reference(spec, [0.0])[0]
        assert abs(r0[0]) <= TOL, spec                                       # rho(0) = 0
        if spec in at0:
            assert abs(r0[1] - at0[spec]) <= TOL * max(1, abs(at0[spec])), spec  # rho'(0) as defined
    # the derivatives are the derivatives: central differences of rho and rho' at 60 digits
    h = mp.mpf("1e-20")
    for spec in lc.LOSS_SPECS:
        for s in (0.05, 1.0, 60.0):
            m, c, p = lr.loss_reference(spec, [mp.mpf(s) - h, s, mp.mpf(s) + h])
            assert abs((p[0] - m[0]) / (2 * h) - c[1]) <= 1e-30 * max(1, abs(c[1])), (spec, s)
            assert abs((p[1] - m[1]) / (2 * h) - c[2]) <= 1e-30 * max(1, abs(c[2])), (spec, s)


def test_manifold_reference_properties():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = lr.DPS
    groups = lr.param_groups()
    for key in ["h%d" % n for n in lc.HOMOGENEOUS_SIZES] + ["q"]:
        plus, xs, ds, rows = groups[key]
        for i in list(rows)[:20] + list(range(0, len(xs), 11)):
            x, d = lr.vec(xs[i]), lr.vec(ds[i])
            xn = lr.norm(x)
            assert _close(plus(x, [mp.mpf(0)] * len(d)), x, xn)                        # Plus(x, 0) = x
            p = plus(x, d)
            assert abs(lr.norm(p) - xn) <= TOL * xn                                    # |Plus(x, delta)| = |x|
            J = lr.plus_jacobian(plus, x, len(d))
            assert all(abs(sum(x[r] * J[r][c] for r in range(len(x)))) <= 1e-24 * xn * xn for c in range(len(d)))  # x^T J = 0 (h^2)
            for c in ("1e-9", "1e9"):                                                  # Plus(c x, delta) = c Plus(x, delta)
                c = mp.mpf(c)
                assert _close(plus([c * v for v in x], d), [c * v for v in p], c * xn)


# ---- planted defects: compare() must reject each by at least 100 x its bound --------------------------------------------------
def _rejected(family, got, hi, lo, unit):
    worst = float(lr.ratios(got, hi, lo, unit).max())
    with pytest.raises(AssertionError):
        lr.compare(family, got, hi, lo, unit)
    return worst / lr.C[family]


def _loss_unit(i, ref):
    return lr.U * lr.loss_scale(lc.loss_s(lc.LOSS_SPECS[i]), ref["loss/%d/hi" % i])


def _old_householder_plus(x, d):
    """Plus with the absolute threshold sigma <= ulp(1) and x's head left in v, in doubles (the branch that was wrong)."""
    n = len(x)
    nd = np.sqrt(d @ d)
    y = np.concatenate([np.sin(0.5 * nd) / nd * d if nd > 0 else 0.5 * d, [np.cos(0.5 * nd)]])
    v = np.concatenate([x[:-1], [1.0]])
    beta = 2.0 if x[-1] < 0 else 0.0
    return np.sqrt(x @ x) * (y - beta * v * (v @ y))


def planted_defects(ref):
    """name -> by how many times its bound compare() rejects it."""
    import mpmath as mp
    mp.mp.dps = lr.DPS
    out = {}
    f2 = lambda a: np.array([[float(v) for v in row] for row in a])
    specs = lc.LOSS_SPECS
    # 1. rho'' with its sign flipped
    i = specs.index(("cauchy", 0.5))
    got = ref["loss/%d/hi" % i].copy()
    got[:, 2] = -got[:, 2]
    out["rho'' sign flipped (cauchy)"] = _rejected("loss", got, ref["loss/%d/hi" % i], ref["loss/%d/lo" % i], _loss_unit(i, ref))
    # 2. tukey rho'' without the 1 / a^2
    i = specs.index(("tukey", 2.0))
    got = ref["loss/%d/hi" % i].copy()
    got[:, 2] *= 4.0
    out["tukey rho'' without 1/a^2"] = _rejected("loss", got, ref["loss/%d/hi" % i], ref["loss/%d/lo" % i], _loss_unit(i, ref))
    # 3. the composed chain rule without f' g''
    i = specs.index(("composed", ("huber", 1.1), ("softlone", 0.9)))
    s = lc.loss_s(specs[i])
    rg = lr.loss_reference(specs[i][2], s)
    got = ref["loss/%d/hi" % i].copy()
    for k in range(len(s)):
        rf = lr.loss_reference(specs[i][1], [rg[k, 0]])[0]
        got[k, 2] = float(rf[2] * rg[k, 1] ** 2)
    out["composed without f' g''"] = _rejected("loss", got, ref["loss/%d/hi" % i], ref["loss/%d/lo" % i], _loss_unit(i, ref))
    # 10. rho by the cancelling forms
    for spec, form in ((("softlone", 0.7), lambda s, a: 2 * a * a * (np.sqrt(1 + s / (a * a)) - 1)),
                       (("cauchy", 0.5), lambda s, a: a * a * np.log(1 + s / (a * a))),
                       (("tukey", 2.0), lambda s, a: np.where(s <= a * a, a * a / 6 * (1 - (1 - s / (a * a)) ** 3), a * a / 6)),
                       (("tolerant", 40.0, 1.0), lambda s, a: np.where(s - a > 36.7, s - a - np.log(1 + np.exp(-a)),
                                                                       np.log(1 + np.exp(np.minimum(s - a, 700.0))) - np.log(1 + np.exp(-a))))):
        i = specs.index(spec)
        got = ref["loss/%d/hi" % i].copy()
        with np.errstate(over="ignore"):
            got[:, 0] = form(lc.loss_s(spec), spec[1])
        fam = "loss_tolerant" if spec[0] == "tolerant" else "loss"
        out["rho by the cancelling form (%s)" % spec[0]] = _rejected(fam, got, ref["loss/%d/hi" % i], ref["loss/%d/lo" % i], _loss_unit(i, ref))
    # 4. a transposed matrix (stride mix-up)
    hi, lo = ref["rot/%d/v/hi" % lc.AA2R], ref["rot/%d/v/lo" % lc.AA2R]
    out["transposed rotation matrix"] = _rejected("rotation_value", lc.to_layout(hi, False), hi, lo, lr.U * lr.block_scale(hi, 1))
    # 5. quaternionToAngleAxis without the wrap for w < 0
    q = lc.rotation_inputs()[lc.Q2AA]
    n = np.sqrt(np.sum(q[:, 1:] ** 2, axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        got = np.where(n > 0, 2 * np.arctan2(n, q[:, :1]) / n, 2.0) * q[:, 1:]
    hi, lo = ref["rot/%d/v/hi" % lc.Q2AA], ref["rot/%d/v/lo" % lc.Q2AA]
    out["quaternionToAngleAxis without the wrap"] = _rejected("rotation_value", got, hi, lo, lr.U * lr.block_scale(hi, 1))
    # 6. the atan2 derivative with x and y swapped: d(angle) changes sign, so the Jet parts of aa = angle * axis come out as
    #    d(axis) angle - axis d(angle) where they are d(axis) angle + axis d(angle)
    K = 3
    hi, lo = ref["rot/%d/j4/hi" % lc.Q2AA][:, :, :K], ref["rot/%d/j4/lo" % lc.Q2AA][:, :, :K]
    seeds = lc.rotation_seeds(lc.Q2AA, K)
    got = hi.copy()
    for r in range(len(q)):
        x = lr.vec(q[r])
        if lr.norm(x[1:]) == 0:
            continue
        neg = x[0] < 0
        angle = lambda y: [lr.norm(lr.log_quaternion(y, neg))]
        axis = lambda y: [v / lr.norm(y[1:]) * (-1 if neg else 1) for v in y[1:]]
        for k in range(K):
            v = lr.vec(seeds[r, :, k])
            dang = lr.directional(angle, x, v)[0]
            got[r, :, k] -= [float(2 * dang * a) for a in axis(x)]
    out["atan2 derivative with x, y swapped"] = _rejected("rotation_jet", got, hi, lo, lr.U * lr.block_scale(hi, (1, 2)))
    # 7. quaternion Plus as x (x) exp(delta)
    xs, ds = lc.quaternion_inputs()
    wrong = lambda x, d: lr.qmul(x, lr.quaternion_plus([mp.mpf(1), 0, 0, 0], d))
    got = f2([wrong(lr.vec(xs[k]), lr.vec(ds[k])) for k in range(len(xs))])
    hi, lo = ref["par/q/plus/hi"], ref["par/q/plus/lo"]
    unit = lr.U * np.sqrt(np.sum(xs * xs, axis=1, keepdims=True))
    out["quaternion Plus as x (x) exp(delta)"] = _rejected("param", got, hi, lo, unit)
    # 8. two rows of the quaternion Jacobian swapped
    hi, lo = ref["par/q/jac/hi"], ref["par/q/jac/lo"]
    rows = lr.param_groups()["q"][3]
    out["quaternion Jacobian rows swapped"] = _rejected("param", hi[:, [0, 2, 1, 3], :], hi, lo, unit[rows][:, :, None])
    # 9. the old absolute Householder threshold
    xs, ds = lc.homogeneous_inputs(4)
    hi, lo = ref["par/h4/plus/hi"], ref["par/h4/plus/lo"]
    got = hi.copy()
    old = np.sum(xs[:, :-1] ** 2, axis=1) <= lc.ULP1
    for k in np.nonzero(old)[0]:
        got[k] = _old_householder_plus(xs[k], ds[k])
    unit = lr.U * np.sqrt(np.sum(xs * xs, axis=1, keepdims=True))
    out["absolute Householder threshold"] = _rejected("param", got, hi, lo, unit)
    return out


def test_compare_rejects_the_planted_defects(ref):
    pytest.importorskip("mpmath")
    pytest.importorskip("sympy")
    defects = planted_defects(ref)
    assert len(defects) == 13
    for name, times in defects.items():
        assert times >= 100.0, (name, times)
