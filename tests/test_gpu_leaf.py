"""The device's leaves — rotation.hpp, loss.hpp, parameterization.hpp, functors.hpp as the kernels run them — against
tests/golden/leaf_reference.npz: values of tests/leaf_reference.py (mpmath / sympy, from the definitions, independent of the
oracle), read here as (hi, lo) pairs of doubles.  Needs neither mpmath nor sympy.  Bounds and their constants: leaf_reference.py;
the ratios measured on the oracle and on the device: profiles/leaf_error.txt."""
import numpy as np
import pytest

import skeres_amd as sk
import leaf_cases as lc
import leaf_reference as lr
from helpers import sk_loss

pytestmark = pytest.mark.gpu

FUNCTOR_CLASSES = {1: sk.SnavelyReprojectionError, 2: sk.ExponentialResidual, 3: sk.PowellF1, 4: sk.PowellF2, 5: sk.PowellF3,
                   6: sk.PowellF4, 7: sk.BinaryScalarCost, 8: sk.BinaryVector3Cost, 9: sk.TenParameterCost, 11: sk.HelloCostFunctor}


class DeviceBackend:
    def rotation(self, op, a, row_major, K):
        return sk.rotation.apply(op, a, row_major, K)

    def loss(self, spec, s):
        return sk_loss(spec).evaluate(s)

    def param(self, key, x, d, rows):
        P = sk.PredefinedLocalParameterizations
        if key[0] == "h":
            dev = P.homogeneousVector(x.shape[1])
        elif key[0] == "q":
            dev = P.quaternion()
        else:
            dev = P.subset(x.shape[1], [int(c) for c in key.split("_")[1]])
        assert (dev.globalSize(), dev.localSize()) == (x.shape[1], d.shape[1])
        return dev.plus(x, d), dev.computeJacobian(np.ascontiguousarray(x[rows]))

    def correct(self, spec, r, J):
        class Fixed(sk.SizedCostFunction):
            def __init__(self):
                super().__init__(len(r), J.shape[1])

            def evaluate(self, parameters, residuals, jacobians):
                for i in range(len(r)):
                    residuals[i] = r[i]
                if jacobians is not None and jacobians[0] is not None:
                    for i in range(len(r)):
                        for j in range(J.shape[1]):
                            jacobians[0][i, j] = J[i, j]
                return True

        x = sk.RichDoubleArray.fromArray(np.zeros(J.shape[1]))
        problem = sk.Problem()
        problem.addResidualBlock(Fixed(), sk_loss(spec), x)
        raw = sk.Problem.EvaluateOptions()
        raw.setApplyLossFunction(False)
        plain, out = problem.evaluate(raw, gradient=False), problem.evaluate(gradient=False)
        np.testing.assert_array_equal(plain["residuals"], r)  # what the corrector was given
        np.testing.assert_array_equal(plain["jacobian"].toDense(), J)
        return out["residuals"], out["jacobian"].toDense(), out["cost"]

    def functor(self, fid, c, p, want_jac):
        nres, sizes, _ = lc.FUNCTORS[fid]
        functor = sk.QuaternionRotationError(c[:3], c[3:]) if fid == 12 else FUNCTOR_CLASSES[fid](*c)
        cf = functor.toAutoDiffCostFunction()
        blocks = np.split(p, np.cumsum(sizes)[:-1])
        residuals = sk.DoubleArray(nres)
        jac = sk.RichDoubleMatrix([sk.DoubleArray(nres * n) for n in sizes]) if want_jac else None
        assert cf.evaluate(sk.RichDoubleMatrix.fromArrays(*blocks), residuals, jac)
        if not want_jac:
            return residuals.toArray(nres), None
        return residuals.toArray(nres), np.concatenate([jac.getRow(i).toArray(nres * n).reshape(nres, n) for i, n in enumerate(sizes)], axis=1)


@pytest.fixture(scope="module")
def ref():
    return lr.load()


@pytest.mark.parametrize("op", range(14), ids=lc.OP_NAMES)
def test_rotation_vs_reference(ref, op):
    tally = lr.run_rotation(DeviceBackend(), ref, lr.Tally(), op)
    assert tally.count == lr.expected_count(ref, "rot/%d/" % op)  # every value, both strides, doubles and Jets of 1, 3, 4


def test_zero_quaternion_has_no_rotation():
    with pytest.raises(sk.SkeresError, match="zero quaternion"):  # the one listed input without a reference value
        sk.rotation.apply(lc.Q2R, lc.ZERO_QUATERNION_RAISES, True)


def test_losses_vs_reference(ref):
    tally = lr.run_losses(DeviceBackend(), ref, lr.Tally())
    assert tally.count == lr.expected_count(ref, "loss/")


def test_local_parameterizations_vs_reference(ref):
    tally = lr.run_params(DeviceBackend(), ref, lr.Tally())
    assert tally.count == lr.expected_count(ref, "par/")


@pytest.mark.parametrize("fid", sorted(lc.FUNCTORS))
def test_functor_vs_reference(ref, fid):
    tally = lr.run_functor(DeviceBackend(), ref, lr.Tally(), fid)
    assert tally.count == lr.expected_count(ref, "fun/%d/" % fid)


# The Triggs corrector has no restated formula: leaf_reference.check_corrector holds the raw and the corrected (residuals,
# Jacobian) of one residual block, as Problem.evaluate returns them with and without the loss, to the two properties that define
# it, on the random r (k = 1, 2, 3) and J (k x 4) of leaf_cases.corrector_inputs(), answered by a host cost function.
def test_corrector_defining_properties():
    tally = lr.Tally()
    branches = lr.run_corrector(DeviceBackend(), tally)
    assert branches == {True, False} and tally.count == 3 * len(lc.corrector_inputs())
