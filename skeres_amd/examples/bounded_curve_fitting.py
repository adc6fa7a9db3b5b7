"""examples/.../CurveFitting.scala:100-133 with a box on c (ceres::Problem::SetParameterLowerBound / SetParameterUpperBound):
y = exp(m x + c) through the 67 samples, c kept inside [0.3, 2].  The unconstrained fit has c = 0.13, so the solve ends with c on
its lower bound and m taking up what it can."""
import os
import sys

import numpy as np

import skeres_amd as sk

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "curve_fitting_data.txt")


def main(argv=()):
    sk.ceres.initGoogleLogging("BoundedCurveFitting")
    data = np.loadtxt(_DATA)
    m = sk.DoubleArray(1)
    m.set(0, 1.0)
    c = sk.DoubleArray(1)
    c.set(0, 0.0)     # outside the box: the solve starts from its projection, c = 0.3
    loss = sk.PredefinedLossFunctions.trivialLoss()
    problem = sk.Problem()
    for x, y in data:
        problem.addResidualBlock(sk.ExponentialResidual(x, y).toAutoDiffCostFunction(), loss, m, c)
    problem.setParameterLowerBound(c, 0, 0.3)
    problem.setParameterUpperBound(c, 0, 2.0)
    options = sk.Solver.Options()
    options.setMaxNumIterations(25)
    options.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
    options.setMinimizerProgressToStdout(True)
    print("Initial: 1.0, 0.0   bounds on c: [%g, %g]" % (problem.getParameterLowerBound(c, 0), problem.getParameterUpperBound(c, 0)))
    summary = sk.Solver.Summary()
    sk.ceres.solve(options, problem, summary)
    final_x = [float(m.get(0)), float(c.get(0))]
    print(summary.briefReport())
    print("Final: %s" % ", ".join(repr(v) for v in final_x))
    return final_x


if __name__ == "__main__":
    main(sys.argv)
