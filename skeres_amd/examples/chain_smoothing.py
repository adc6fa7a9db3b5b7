"""A long chain of small parameter blocks solved with CGNR (no counterpart among the reference's examples: its linear solvers are
native Ceres').  Block k is a pair of doubles; BinaryVector3Cost joins every block to its neighbour, and one shared block (a
calibration-like hub) to many others.  The Jacobian has twelve stored entries per residual block and is never densified: with
100 000 blocks the dense path's normal matrix alone would be 320 GB.

    python -m skeres_amd.examples.chain_smoothing [blocks] [residual blocks on the shared block]
"""
import sys

import numpy as np

import skeres_amd as sk

HUB = 7


def chain_problem(num_blocks=100000, hub_blocks=2000, seed=3, noise=0.01, perturb=0.02):
    """(x0 [2 * num_blocks], c [residual blocks, 1], offsets [residual blocks, 2] of the two parameter blocks in x).  The three
    residuals of BinaryVector3Cost between (x0, x1) and (y0, y1) vanish together only where x0 y0 = 0, x1 y1 = c and
    x0 x1 + y0 y1 = -10 c: the hidden truth has even blocks (0, V) and odd blocks (-10 V, w_k), so every (even, odd) pair is
    consistent with c = V w_k; c carries noise, and the start is the truth perturbed."""
    rng = np.random.default_rng(seed)
    V = 0.2
    truth = np.zeros((num_blocks, 2))
    truth[0::2, 1] = V
    truth[1::2, 0] = -10 * V
    truth[1::2, 1] = rng.uniform(0.5, 1.5, len(truth[1::2]))
    a = np.arange(num_blocks - 1)
    pairs = np.stack([a, a + 1], axis=1)
    stride = 2 * max(1, (num_blocks - 40) // (2 * max(hub_blocks, 1)))
    partners = 20 + stride * np.arange(hub_blocks)
    partners = partners[partners < num_blocks]
    pairs = np.concatenate([pairs, np.stack([np.full(len(partners), HUB), partners], axis=1)])
    c = truth[pairs[:, 0], 1] * truth[pairs[:, 1], 1] + rng.normal(0, noise, len(pairs))
    x0 = (truth + rng.uniform(-perturb, perturb, truth.shape)).ravel()
    return x0, c[:, None], 2 * pairs.astype(np.int64)


def build(x0, c, offsets):
    params = sk.RichDoubleArray.fromArray(x0)
    problem = sk.Problem()
    problem.addResidualBlocks(sk.BinaryVector3Cost.FUNCTOR_ID, c, None, params, offsets)
    return problem, params


def main(argv=()):
    num_blocks = int(argv[1]) if len(argv) > 1 else 100000
    hub_blocks = int(argv[2]) if len(argv) > 2 else 2000
    x0, c, offsets = chain_problem(num_blocks, hub_blocks)
    problem, params = build(x0, c, offsets)
    options = sk.Solver.Options()
    options.setLinearSolverType(sk.LinearSolverType.CGNR)
    options.setPreconditionerType(sk.PreconditionerType.JACOBI)
    options.setMinimizerProgressToStdout(True)
    summary = sk.Solver.Summary()
    sk.ceres.solve(options, problem, summary)
    print(summary.fullReport())
    return summary


if __name__ == "__main__":
    main(sys.argv)
