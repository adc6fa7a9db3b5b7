"""Worker of tests/test_gpu_inner.py: solves the named cases of tests/inner_cases.py with inner iterations in this process (whose
SK_INNER_BATCH the parent has set) and writes x after every LM iteration and the rounds per iteration to an .npz file."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import skeres_amd as sk
import inner_cases as k


def main():
    out = {}
    for name in sys.argv[2:]:
        problem, params, n, keep = k.build_device(name)
        solver = sk.StepSolver(k.device_options(name), problem)
        summary = sk.Solver.Summary()
        xs = [params.toArray(n)]
        while not solver.step():
            solver.finish(summary)
            xs.append(params.toArray(n))
        solver.finish(summary)
        out[name + "/xs"] = np.array(xs)
        out[name + "/rounds"] = np.array([int(e["inner_iteration_rounds"]) for e in summary.iterations()])
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
