"""Subprocess of tests/test_gpu_cgnr_schur.py::test_same_bytes_for_every_batch_size: solves the cases named in argv[2:] with CGNR and
the Schur elimination and stores x after every LM iteration and the solver's counters in argv[1] (.npz).  The parent runs it with
SK_CGNR_BATCH = 1, 3 and unset and compares bits: the environment is read once per process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skeres_amd as sk  # noqa: E402
import cgnr_schur_cases as k  # noqa: E402


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
        assert solver.stat("schur_elimination") == 1
        out[name + "/xs"] = np.array(xs)
        out[name + "/cg"] = np.array([it["linear_solver_iterations"] for it in summary.iterations()])
        out[name + "/batches"] = np.array([solver.stat("cg_batches"), solver.stat("linear_solves"), solver.stat("cg_iterations")])
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
