"""Subprocess of tests/test_gpu_dogleg.py::test_mu_loop_after_factorisations_that_fail: the device run of one case of
tests/dogleg_cases.py (argv[1]) with the resident kernels on, pickled to argv[2].  A process of its own because a time-out of the
resident chain or of the resident back-substitution clears a process-wide switch, which must not leak into other tests."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dogleg_cases as dc  # noqa: E402
import test_gpu_dogleg as tg  # noqa: E402


def main():
    name, path = sys.argv[1], sys.argv[2]
    c, prob = dc.CASES[name], dc.problem(name)
    problem, params = tg._build(prob, loss=c.get("loss"), const_cams=c.get("const_cams", dc.CONST_CAMS))
    options = {k: v for k, v in c.get("options", {}).items() if k not in dc.REFERENCE_ONLY_OPTIONS}
    knobs = {"setMinLmDiagonal": options.pop("min_lm_diagonal")} if "min_lm_diagonal" in options else {}
    run = tg._solve(problem, params, prob.num_parameters, tg._options(c["kmax"], knobs=knobs, **options))
    with open(path, "wb") as f:
        pickle.dump(run, f)
    print("DOGLEG_WORKER_OK", name, flush=True)


if __name__ == "__main__":
    main()
