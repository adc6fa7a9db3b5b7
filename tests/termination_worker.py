"""Worker of tests/test_gpu_termination.py::test_world_*: the parameter bracket and the iteration-limit run of
tests/termination_check.py in a world of ranks that share GPU 0 and exchange through gloo (the host-staged all-reduce of
tests/dist_gpu_worker2.py, whose set-up this follows).  Only the baseline, x_{k-1}, the two runs of the parameter bracket and the
limit run: |x| of a world is host arithmetic over the ranks' shares (BalSolver::evaluate_with_jacobian), and the parameter bracket
is the one check that sees it.

    termination_worker.py MODE C,P,N,SEED,KEPT [SEGMENTS]      MODE: sharded | segmented; KEPT: kept | kept2 | keptN

Every rank runs the same harness on its own log.  After every run, before it is judged, the ranks compare termination, len(log), x
and the logged fields the thresholds are made of (all-reduce MIN and MAX): either all ranks go on with the same data or all stop at
the same place.  delta is four orders above any rank-to-rank rounding difference of one sum, so both thresholds of a bracket lie on
the same side for every rank."""
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dist_gpu_worker2 import HostStagedAllReduce  # noqa: E402

K = 4
CODES = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}


def _same_on_all_ranks(values, what):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).copy())
    lo, hi = t.clone(), t.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    assert torch.equal(lo, hi), "the ranks differ in " + what


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")  # torch initialises HIP before the library does
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import skeres_amd as sk
    from skeres_amd import bal
    from helpers import bal_problem_to_sk
    import termination_cases as tc
    import termination_check as tk

    mode, fields = sys.argv[1], sys.argv[2].split(",")
    segments = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    shape, kept = [int(v) for v in fields[:4]], fields[4]
    prob = bal.generate(shape[0], shape[1], shape[2], seed=shape[3])
    hook = HostStagedAllReduce()
    plan = {}

    def build():
        problem, params, loss = bal_problem_to_sk(prob)
        return problem, params, prob.num_parameters, loss

    def configure():
        o = sk.Solver.Options()
        o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
        o.setDistributed(rank, world, hook)
        o.setDistributionMode({"sharded": 1, "segmented": 3}[mode])
        o.setRetainedPoints("on", 12)
        if kept == "kept2":
            o.setMaxSegments(2)
        return o

    device = tc.device_runner(build, configure, stats=("retained_points", "dissected", "segments"), distribution=True, track_xs=False)

    def run(opts):
        r = device(opts)
        _same_on_all_ranks([CODES[r["termination"]], len(r["log"])], "termination or len(log)")
        _same_on_all_ranks(np.concatenate([r["x"], [e[f] for e in r["log"] for f in tk.PREFIX_FIELDS]]), "x or the log")
        plan.update(r["stats"])
        assert r["stats"]["distribution"] == mode and r["stats"]["retained_points"] == 12, r["stats"]
        if mode == "segmented":
            assert r["stats"]["dissected"] == 1 and r["stats"]["segments"] == segments, r["stats"]
        return r

    t0 = time.time()
    b = tk.Brackets(run, K, prob.num_parameters, show="rank %d" % rank if rank == 0 else None)
    par = b.parameter()
    lim = b.limit()
    dist.barrier()
    if rank == 0:
        print("TERMINATION_WORKER_OK world=%d mode=%s kept=%s parameter k=%d threshold=%.17g delta=%.3e limit k=%d solves=%d plan=%s seconds=%.1f" % (
            world, mode, kept, par["k"], par["threshold"], par["delta"], lim["k"], b.solves, sorted(plan.items()), time.time() - t0), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
