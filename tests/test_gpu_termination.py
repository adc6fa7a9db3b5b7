"""Every exit of the trust-region loop on the device, bracketed at its threshold (tests/termination_check.py) on the cases of
tests/termination_cases.py: an "in" run that must end for that reason at that iteration, field by field, and an "out" run an ulp or
so away that must not.  The parameter bracket holds |x| as the solver sums it — a value no log shows — to (n + 8) 2^-53 on every
path that produces it: DENSE_SCHUR's fused reduction (replayed and launch by launch, with retained points, pseudo-camera and
padding slots, held coordinates), the dense solvers' sum over the ambient vector, dense rows, CGNR's norms, and the host arithmetic
of a world of ranks (tests/termination_worker.py).

With TERMINATION_LOG set, every bracket appends one line (case, exit, k, threshold, delta, the plan's stats, seconds) there:
profiles/termination_exits.txt is such a file."""
import os
import subprocess
import sys
import time

import pytest

import skeres_amd as sk
import termination_cases as tc
import termination_check as tk

pytestmark = pytest.mark.gpu

# (world, mode, shape, segments): shapes of the generator's family (C, 10 C, 43 C).  retainedPlan gives twelve retained points and
# segmentPlan two segments from 100 cameras on and three from 150 on (48 cameras: one); segmentPlan cuts the sequence WITHOUT retained
# points, though, and with their twelve pseudo-cameras the device cuts 150 cameras in two, whatever the world: 150 serves the worlds of
# two, and the world of three takes 300, the next size tried (600 and 900 are what the other world tests run)
WORLDS = {"sharded-2": (2, "sharded", "150,1500,6500,9,kept", None), "segmented-2": (2, "segmented", "150,1500,6500,9,kept2", 2),
          "segmented-3": (3, "segmented", "300,3000,13000,9,keptN", 3)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _record(case, entry, stats, seconds):
    path = os.environ.get("TERMINATION_LOG")
    line = "%s %s k=%s threshold=%s delta=%s plan=%s seconds=%.2f" % (
        case, entry["exit"], entry["k"], entry["threshold"] if isinstance(entry["threshold"], tuple) else "%.17g" % entry["threshold"],
        "%.3e" % entry["delta"] if "delta" in entry else "-", sorted(stats.items()), seconds)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def brackets():
    """The baseline of a case, once per module; every DENSE_SCHUR case ran the plan it names."""
    cache = {}

    def get(case):
        if case not in cache:
            c = tc.CASES[case]
            b = tk.Brackets(c["device"](), c["K"], c["n"], show=case)
            tc.check_plan(case, b.base["stats"])
            print(case, "baseline", [(e["cost"], e["gradient_max_norm"], e["step_norm"], e["trust_region_radius"], e["step_is_successful"]) for e in b.log], flush=True)
            cache[case] = b
        return cache[case]
    return get


def _bracket(brackets, case, exit):
    t = time.time()
    b = brackets(case)
    entry = b.order(tc.CASES[case].get("parameter_before_function", True)) if exit == "order" else getattr(b, exit)()
    _record(case, entry, b.base["stats"], time.time() - t)


@pytest.mark.parametrize("case", tc.names("gradient"))
def test_gradient_tolerance_exit(brackets, case):
    _bracket(brackets, case, "gradient")


@pytest.mark.parametrize("case", tc.names("radius"))
def test_minimum_trust_region_radius_exit(brackets, case):
    _bracket(brackets, case, "radius")


@pytest.mark.parametrize("case", tc.names("function"))
def test_function_tolerance_exit(brackets, case):
    _bracket(brackets, case, "function")


@pytest.mark.parametrize("case", tc.names("parameter"))
def test_parameter_tolerance_exit(brackets, case):
    _bracket(brackets, case, "parameter")


@pytest.mark.parametrize("case", tc.names("order"))
def test_order_of_the_tests_and_the_iteration_limit(brackets, case):
    _bracket(brackets, case, "order")


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_of_ranks_parameter_bracket(name):
    """The ranks share GPU 0 and exchange through gloo.  The existing world tests take 25 to 60 s on shapes four to six times this
    one with a single solve; the time limit is ten times that.  Nothing is retried."""
    world, mode, shape, segments = WORLDS[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29500 + world + (os.getpid() % 83)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "termination_worker.py"), mode, shape] + ([str(segments)] if segments else [])
    t = time.time()
    out = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TERMINATION_WORKER_OK world=%d" % world)]
    assert line, out.stdout[-3000:]
    print(line[-1], "wall %.1f s" % (time.time() - t), flush=True)
    path = os.environ.get("TERMINATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write("world-%s %s wall=%.1f\n" % (name, line[-1], time.time() - t))
