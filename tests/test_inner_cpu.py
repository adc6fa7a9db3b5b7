"""Inner iterations without a device: the host plan (sk_inner_iteration_plan) against the recursion of tests/inner_reference.py on
every case, option validation and the refusals (decided from host data, before a device is touched), the planted defects of the
reference, the stand-alone plan check under the host sanitizers, and the rule the cases of tests/inner_cases.py were chosen by:

  * double and long double take the same outer pattern, the same CG iteration counts, the same rounds and, for every block, the
    same inner iteration count and final status;
  * every decision — each block's gradient max-norm, relative step, relative cost change and rho at every inner iteration, and
    the outer loop's — keeps inner_cases.DECISION_MARGIN from its threshold, in both precisions, at EVERY iteration (so also at
    the one that decides and the one before); the margin is a thousand times the largest difference of a decision of its kind
    between the two precisions over all cases (inner_cases.decisions, which says why per kind; profiles/inner_iterations_error.txt);
  * no block is left out."""
import os
import subprocess

import numpy as np
import pytest

import skeres_amd as sk
import cgnr_cases as cc
import inner_cases as k
import inner_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFECTS = {"no_boost": "bal-small", "no_useful": "bal-useful", "group1_unrefined": "bal-small", "outer_tolerances": "bal-small"}


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _device_groups(name, options=None):
    problem, params, n, keep = k.build_device(name)
    o = options or k.device_options(name)
    k.set_caller_ordering(name, o, params)
    plan = sk.Solver.innerIterationPlan(problem, o)
    order = k.problem_order(name)
    return [[b for b in range(len(order)) if plan["group_of_block"][order[b]] == g] for g in range(plan["num_groups"])], plan


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_plan_against_the_reference(name):
    got, plan = _device_groups(name)
    want = [list(g) for g in k.groups(name)]
    assert got == want and plan["num_groups"] == len(want)
    m, blocks = k.model(name), k.column_blocks(name)
    for g in want:                                        # the reference's own check of what it was handed
        assert ir.independent(m, k.x0(name), blocks, g) is None
    moving = {b for b, (start, size) in enumerate(blocks) if np.any(m.free[start:start + size])}
    listed = {b for g in want for b in g}
    assert listed <= moving and (listed == moving or k.caller_groups(name) is not None)
    assert int(np.sum(plan["group_of_block"] >= 0)) == len(listed)


def test_automatic_plan_without_options():
    problem, params, n, keep = k.build_device("bal-small")
    plan = sk.Solver.innerIterationPlan(problem)
    C = 6
    order = k.problem_order("bal-small")
    assert plan["num_groups"] == 2
    assert [int(plan["group_of_block"][order[b]]) for b in range(C)] == [-1, -1, 1, 1, 1, 1]        # cameras 0 and 1 are constant
    assert all(int(plan["group_of_block"][order[b]]) == 0 for b in range(C, C + 40))               # the points first


def test_the_shapes_reach_their_paths():
    """chain: a third group and a long hub, at the fewest blocks the builder allows; bal-robust: cameras of three and of four parts;
    quaternion: blocks of two parts; bal-small: single parts."""
    groups = k.groups("chain")
    hub = cc.CHAIN_HUB
    assert len(groups) >= 3 and hub in groups[-1] + groups[-2] and hub not in groups[0] + groups[1]
    m = k.model("chain")
    slots = sum(1 for blk in m.blocks for b in blk[2] if b == hub)
    assert slots == 64 + 1 == k.CHAIN_HUB_BLOCKS + 2      # one more than a part holds: with a hub block less it is a single part
    partners = [b for blk in m.blocks if hub in blk[2] for b in blk[2] if b != hub]
    assert max(partners) == k.CHAIN_BLOCKS - 1            # the last block is the hub's last partner: with a block less it does not exist
    prob = k.csc.bal_problem("bal-robust")
    counts = np.bincount(prob.camera_index)
    assert int(np.sum((counts > 128) & (counts <= 192))) >= 1 and int(np.max(counts)) > 192      # cameras of three parts, and of four
    assert 64 < k.cc.quaternion_setup()[1].shape[0] <= 128
    small = k.csc.bal_problem("bal-small")
    assert int(np.max(np.bincount(small.camera_index))) <= 64
    assert len(k.groups("all-eliminated")) == 1 and len(k.groups("all-eliminated")[0]) == 3
    assert len(k.groups("bal-points")) == 1 and len(k.groups("bal-points")[0]) == 40


def test_option_validation():
    o = sk.Solver.Options()
    assert o.useInnerIterations() is False and o.innerIterationTolerance() == 1e-3
    o.setUseInnerIterations(True)
    o.setInnerIterationTolerance(0.0)
    assert o.useInnerIterations() is True and o.innerIterationTolerance() == 0.0
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="inner_iteration_tolerance"):
            o.setInnerIterationTolerance(bad)
    assert o.innerIterationTolerance() == 0.0
    problem, params, n, keep = k.build_device("bal-small")
    with pytest.raises(ValueError, match="negative group"):
        o.setInnerIterationOrdering([(params.slice(9 * 6), -1)])
    o.setInnerIterationOrdering(None)       # automatic again
    assert sk.Solver.innerIterationPlan(problem, o)["num_groups"] == 2


def test_other_solver_types_refuse_the_option():
    """SK_ERR_UNSUPPORTED (4) with the solver's name, from the options alone: this machine needs no device for it."""
    problem, params, n, keep = k.build_device("bal-small")
    for t, nm in ((sk.LinearSolverType.DENSE_SCHUR, "DENSE_SCHUR"), (sk.LinearSolverType.DENSE_QR, "DENSE_QR"),
                  (sk.LinearSolverType.DENSE_NORMAL_CHOLESKY, "DENSE_NORMAL_CHOLESKY")):
        o = sk.Solver.Options()
        o.setLinearSolverType(t)
        o.setUseInnerIterations(True)
        with pytest.raises(sk.SkeresError, match="status 4: use_inner_iterations.*" + nm):
            sk.StepSolver(o, problem)


def test_refused_orderings():
    """Two cameras and a point they share in one group; a pointer that is no block of the problem: SK_ERR_INVALID_ARGUMENT (1) when
    the solver is created, and from sk_inner_iteration_plan."""
    problem, params, n, keep = k.build_device("bal-small")
    prob = k.csc.bal_problem("bal-small")
    C = prob.num_cameras
    cams = {}
    for c, p in zip(prob.camera_index, prob.point_index):
        if c >= 2:
            cams.setdefault(int(p), set()).add(int(c))
    point, seen_by = next((p, sorted(v)) for p, v in sorted(cams.items()) if len(v) >= 2)
    o = k.device_options("bal-small")
    o.setInnerIterationOrdering({0: [params.slice(9 * seen_by[0]), params.slice(9 * seen_by[1]), params.slice(9 * C + 3 * point)]})
    order = k.problem_order("bal-small")
    with pytest.raises(sk.SkeresError, match="status 1: .*not an independent set") as err:
        sk.StepSolver(o, problem)
    named = {order[seen_by[0]], order[seen_by[1]], order[C + point]}
    import re
    got = [int(v) for v in re.findall(r"parameter blocks (\d+) and (\d+)", str(err.value))[0]]
    assert len(set(got)) == 2 and set(got) <= named
    with pytest.raises(ValueError, match="not an independent set"):
        sk.Solver.innerIterationPlan(problem, o)
    other = sk.RichDoubleArray.fromArray(np.zeros(3))
    o = k.device_options("bal-small")
    o.setInnerIterationOrdering({0: [params.slice(9 * C), other.slice(0)]})
    with pytest.raises(sk.SkeresError, match="status 1: .*entry 1 is not a parameter block"):
        sk.StepSolver(o, problem)
    # a constant block is ignored, a valid ordering passes the host checks (and then needs a device)
    o = k.device_options("bal-small")
    o.setInnerIterationOrdering({5: [params.slice(0), params.slice(9 * C)]})
    plan = sk.Solver.innerIterationPlan(problem, o)
    assert plan["num_groups"] == 1 and int(np.sum(plan["group_of_block"] == 0)) == 1


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_defects_are_rejected(defect):
    """The comparison that holds the device to the reference (cgnr_cases.compare_logs and the rounds) rejects each planted defect."""
    name = DEFECTS[defect]
    good, bad = k.reference(name)[1], k.reference(name, defect=defect)[1]
    kmax = k.CASES[name]["kmax"]
    try:
        cc.compare_logs(bad, good, kmax)
        same = all(a["inner_iteration_rounds"] == b["inner_iteration_rounds"] and a["inner_blocks"] == b["inner_blocks"] for a, b in zip(bad, good))
    except AssertionError:
        same = False
    assert not same


def test_useful_accepts_what_rho_would_reject():
    log = k.reference("bal-useful")[1]
    e = log[2]
    assert e["useful"] and e["step_is_successful"] and 0 < e["relative_decrease"] <= 1e-3 * (1 - k.DECISION_MARGIN["outer rho"])
    assert not k.reference("bal-useful", defect="no_useful")[1][2]["step_is_successful"]


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_case_rule(name):
    a, b = k.reference(name)[1], k.reference(name, True)[1]
    kmax = k.CASES[name]["kmax"]
    assert len(a) == len(b) == kmax + 1
    for ea, eb in zip(a, b):
        for f in ("step_is_valid", "step_is_successful", "linear_solver_iterations", "inner_iteration_rounds", "useful"):
            assert ea[f] == eb[f], f
        assert ea["inner_blocks"] == eb["inner_blocks"]           # every block: iterations and status
    assert a[1]["inner_blocks"] is not None and a[1]["step_is_successful"] and set(a[1]["inner_blocks"]) == {q for g in k.groups(name) for q in g}
    cc.compare_logs(a, b, kmax, factor=0.1)                       # the two precisions agree ten times inside the device tolerances
    for kind, (deviation, closest, where, count) in sorted(k.decisions(name).items()):
        print("%s %s: %d decisions, difference %.3e (recorded %.3e), closest %.3e at %s, margin %.3e"
              % (name, kind, count, deviation, k.MEASURED_DECISION_DEVIATION[kind], closest, where, k.DECISION_MARGIN[kind]), flush=True)
        assert deviation <= k.MEASURED_DECISION_DEVIATION[kind], kind
        assert closest > k.DECISION_MARGIN[kind], (kind, where, closest)


def test_tolerance_case_switches_off():
    log = k.reference("bal-tolerance")[1]
    assert log[1]["inner_iteration_rounds"] > 0 and all(e["inner_iteration_rounds"] == 0 and e["inner_blocks"] is None for e in log[2:])


def test_plan_check_under_the_host_sanitizers(tmp_path):
    """tools/inner_plan_check.cpp is a stand-alone program over the host-only sources: address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "inner_plan_check")
    srcs = [os.path.join(ROOT, "tools", "inner_plan_check.cpp")] + [os.path.join(ROOT, "skeres_amd", "csrc", f)
                                                                    for f in ("inner_plan.cpp", "cgnr_plan.cpp", "jacobian_plan.cpp", "evaluate_plan.cpp")]
    out = subprocess.run(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")] + srcs + ["-o", exe],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "inner_plan_check ok" in run.stdout and "ordering ok" in run.stdout
