"""The termination brackets (tests/termination_check.py) on the runners that need no device: tests/failure_reference.py in double
and in long double, and the compiled oracle, on every case of tests/termination_cases.py a reference model exists for.  The
conditions of the cases (every running minimum, the same k per exit on all three runners), every bracket and order run, and the
planted defects: the reference's loop with one defect each, which the harness must reject."""
import ast
import os

import numpy as np
import pytest

import step_check as sc
import termination_cases as tc
import termination_check as tk

# ("schur-small-launches" and "schur-dissected" are "schur-small-replay" and "schur-retained" to a CPU runner: the knobs are the device's;
# the reference's loop does not depend on the dense solver named, the oracle's factorisation does)
REFERENCE_CASES = ["schur-small-replay", "schur-rejecting", "curve-DENSE_QR", "dense-bal-DENSE_QR", "dense-bal-tangent-DENSE_QR"]
ORACLE_CASES = ["schur-small-replay", "schur-rejecting", "schur-retained", "curve-DENSE_QR", "curve-DENSE_NORMAL_CHOLESKY"]
# what the cases were chosen for: k of (gradient, radius, function, parameter)
EXPECTED_K = {"schur-small-replay": (2, 0, 2, 2), "schur-rejecting": (2, 5, 5, 2), "curve-DENSE_QR": (8, 1, 5, 7), "curve-DENSE_NORMAL_CHOLESKY": (8, 1, 5, 7)}
_chosen = {}


def _runner(case, which):
    c = tc.CASES[case]
    if which == "oracle":
        return c["oracle"]()
    return c["reference"](long_double=which == "long-double")


def _all(case, which):
    c = tc.CASES[case]
    b = tk.Brackets(_runner(case, which), c["K"], c["n"])
    out = b.all()
    ks = tuple(e["k"] for e in out[:4])
    print(case, which, "k (gradient, radius, function, parameter) =", ks, "order at", out[4]["k"], "solves", b.solves,
          "thresholds", ["%.17g" % e["threshold"] for e in out[:4]], flush=True)
    for exit, k in zip(("gradient", "function", "parameter"), (ks[0], ks[2], ks[3])):
        assert k >= 2 and b.is_running_minimum(exit, k)
    _chosen.setdefault(case, {})[which] = ks
    if case in EXPECTED_K:
        assert ks == EXPECTED_K[case]
    return b


@pytest.mark.parametrize("which", ["double", "long-double"])
@pytest.mark.parametrize("case", REFERENCE_CASES)
def test_brackets_on_the_reference(built, case, which):
    sc._require_long_double()
    _all(case, which)


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_brackets_on_the_oracle(built, case):
    b = _all(case, "oracle")
    assert "xs" not in b.base   # (this runner has its x_k fetched by runs of k iterations: the harness's other path)


def test_every_runner_chooses_the_same_iterations(built):
    """(after the tests above, whose choices it compares; alone, it makes them)"""
    for case in REFERENCE_CASES:
        for which in ("double", "long-double") + (("oracle",) if case in ORACLE_CASES else ()):
            if which not in _chosen.get(case, {}):
                _all(case, which)
        assert len(set(_chosen[case].values())) == 1, (case, _chosen[case])


def test_the_radius_bracket_stands_behind_a_rejection(built):
    c = tc.CASES["schur-rejecting"]
    b = tk.Brackets(c["reference"](), c["K"], c["n"])
    k = b.choose("radius")
    assert k == 5 and not b.log[k]["step_is_successful"] and all(e["trust_region_radius"] == 1e4 for e in b.log[:k])
    assert [e["trust_region_radius"] for e in b.log[k:]] == [5000.0, 1250.0, 156.25]


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def _small(defect, held=False):
    """The brackets of the 6-camera problem on the reference with a defect planted (held: one constant camera, one constant point,
    the intrinsics held by a subset parameterization — the reference's model, like the device's, leaves those coordinates in |x|)."""
    shape, seed, perturb = tc.SMALL
    prob = tc._bal(shape, seed, perturb)
    cam_mask, pt_mask = tc._schur_masks(prob, (1,), (3,), True) if held else (None, None)
    model = sc.BalModel(prob, cam_mask=cam_mask, pt_mask=pt_mask)
    run = tc.reference_runner(model, prob.parameters, None, False, schur=(prob.num_cameras, prob.num_points), defect=defect(prob, model) if callable(defect) else defect)
    return tk.Brackets(run, 4, prob.num_parameters)


def _norm(sel):
    return lambda x: float(np.sqrt(np.sum(np.asarray(x, dtype=np.longdouble)[sel] ** 2)))


TOLERANCE_EXITS = ("parameter", "function", "order")
# name: (the defect, the brackets that must fail — every other one must pass: the defect is the only thing wrong —, the held variant)
DEFECTS = {
    "xnorm over the cameras only": (lambda prob, model: dict(xnorm=_norm(slice(0, 9 * prob.num_cameras))), ("parameter", "order"), False),
    "xnorm with the last camera counted twice": (
        lambda prob, model: dict(xnorm=_norm(np.r_[0:prob.num_parameters, 9 * (prob.num_cameras - 1):9 * prob.num_cameras])), ("parameter", "order"), False),
    "xnorm over the free coordinates only": (lambda prob, model: dict(xnorm=_norm(model.free)), ("parameter", "order"), True),
    "< in the gradient test": (dict(gradient_strict=True), ("gradient", "order"), False),
    "<= in the radius test": (dict(radius_not_strict=True), ("radius",), False),
    "the function test before the parameter test": (dict(function_first=True), ("order",), False),
    "the tolerance tests after acceptance": (dict(after_acceptance=True), TOLERANCE_EXITS, False),
    "the exit's log entry missing": (dict(no_exit_entry=True), TOLERANCE_EXITS, False),
    "the exit's entry marked successful": (dict(exit_entry_successful=True), TOLERANCE_EXITS, False),
}


@pytest.mark.parametrize("held", [False, True])
def test_the_reference_without_a_defect_passes(built, held):
    _small(None, held).all()


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect_is_rejected(built, name):
    defect, fails, held = DEFECTS[name]
    b = _small(defect, held)
    for exit in tk.EXITS + ("order",):
        if exit in fails:
            with pytest.raises(AssertionError) as e:
                getattr(b, exit)()
            print(name, "->", exit, "rejects it:", str(e.value)[:200], flush=True)
        else:
            getattr(b, exit)()


def test_one_retained_point_is_far_above_the_parameter_bracket():
    """The figures the bracket is there for: on the 6-camera problem the points are 1.8e-5 of |x|; one point among the 150 cameras'
    10 350 coordinates is held to delta = 1.15e-12."""
    shape, seed, perturb = tc.SMALL
    x = tc._bal(shape, seed, perturb).parameters
    with_points, cameras_only = float(tk.xnorm(x)), float(tk.xnorm(x[:54]))
    assert 1e-5 < 1 - cameras_only / with_points < 3e-5
    assert tk.delta(174) < 1e-8 * (1 - cameras_only / with_points)
    big = tc.CASES["schur-retained"]["problem"]().parameters
    one_point = 1 - float(tk.xnorm(big[:-3]) / tk.xnorm(big))
    print("one point of %d coordinates: %.3e of |x|; delta %.3e" % (len(big), one_point, tk.delta(len(big))), flush=True)
    assert tk.delta(len(big)) < 1e-3 * one_point


def test_the_message_comparison_allows_one_unit_in_the_last_digit_and_no_more():
    assert tk._e_within_one_unit("9.813849e-05", "9.813850e-05") and tk._e_within_one_unit("9.999999e-05", "1.000000e-04")
    assert not tk._e_within_one_unit("9.813849e-05", "9.813851e-05") and not tk._e_within_one_unit("9.813849e-05", "9.813849e-04")


def test_the_parameter_threshold_solves_its_equation():
    for xn, sn in ((1645.7, 5.0), (1506.887000279133, 0.14788362866240054), (0.0, 0.75), (1e3, 1e-9)):
        p = tk.parameter_threshold(xn, sn)
        assert abs(p * (np.longdouble(xn) + p) - np.longdouble(sn)) <= 4 * np.finfo(np.longdouble).eps * np.longdouble(sn)


def test_the_harness_imports_neither_the_native_library_nor_the_oracle():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "termination_check.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported.update(a.name.split(".")[0] for a in node.names)
        if isinstance(node, ast.ImportFrom):
            imported.add((node.module or "").split(".")[0])
    assert imported == {"re", "numpy"}, imported
