"""Problem::Evaluate (include/skeres_amd.h: sk_problem_evaluate_*), what needs no device: the host plan's sizes and structure against
the numpy reference on every case, the argument errors, SK_ERR_NO_DEVICE, the reference checked against central differences of its
own cost, and the comparison function shown to reject planted defects (the tolerances hide nothing)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import skeres_amd as sk
from evaluate_cases import CASES, case
from evaluate_reference import LD, check, compare, reference, reference_of, tangent_size


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


@pytest.mark.parametrize("name", sorted(CASES))
def test_sizes_and_structure_equal_the_reference(name):
    c = case(name)
    ref = reference(c, structure_only=True)
    problem, options, params, keep = c.build()
    m = problem.evaluateStructure(options)
    assert (m.num_rows, m.num_cols, len(m.cols)) == (ref["num_rows"], ref["num_cols"], len(ref["cols"]))
    assert np.array_equal(m.rows, ref["rows"]) and np.array_equal(m.cols, ref["cols"])
    inside = np.ones(max(len(m.cols) - 1, 0), dtype=bool)   # strictly ascending columns inside every row
    ends = m.rows[1:-1]
    inside[ends[(ends > 0) & (ends < len(m.cols))] - 1] = False
    assert np.all(np.diff(m.cols)[inside] > 0) and np.all(np.diff(m.rows) >= 0)


def test_structure_conventions_on_the_manifolds_case():
    """tangent sizes 3 (quaternion), 3 (homogeneous vector of 4), 3 (subset {0}), 4 (constant: columns kept, nothing stored), 4"""
    c = case("manifolds")
    problem, options, params, keep = c.build()
    m = problem.evaluateStructure(options)
    assert m.num_cols == 3 + 3 + 3 + 4 + 4 and m.num_rows == 60
    stored = set(m.cols.tolist())
    assert stored == set(range(9)) | set(range(13, 17))   # the constant block's columns 9..12 hold no entry


def _raises_invalid(fn):
    with pytest.raises((ValueError, sk.SkeresError)) as e:
        fn()
    assert "status 1" in str(e.value) or isinstance(e.value, ValueError), e.value
    return str(e.value)


def test_argument_errors():
    c = case("powell")
    problem, _, params, keep = c.build()
    o = sk.Problem.EvaluateOptions()
    o.setResidualBlocks([0, 4])
    assert "no residual block" in _raises_invalid(lambda: problem.evaluateStructure(o))
    o.setResidualBlocks([-1])
    _raises_invalid(lambda: problem.evaluateStructure(o))
    o.setResidualBlocks([2, 1, 2])
    assert "twice" in _raises_invalid(lambda: problem.evaluateStructure(o))
    o.setResidualBlocks([])                 # n == 0: all again
    assert problem.evaluateStructure(o).num_rows == 4
    stranger = sk.RichDoubleArray.fromArray([0.0])
    o.setParameterBlocks([params.slice(0), stranger])
    assert "no parameter block" in _raises_invalid(lambda: problem.evaluateStructure(o))
    o.setParameterBlocks([params.slice(1), params.slice(1)])
    assert "twice" in _raises_invalid(lambda: problem.evaluateStructure(o))
    # the same through sk_problem_evaluate, whatever the device: argument errors come first
    _raises_invalid(lambda: problem.evaluate(o))
    o.setParameterBlocks([])
    assert problem.evaluateStructure(o).num_cols == 4


def test_dense_rows_are_unsupported():
    from skeres_amd import dense_synth  # noqa: F401  (the functor's home)
    x = sk.RichDoubleArray.ofSize(4)
    problem = sk.Problem()
    problem.addDenseRows(10, np.array([[1.0, 0.0, 0.5], [1.0, 1.0, -0.5]]), None, x, 4)
    with pytest.raises(sk.SkeresError) as e:
        problem.evaluateStructure()
    assert "status 4" in str(e.value) and "dense" in str(e.value)


def test_a_matrix_with_2_31_entries_is_refused():
    """One callback block of 1 << 16 residuals over a block of 1 << 15 parameters: 2^31 stored entries — sizes alone, nothing allocated."""
    big = 1 << 15

    class Wide(sk.SizedCostFunction):
        def __init__(self):
            super().__init__(1 << 16, big)

        def evaluate(self, parameters, residuals, jacobians):
            return False
    x = sk.RichDoubleArray.ofSize(big)
    problem, cost = sk.Problem(), Wide()
    problem.addResidualBlock(cost, None, x)
    with pytest.raises(sk.SkeresError) as e:
        problem.evaluateStructure()
    assert "status 4" in str(e.value) and "2^31" in str(e.value)


def test_without_a_device_evaluate_reports_no_device():
    if sk.device_count() > 0:
        pytest.skip("a device is present: the evaluation runs (tests/test_gpu_evaluate.py)")
    problem, options, params, keep = case("powell").build()
    cost = C.c_double()
    rc = sk.lib().sk_problem_evaluate(problem._h, None, C.byref(cost), None, None, None)
    assert rc == 2 and b"no HIP device" in sk.lib().sk_last_error()


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def _plus(c, x, b, j, h):
    """x with parameter block b moved by h along tangent coordinate j"""
    out = x.copy()
    a, e = c.off[b], c.off[b] + c.sizes[b]
    p = c.parameterizations.get(b)
    delta = np.zeros(tangent_size(c, b))
    delta[j] = h
    out[a:e] = oracle.parameterization_plus(p, x[a:e], delta) if p is not None else x[a:e] + delta
    return out


@pytest.mark.parametrize("name", ["powell", "curve_robust", "curve_robust_noloss", "mixed_sizes", "manifolds", "bal_small"])
def test_reference_gradient_against_central_differences_of_its_own_cost(name):
    """g_j = d cost / d delta_j of cost(Plus(x, delta)) — with a loss too: J~^T r~ = rho' J^T r.  Central differences of the
    reference's own cost (sums in long double, functors in double) with h = 1e-6: truncation ~ h^2, rounding ~ 2^-53 cost_scale / h
    ~ 1e-10 cost_scale, both far below 1e-6 x (grad_scale_j + cost_scale).  A wrong term moves g_j by a multiple of its
    ||J_b|| ||r_b||, the summands of grad_scale_j."""
    import copy
    c = case(name)
    ref = reference_of(name)
    columns = c.parameter_blocks if c.parameter_blocks is not None else c.first_seen()
    rng = np.random.default_rng(1)
    col, checked = 0, 0
    for b in columns:
        ts = tangent_size(c, b)
        if b in c.constant:
            assert np.all(ref["gradient"][col:col + ts] == 0)
        elif name != "bal_small" or rng.random() < 0.25:   # (a quarter of the 46 blocks of the bundle adjustment case)
            for j in range(ts):
                h = 1e-6
                costs = []
                for sign in (1, -1):
                    moved = copy.copy(c)
                    moved.x = _plus(c, c.x, b, j, sign * h)
                    costs.append(reference(moved)["cost"])
                fd = (costs[0] - costs[1]) / (2 * LD(h))
                tol = 1e-6 * (ref["grad_scale"][col + j] + ref["cost_scale"])
                assert abs(fd - ref["gradient"][col + j]) <= tol, (name, b, j, float(fd), float(ref["gradient"][col + j]), float(tol))
                checked += 1
        col += ts
    assert checked >= 2


# ---- the comparison rejects planted defects ---------------------------------------------------------------------------------------
def _copy_of(ref):
    return {k: np.array(ref[k], dtype=np.float64) for k in ("residuals", "gradient", "values")} | {"cost": float(ref["cost"]), "rows": ref["rows"], "cols": ref["cols"]}


@pytest.mark.parametrize("name", ["curve_robust", "manifolds", "bal_small"])
def test_the_reference_rounded_to_double_passes_its_own_comparison(name):
    ratios = check(reference_of(name), _copy_of(reference_of(name)), case(name))
    assert max(ratios.values()) < 0.1


def test_comparison_rejects_a_missing_loss_correction():
    c, ref = case("curve_robust"), reference_of("curve_robust")
    got = _copy_of(ref)
    got["values"] = np.array(reference(c, defect="no_loss")["values"], dtype=np.float64)
    assert compare(ref, got, c)["jacobian"] > 1e3


def test_comparison_rejects_an_unprojected_quaternion_block():
    c, ref = case("manifolds"), reference_of("manifolds")
    got = _copy_of(ref)
    got["values"] = np.array(reference(c, defect="no_projection")["values"], dtype=np.float64)
    assert compare(ref, got, c)["jacobian"] > 1e3


def test_comparison_rejects_two_swapped_columns_of_a_row():
    c, ref = case("bal_small"), reference_of("bal_small")
    got = _copy_of(ref)
    a = int(ref["rows"][11])
    got["values"][[a + 3, a + 4]] = got["values"][[a + 4, a + 3]]
    assert compare(ref, got, c)["jacobian"] > 1e3


def test_comparison_rejects_a_block_written_at_its_neighbours_offset():
    c, ref = case("mixed_sizes"), reference_of("mixed_sizes")
    got = _copy_of(ref)
    br, rows = ref["block_rows"], ref["rows"]
    a, b, e = int(rows[br[2]]), int(rows[br[3]]), int(rows[br[4]])   # block 2 (1 x 4) written where block 3 (3 x 4) begins
    block = got["values"][a:b].copy()
    got["values"][a:b] = 0.0
    got["values"][b:b + len(block)] = block
    assert e - b >= len(block) and compare(ref, got, c)["jacobian"] > 1e3


def test_comparison_rejects_a_gradient_column_missing_its_last_term():
    c, ref = case("wide_column"), reference_of("wide_column")
    got = _copy_of(ref)
    j = 4                                    # a column of camera 0: 400 rows touch it
    rows_with_j = [r for r in range(ref["num_rows"]) if j in ref["cols"][ref["rows"][r]:ref["rows"][r + 1]]]
    assert len(rows_with_j) == 400
    r = rows_with_j[-1]
    k = int(ref["rows"][r]) + list(ref["cols"][ref["rows"][r]:ref["rows"][r + 1]]).index(j)
    got["gradient"][j] -= float(ref["values"][k] * ref["residuals"][r])
    assert compare(ref, got, c)["gradient"] > 1e3
