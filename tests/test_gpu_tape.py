"""The device interpreter of recorded functors (csrc/tape.hpp: tape_run) against the extended-precision reference with a running
error bound (tests/tape_reference.py; tests/test_tape_reference_cpu.py shows what that bound catches).

One block at a time, through sk_cost_function_evaluate (single_eval_tape_kernel<W>, the only path that returns the Jacobian
itself): residuals and every Jacobian block of the whole generated corpus within 2 x bound; the cost-only branch; partial
Jacobian requests, beyond 32 parameter blocks too; singular points pinned against the body over rotation.Jet; and the same tape
under renumberings of its registers into files on both sides of every switch of the interpreter's width W.

Through the solvers (dense_eval_tape_kernel<0|W>, bal_eval_jac_tape_kernel<kLoss, W>, bal_eval_cost_tape_kernel<kLoss>, which
return nothing but LM steps): every accepted step against the damped normal equations formed from the long-double evaluation
of the same tape (tests/step_check.py: TapeModel), each case asserting through stat() the W and the LDS bytes it names.

With TAPE_CHECK_LOG set, every single-block case and every solver case appends one JSON line there (profiles/tape_interpreter_error.txt
is made from them)."""
import json
import os

import numpy as np
import pytest

import skeres_amd as sk
from helpers import sk_loss
import step_check as sc
import tape_reference as tr
from test_gpu_step_check import _device_steps, _check_steps

pytestmark = pytest.mark.gpu

FACTOR = 2.0   # another operation order than the bound's (tape_reference.py); not tuned to what the device returns
SENTINEL = -7.0e77


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    if sk.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: libskeres_amd has no CPU fallback")


def _log(**line):
    path = os.environ.get("TAPE_CHECK_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def _split(x, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [np.asarray(x[off[q]:off[q + 1]], dtype=np.float64) for q in range(len(sizes))]


def _evaluate(cf, x, sizes, nres, want=None, jacobians=True):
    """cf.evaluate at x: (r [nres], J [nres, dim]); want: the parameter blocks whose Jacobian is asked for (None: all).  The
    columns of a block not asked for hold SENTINEL, as does everything the call must not touch."""
    want = set(range(len(sizes))) if want is None else set(want)
    parameters = sk.RichDoubleMatrix.fromArrays(*_split(x, sizes))
    residuals = sk.RichDoubleArray.fromArray(np.full(nres, SENTINEL))
    rows = [sk.RichDoubleArray.fromArray(np.full(nres * s + 1, SENTINEL)) for s in sizes]   # one double past the end as a guard
    jac = sk.RichDoubleMatrix([rows[q] if q in want else None for q in range(len(sizes))]) if jacobians else None
    assert cf.evaluate(parameters, residuals, jac)
    J = np.full((nres, int(sum(sizes))), SENTINEL)
    off = 0
    for q, s in enumerate(sizes):
        got = rows[q].toArray(nres * s + 1)
        assert got[-1] == SENTINEL, "block %d: written past its end" % q
        if q in want and jacobians:
            J[:, off:off + s] = got[:-1].reshape(nres, s)
        else:
            assert np.all(got == SENTINEL), "block %d was not asked for and was written" % q
        off += s
    return residuals.toArray(nres), J


def _columns(sizes, blocks):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([np.arange(off[q], off[q + 1]) for q in sorted(blocks)]).astype(np.int64) if blocks else np.zeros(0, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# one block at a time
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_whole_corpus_within_twice_the_bound_of_the_reference():
    """Residuals and every Jacobian block of every corpus case <= 2 x bound from the extended-precision value; the cost-only
    branch gives residuals within the same bound; a request for some of the blocks returns those blocks' bits and leaves the
    others alone.  The corpus' tapes have at most 36 registers: W = 3 (the other widths: the renumbered files below)."""
    rng = np.random.default_rng(11)
    failures, per_op, worst, ran = [], {}, 0.0, 0
    for c in tr.corpus():
        ref = c.reference()
        if not isinstance(ref, tr.Reference):
            continue
        assert tr.pick_width(int(c.tape[2]), 64)[0] == 3
        cf = c.device_functor().toAutoDiffCostFunction()
        r, J = _evaluate(cf, c.x, c.sizes, c.nres)
        w = tr.worst_ratio(ref, r, J)
        r_cost, _ = _evaluate(cf, c.x, c.sizes, c.nres, jacobians=False)
        w_cost = tr.ratio(r_cost, ref.r, ref.r_bound)
        want = [q for q in range(len(c.sizes)) if rng.random() < 0.5]
        r_part, J_part = _evaluate(cf, c.x, c.sizes, c.nres, want=want)
        cols = _columns(c.sizes, want)
        same = np.array_equal(r_part, r, equal_nan=True) and np.array_equal(J_part[:, cols], J[:, cols], equal_nan=True)
        _log(kind="single", case=c.name, W=3, registers=int(c.tape[2]), dim=c.dim, ratio=w, ratio_cost_only=w_cost, ops=sorted(ref.ops))
        for op in ref.ops:
            per_op[op] = max(per_op.get(op, 0.0), w)
        worst, ran = max(worst, w, w_cost), ran + 1
        if not (w <= FACTOR and w_cost <= FACTOR and same):
            failures.append((c.name, w, w_cost, same))
    print("device / bound over %d cases: worst %.3f; per opcode: %s" % (ran, worst, {tr.OPCODE_NAMES[k]: round(v, 3) for k, v in sorted(per_op.items())}))
    assert ran >= 190 and set(per_op) == set(range(20))
    assert not failures, failures


@pytest.mark.parametrize("name", ["blocks-33", "blocks-48", "blocks-63", "blocks-64"])
def test_partial_jacobian_requests_beyond_32_parameter_blocks(name):
    """Block 32 alone, every odd block, all but block 0, the last block alone: the request mask has a bit per parameter block,
    up to 64 of them.  Each request returns the bits of the full evaluation for its blocks and leaves the other arrays alone."""
    c = next(c for c in tr.directed_cases() if c.name == name)
    ref = c.reference()
    nb = len(c.sizes)
    cf = c.device_functor().toAutoDiffCostFunction()
    r, J = _evaluate(cf, c.x, c.sizes, c.nres)
    assert tr.worst_ratio(ref, r, J) <= FACTOR
    for want in ([32], list(range(1, nb, 2)), list(range(1, nb)), [nb - 1], [0, 31, 32, nb - 1], []):
        r_part, J_part = _evaluate(cf, c.x, c.sizes, c.nres, want=want)
        cols = _columns(c.sizes, want)
        assert np.array_equal(r_part, r)
        assert np.array_equal(J_part[:, cols], J[:, cols]), want
        assert tr.ratio(J_part[:, cols], ref.J[:, cols], ref.J_bound[:, cols]) <= FACTOR


def test_singular_points_are_those_of_the_body_over_jets():
    """sqrt at 0 with zero and non-zero derivative parts, abs at +0 / -0, LT / LE at equality, NaN and Inf — value and derivative
    — in the arm a SELECT does not take, a NaN condition, literals and captured doubles as outputs: the pattern of NaN, Inf and
    signed zeros that HostAutoDiffCostFunctor's evaluation over rotation.Jet gives, finite values to the library's 4 ulp."""
    for name, f, x, expected in tr.singular_cases():
        r_j, J_j = expected if expected is not None else tr.jet_twin(f, np.asarray(x))
        r, J = _evaluate(f.toAutoDiffCostFunction(), np.asarray(x, dtype=np.float64), list(f.N), f.kNumResiduals)
        r_cost, _ = _evaluate(f.toAutoDiffCostFunction(), np.asarray(x, dtype=np.float64), list(f.N), f.kNumResiduals, jacobians=False)
        for got, want in ((r, r_j), (J, J_j), (r_cost, r_j)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, got, want)
            fin = np.isfinite(want)
            assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (name, got, want)   # infinities, with their sign
            assert np.array_equal(np.signbit(got[fin]), np.signbit(want[fin])), (name, got, want)
            assert np.all(np.abs(got[fin] - want[fin]) <= 4 * 2.0 ** -52 * np.abs(want[fin])), (name, got, want)


SINGLE_REGISTER_FILES = (36, 37, 48, 49, 72, 73, 96, 97, 144)   # both sides of every switch of W at 64 threads; 145: refused


@pytest.mark.parametrize("name", ["dim-13", "dim-64", "residuals-16", "blocks-7-13-1-43", "signs-2", "random-5"])
def test_a_renumbered_register_file_gives_the_result_of_the_compact_one(name):
    """The same tape with its registers renumbered into a declared file of R registers, register R - 1 in use: R on both sides
    of every switch of the width (64 threads: W = 3 up to 36, 2 up to 48, 1 up to 72, then — one workgroup per CU — 2 up to 96 and
    1 up to 144 registers, 144 KiB of LDS).  Every Jacobian column is computed by the same expression whatever W is, so the
    result is asserted bitwise equal to the compact tape's (W = 3)."""
    c = next(c for c in tr.corpus() if c.name == name)
    ref = c.reference()
    r0, J0 = _evaluate(c.device_functor().toAutoDiffCostFunction(), c.x, c.sizes, c.nres)
    assert tr.worst_ratio(ref, r0, J0) <= FACTOR
    widths = set()
    for k, R in enumerate(SINGLE_REGISTER_FILES):
        W, lds = tr.pick_width(R, 64)
        widths.add(W)
        f = tr.FixedTapeFunctor(tr.renumber(c.tape, R, seed=k), c.nres, c.sizes, c.captured)
        r, J = _evaluate(f.toAutoDiffCostFunction(), c.x, c.sizes, c.nres)
        w = tr.worst_ratio(ref, r, J)
        _log(kind="single-renumbered", case=c.name, W=W, registers=R, lds_bytes=lds, dim=c.dim, ratio=w, bitwise=bool(np.array_equal(r, r0) and np.array_equal(J, J0)))
        assert w <= FACTOR, (R, W, w)
        assert np.array_equal(r, r0) and np.array_equal(J, J0), (R, W, float(np.max(np.abs(J - J0))))
        r_cost, _ = _evaluate(f.toAutoDiffCostFunction(), c.x, c.sizes, c.nres, jacobians=False)
        assert tr.ratio(r_cost, ref.r, ref.r_bound) <= FACTOR
    assert widths == {1, 2, 3}
    too_many = tr.FixedTapeFunctor(tr.renumber(c.tape, 145, seed=99), c.nres, c.sizes, c.captured)
    with pytest.raises(sk.SkeresError, match="more than the device interpreter holds"):
        _evaluate(too_many.toAutoDiffCostFunction(), c.x, c.sizes, c.nres)


# ---------------------------------------------------------------------------------------------------------------------------
# through the solvers: every accepted LM step against the long-double evaluation of the same tape (tests/step_check.py)
# ---------------------------------------------------------------------------------------------------------------------------
TAPE_STATS = ("tape_blocks", "tape_width", "tape_lds_bytes", "retained_points", "host_callback_blocks")   # (the last two: DENSE_SCHUR only)


class _LeastSquares(tr.BodyFunctor):
    """A corpus body minus a target: the targets are captured doubles after the body's own (targets = False: the body alone)."""

    def __init__(self, body, targets=True):
        super().__init__(body, captured=np.zeros(body.ncap + (body.k if targets else 0)))
        self.targets = targets

    def apply(self, *blocks):
        cap = self.captured_values()
        y = self.body.apply(cap[:self.body.ncap], *blocks)
        return [y[r] - cap[self.body.ncap + r] for r in range(self.body.k)] if self.targets else y


def _functor_and_tape(seed, sizes, nres, nsteps, ncap, registers, targets=True):
    """A least-squares functor of a random corpus body and its tape, renumbered into a file of `registers` (None: as recorded)."""
    rng = np.random.default_rng(seed)
    f = _LeastSquares(tr.Body(rng, sizes, nres, nsteps, ncap, touch_all="leaves"), targets)
    tape = f.tape()
    assert registers is None or int(tape[2]) <= registers, (int(tape[2]), registers)
    return f, (tape if registers is None else tr.renumber(tape, registers, seed=seed)), rng


TARGET_NOISE = 0.1   # the problems are no zero-residual ones: at a residual of 1e-6 the subtraction body - target alone loses the digits
KMAX = 2             # that check()'s 1e-11 on gradient_max_norm asks for, as does the gradient within a few steps of its zero


def _targets(f, tape, rng, X_true, ncap_body):
    """captured doubles per residual block: the body's own, then (if the functor takes targets) the body's value at X_true plus noise"""
    nb = X_true.shape[0]
    cap = np.concatenate([rng.normal(0, 1, (nb, ncap_body)), np.zeros((nb, f.body.k if f.targets else 0))], axis=1)
    if f.targets:
        r, _ = tr.run_np(tape, X_true, cap)
        cap[:, ncap_body:] = r + TARGET_NOISE * rng.normal(0, 1, r.shape)
    return cap


def _run_case(case, build, model, configure, kmax, expect, no_loss_cost=None):
    xs, logs, stats, sums = _device_steps(build, kmax, configure, names=TAPE_STATS)
    for k, v in expect.items():
        assert stats[k] == v, (k, stats)
    if no_loss_cost is not None:   # iteration 0 compares the evaluation directly: the cost here, gradient_max_norm in check(),
        cost = sum(float(np.sum(r * r)) for r, _ in model.chunks(xs[0])) / 2   # both to check()'s 1e-11 (observed: below 1e-13)
        assert abs(logs[1][0]["cost"] - cost) <= 1e-11 * cost, (logs[1][0]["cost"], cost)
    checked, _ = _check_steps(case, model, xs, logs, kmax)
    _log(kind="solver", case=case, W=stats["tape_width"], lds_bytes=stats["tape_lds_bytes"], tape_blocks=stats["tape_blocks"], steps_checked=checked,
         solver=int(sums[1].linearSolverTypeUsed()))
    return stats, sums


DENSE_CASES = {
    # name: (solver, residual blocks, parameter block sizes, residuals, registers, loss, held)   [128 lanes per workgroup]
    "one-block-dim5-W3": ("DENSE_QR", 1, (2, 2, 1), 3, None, None, False),
    "127-blocks-dim13-W2-57KiB": ("DENSE_NORMAL_CHOLESKY", 127, (5, 4, 3, 1), 1, 19, None, False),
    "129-blocks-dim64-16res-W1": ("DENSE_QR", 129, (16, 16, 16, 8, 4, 4), 16, 36, None, False),
    "300-blocks-dim13-W3-72KiB-cauchy": ("DENSE_QR", 300, (3, 3, 3, 4), 3, 18, ("cauchy", 1.5), False),
    "300-blocks-dim5-W2-144KiB-held": ("DENSE_NORMAL_CHOLESKY", 300, (2, 2, 1), 3, 48, None, True),
    "129-blocks-dim13-W1-144KiB": ("DENSE_QR", 129, (5, 4, 3, 1), 1, 72, None, False),
    "127-blocks-dim5-5blocks-W1-50KiB": ("DENSE_NORMAL_CHOLESKY", 127, (1, 1, 1, 1, 1), 3, 25, None, False),
}


@pytest.mark.parametrize("case", sorted(DENSE_CASES))
def test_dense_solver_steps_of_a_recorded_functor(case):
    """dense_eval_tape_kernel<W> (Jacobian) and <0> (candidate cost) under DENSE_QR / DENSE_NORMAL_CHOLESKY: residual blocks over
    3 - 6 parameter blocks at scattered offsets, shared between residual blocks; the register file renumbered so that the case
    runs the width and the LDS request its name says, asserted through stat()."""
    solver, count, sizes, nres, registers, loss, held = DENSE_CASES[case]
    seed = sorted(DENSE_CASES).index(case) + 100
    f, tape, rng = _functor_and_tape(seed, sizes, nres, 14, 1, registers)
    W, lds = tr.pick_width(int(tape[2]), 128)
    per_position = max(1, count // 16) if count > 1 else 1
    # the pool of parameter blocks: per_position blocks for each position of the functor, laid out in a random order
    blocks = [(q, j) for q in range(len(sizes)) for j in range(per_position)]
    order = rng.permutation(len(blocks))
    offset, n = {}, 0
    for i in order:
        offset[blocks[i]] = n
        n += sizes[blocks[i][0]]
    offs = np.array([[offset[(q, int(rng.integers(per_position)))] for q in range(len(sizes))] for _ in range(count)], dtype=np.int64)
    x_true = rng.normal(0, 1, n)
    X_true = np.concatenate([x_true[offs[:, q, None] + np.arange(s)] for q, s in enumerate(sizes)], axis=1)
    cap = _targets(f, tape, rng, X_true, 1)
    x0 = x_true + 0.05 * rng.normal(0, 1, n)
    held_cols, constant_at, subset_at = [], None, None
    if held:   # a constant block and a subset parameterization (of two different blocks in use)
        constant_at, subset_at = int(offs[0, 0]), int(offs[0, 1])
        held_cols = list(range(constant_at, constant_at + sizes[0])) + [subset_at + 1]

    def build():
        params = sk.RichDoubleArray.fromArray(x0)
        problem = sk.Problem()
        problem.addResidualBlocksTraced(tr.FixedTapeFunctor(tape, nres, sizes, captured=np.zeros(cap.shape[1])), cap, sk_loss(loss), params, offs)
        if held:
            problem.setParameterBlockConstant(params.slice(constant_at))
            problem.setParameterization(params.slice(subset_at), sk.PredefinedLocalParameterizations.subset(sizes[1], [1]))
        return problem, params, n

    model = sc.TapeModel(n, [(tape, sizes, cap, offs, loss)], held=held_cols)
    stats, sums = _run_case("dense-" + case, build, model, lambda o: o.setLinearSolverType(getattr(sk.LinearSolverType, solver)), KMAX,
                            {"tape_blocks": count, "tape_width": W, "tape_lds_bytes": lds}, no_loss_cost=None if loss else True)
    assert ("W%d" % W) in case and sums[1].linearSolverTypeUsed() == getattr(sk.LinearSolverType, solver)


def test_dense_solver_refuses_a_register_file_beyond_144_kib():
    f, tape, rng = _functor_and_tape(7, (2, 2), 2, 10, 0, 73)
    assert tr.pick_width(73, 128)[0] == 0 and tr.pick_width(72, 128)[0] == 1
    params = sk.RichDoubleArray.fromArray(rng.normal(0, 1, 4))
    problem = sk.Problem()
    problem.addResidualBlocksTraced(tr.FixedTapeFunctor(tape, 2, (2, 2), captured=np.zeros(2)), np.zeros((1, 2)), None, params, np.array([[0, 2]]))
    options = sk.Solver.Options()
    options.setLinearSolverType(sk.LinearSolverType.DENSE_QR)
    with pytest.raises(sk.SkeresError, match="more than the device interpreter holds"):
        solver = sk.StepSolver(options, problem)
        while not solver.step():
            pass


BAL_CASES = {
    # name: ((residuals; camera, point), registers, captured by the body, targets, loss, retained points, every n-th block on the host)
    "2-9-3-W3-no-captured": ((2, 9, 3), None, 0, False, None, 0, 0),
    "2-9-3-W3-8-captured-huber": ((2, 9, 3), 9, 6, True, ("huber", 0.5), 0, 0),
    "2-7-3-W2-72KiB-cauchy": ((2, 7, 3), 12, 1, True, ("cauchy", 1.0), 0, 0),
    "2-8-2-W1-72KiB-retained": ((2, 8, 2), 18, 2, True, None, 6, 0),
    "1-6-3-W2-144KiB-1-captured-host-every-4th": ((1, 6, 3), 24, 0, True, None, 0, 4),
    "2-1-1-W1-144KiB-huber": ((2, 1, 1), 36, 2, True, ("huber", 0.5), 0, 0),
    "2-9-3-W2-retained-host-every-4th": ((2, 9, 3), 10, 1, True, None, 6, 4),
}


def _bal_setup(case):
    (nres, cs, ps), registers, ncap, targets, loss, retained, host_every = BAL_CASES[case]
    seed = sorted(BAL_CASES).index(case) + 200
    f, tape, rng = _functor_and_tape(seed, (cs, ps), nres, 7, ncap, registers, targets)
    C, P, N = 16, 200, 900   # N is no multiple of the 256 lanes of a workgroup
    cam = rng.integers(0, C, N)
    pt = np.concatenate([np.arange(P), np.arange(P), rng.integers(0, P, N - 2 * P)])   # every point at least twice
    offs = np.stack([cs * cam, cs * C + ps * pt], axis=1).astype(np.int64)
    n = cs * C + ps * P
    x_true = rng.normal(0, 1, n)
    X_true = np.concatenate([x_true[offs[:, q, None] + np.arange(s)] for q, s in enumerate((cs, ps))], axis=1)
    cap = _targets(f, tape, rng, X_true, ncap)
    x0 = x_true + 0.03 * rng.normal(0, 1, n)
    return f, tape, cap, offs, n, x0, (nres, cs, ps), loss, retained, host_every, C


@pytest.mark.parametrize("case", sorted(BAL_CASES))
def test_dense_schur_steps_of_a_recorded_functor(case):
    """bal_eval_jac_tape_kernel<kLoss, W> and bal_eval_cost_tape_kernel<kLoss> under DENSE_SCHUR: the block shapes (2; 9, 3),
    (2; 7, 3), (2; 8, 2), (1; 6, 3), (2; 1, 1) — 12, 10, 10, 9 and 2 parameters, so each W meets a last pass it does not fill —,
    register files for W = 3, 2, 1 up to 144 KiB of LDS, 0 / 1 / 8 captured doubles, with and without a loss, with retained points
    forced on and with every fourth block through the director path."""
    f, tape, cap, offs, n, x0, (nres, cs, ps), loss, retained, host_every, C = _bal_setup(case)
    W, lds = tr.pick_width(int(tape[2]), 256)
    N = offs.shape[0]
    device = tr.FixedTapeFunctor(tape, nres, (cs, ps), captured=np.zeros(cap.shape[1]))

    def build():
        params = sk.RichDoubleArray.fromArray(x0)
        problem = sk.Problem()
        if not host_every:
            problem.addResidualBlocksTraced(device, cap, sk_loss(loss), params, offs)
        else:
            keep = []
            for i in range(N):
                cf = f.withCaptured(*cap[i]).toHostAutoDiffCostFunction() if i % host_every == 0 else device.withCaptured(*cap[i]).toAutoDiffCostFunction()
                keep.append(cf)
                problem.addResidualBlock(cf, sk_loss(loss) or sk.PredefinedLossFunctions.trivialLoss(), params.slice(int(offs[i, 0])), params.slice(int(offs[i, 1])))
            problem._keep_alive_for_the_test = keep
        return problem, params, n

    def configure(o):
        o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR)
        if retained:
            o.setRetainedPoints("on", retained)
        if not f.targets or nres == 1:   # the body alone is far from a minimum, and 900 residuals hardly determine 696 unknowns:
            o.setInitialTrustRegionRadius(0.1)   # a Gauss-Newton step overshoots and is rejected, a damped one is accepted

    kind = np.zeros(n, dtype=np.int8)
    kind[cs * C:] = 1
    model = sc.TapeModel(n, [(tape, (cs, ps), cap, offs, loss)], kind=kind)
    hosted = len(range(0, N, host_every)) if host_every else 0
    kept = 0
    if retained:   # (at most `retained`: the plan keeps the widest tracks the reduced system has room for)
        kept = build()[0].retainedPlan("on", retained)["retained_points"]
        assert 1 <= kept <= retained
    stats, sums = _run_case("schur-" + case, build, model, configure, KMAX,
                            {"tape_blocks": N - hosted, "host_callback_blocks": hosted, "tape_width": W, "tape_lds_bytes": lds, "retained_points": kept},
                            no_loss_cost=None if loss else True)
    assert ("W%d" % W) in case and sums[1].linearSolverTypeUsed() == sk.LinearSolverType.DENSE_SCHUR
    assert cap.shape[1] == {"2-9-3-W3-no-captured": 0, "1-6-3-W2-144KiB-1-captured-host-every-4th": 1, "2-9-3-W3-8-captured-huber": 8}.get(case, cap.shape[1])


@pytest.mark.parametrize("registers,captured", [(37, 2), (9, 9)])
def test_dense_schur_hands_a_tape_it_cannot_hold_to_the_alternate_solver(registers, captured):
    """37 registers (256 lanes: more than 144 KiB at W = 1) or 9 captured doubles: the DENSE_QR alternate takes the problem and says
    so; its steps are checked all the same."""
    rng = np.random.default_rng(5)
    nres, cs, ps = 2, 9, 3
    f, tape, rng = _functor_and_tape(300 + registers, (cs, ps), nres, 7, captured - nres, registers)
    C, P, N = 3, 8, 40
    offs = np.stack([cs * rng.integers(0, C, N), cs * C + ps * np.concatenate([np.arange(P), rng.integers(0, P, N - P)])], axis=1).astype(np.int64)
    n = cs * C + ps * P
    x_true = rng.normal(0, 1, n)
    cap = _targets(f, tape, rng, np.concatenate([x_true[offs[:, q, None] + np.arange(s)] for q, s in enumerate((cs, ps))], axis=1), captured - nres)
    x0 = x_true + 0.03 * rng.normal(0, 1, n)
    assert tr.pick_width(registers, 256)[0] == (0 if registers == 37 else 3) and cap.shape[1] == captured

    def build():
        params = sk.RichDoubleArray.fromArray(x0)
        problem = sk.Problem()
        problem.addResidualBlocksTraced(tr.FixedTapeFunctor(tape, nres, (cs, ps), captured=np.zeros(captured)), cap, None, params, offs)
        return problem, params, n
    W, lds = tr.pick_width(registers, 128)
    model = sc.TapeModel(n, [(tape, (cs, ps), cap, offs, None)])
    stats, sums = _run_case("alternate-%d-registers-%d-captured" % (registers, captured), build, model,
                            lambda o: o.setLinearSolverType(sk.LinearSolverType.DENSE_SCHUR), KMAX, {"tape_blocks": N, "tape_width": W, "tape_lds_bytes": lds},
                            no_loss_cost=True)
    assert sums[1].linearSolverTypeGiven() == int(sk.LinearSolverType.DENSE_SCHUR) and sums[1].linearSolverTypeUsed() == int(sk.LinearSolverType.DENSE_QR)


def _costs_of_two_iterations(build, solver_type, names):
    problem, params, n = build()
    options = sk.Solver.Options()
    options.setLinearSolverType(solver_type)
    options.setMaxNumIterations(2)
    solver = sk.StepSolver(options, problem)
    stats = {nm: solver.stat(nm) for nm in names}
    while not solver.step():
        pass
    summary = sk.Solver.Summary()
    solver.finish(summary)
    return stats, [(it["cost"], it["gradient_max_norm"], it["step_norm"]) for it in summary.iterations()], params.toArray(n), summary


def test_dense_kernel_on_both_sides_of_every_switch_of_the_width():
    """128 lanes: W = 3 up to 18 registers, 2 up to 24, 1 up to 36, then 2 up to 48 and 1 up to 72.  Every Jacobian column is the
    same expression whatever W is, so two LM iterations on the renumbered tape log the bits of the compact tape's."""
    sizes, nres, count = (3, 2, 2), 2, 40
    f, tape, rng = _functor_and_tape(41, sizes, nres, 12, 1, None)
    offs = np.array([[3 * int(rng.integers(4)), 12 + 2 * int(rng.integers(4)), 20 + 2 * int(rng.integers(4))] for _ in range(count)], dtype=np.int64)
    n = 28
    x_true = rng.normal(0, 1, n)
    cap = _targets(f, tape, rng, np.concatenate([x_true[offs[:, q, None] + np.arange(s)] for q, s in enumerate(sizes)], axis=1), 1)
    x0 = x_true + 0.03 * rng.normal(0, 1, n)

    def builder(t):
        def build():
            params = sk.RichDoubleArray.fromArray(x0)
            problem = sk.Problem()
            problem.addResidualBlocksTraced(tr.FixedTapeFunctor(t, nres, sizes, captured=np.zeros(cap.shape[1])), cap, None, params, offs)
            return problem, params, n
        return build
    names = ("tape_width", "tape_lds_bytes")
    _, log0, x_end0, _ = _costs_of_two_iterations(builder(tape), sk.LinearSolverType.DENSE_QR, names)
    assert len(log0) == 3 and log0[-1][0] < log0[0][0]
    widths = []
    for k, R in enumerate((18, 19, 24, 25, 36, 37, 48, 49, 72)):
        stats, log, x_end, _ = _costs_of_two_iterations(builder(tr.renumber(tape, R, seed=k)), sk.LinearSolverType.DENSE_QR, names)
        W, lds = tr.pick_width(R, 128)
        assert stats == {"tape_width": W, "tape_lds_bytes": lds}, (R, stats)
        assert log == log0 and np.array_equal(x_end, x_end0), (R, W)
        widths.append(W)
    assert widths == [3, 2, 2, 1, 1, 2, 2, 1, 1]


def test_dense_schur_kernels_on_both_sides_of_every_switch_of_the_width():
    """256 lanes: W = 3 up to 9 registers, 2 up to 12, 1 up to 18, then 2 up to 24 and 1 up to 36 — and 8 | 9 captured doubles: with 9
    the alternate solver takes the problem."""
    nres, cs, ps = 2, 9, 3
    f, tape, rng = _functor_and_tape(43, (cs, ps), nres, 7, 6, None)
    C, P, N = 4, 30, 150
    offs = np.stack([cs * rng.integers(0, C, N), cs * C + ps * np.concatenate([np.arange(P), np.arange(P), rng.integers(0, P, N - 2 * P)])], axis=1).astype(np.int64)
    n = cs * C + ps * P
    x_true = rng.normal(0, 1, n)
    cap = _targets(f, tape, rng, np.concatenate([x_true[offs[:, q, None] + np.arange(s)] for q, s in enumerate((cs, ps))], axis=1), 6)
    assert cap.shape[1] == 8
    x0 = x_true + 0.03 * rng.normal(0, 1, n)

    def builder(t):
        def build():
            params = sk.RichDoubleArray.fromArray(x0)
            problem = sk.Problem()
            problem.addResidualBlocksTraced(tr.FixedTapeFunctor(t, nres, (cs, ps), captured=np.zeros(8)), cap, None, params, offs)
            return problem, params, n
        return build
    names = ("tape_width", "tape_lds_bytes", "tape_blocks")
    _, log0, x_end0, s0 = _costs_of_two_iterations(builder(tape), sk.LinearSolverType.DENSE_SCHUR, names)
    assert len(log0) == 3 and log0[-1][0] < log0[0][0] and s0.linearSolverTypeUsed() == sk.LinearSolverType.DENSE_SCHUR
    widths = []
    for k, R in enumerate((9, 10, 12, 13, 18, 19, 24, 25, 36)):
        stats, log, x_end, s = _costs_of_two_iterations(builder(tr.renumber(tape, R, seed=k)), sk.LinearSolverType.DENSE_SCHUR, names)
        W, lds = tr.pick_width(R, 256)
        assert s.linearSolverTypeUsed() == sk.LinearSolverType.DENSE_SCHUR
        assert stats == {"tape_width": W, "tape_lds_bytes": lds, "tape_blocks": N}, (R, stats)
        assert log == log0 and np.array_equal(x_end, x_end0), (R, W)
        widths.append(W)
    assert widths == [3, 2, 2, 1, 1, 2, 2, 1, 1]
