"""The extended-precision reference of recorded functors (tests/tape_reference.py) checked on the CPU: what makes the power of
tests/test_gpu_tape.py a checked fact.  Its float64 twins stay inside the reference's bound; the bound is tight (1e-15 .. 1e-13
relative); few generated cases are dropped for an undecided comparison; the pass loop over W derivative slots and a renumbered
register file give the plain twin's bits; the long-double model agrees with the mpmath one; and each of a list of wrong rules,
planted in the twin, exceeds 2 x bound on at least three cases of the corpus — with every opcode hit by a defect that is caught.

Every test prints its figures (pytest -s shows them)."""
import functools

import numpy as np
import pytest

from skeres_amd import tape as T
import tape_reference as tr

FACTOR = 2.0      # what tests/test_gpu_tape.py allows the device: another operation order (tape_reference.py)
MIN_CAUGHT = 3


@functools.lru_cache(maxsize=None)
def _corpus():
    return tuple(tr.corpus())


@functools.lru_cache(maxsize=None)
def _kept():
    return tuple(c for c in _corpus() if isinstance(c.reference(), tr.Reference))


def test_few_cases_are_dropped_for_an_undecided_comparison():
    cases = _corpus()
    random = [c for c in cases if not c.directed]
    dropped = [c.name for c in random if not isinstance(c.reference(), tr.Reference)]
    dropped_directed = [(c.name, repr(c.reference())) for c in cases if c.directed and not isinstance(c.reference(), tr.Reference)]
    print("cases: %d random, %d directed; dropped: %d random (%.1f %%), %d directed" %
          (len(random), len(cases) - len(random), len(dropped), 100.0 * len(dropped) / len(random), len(dropped_directed)))
    assert len(random) >= 150 and len(dropped) <= 0.05 * len(random), dropped
    assert not dropped_directed, dropped_directed
    ops = set()
    for c in _kept():
        ops |= c.reference().ops
    assert ops == set(range(20)), sorted(set(range(20)) - ops)   # every opcode is live in some kept case


def test_the_float64_twins_stay_inside_the_bound():
    """The tape in float64 (run_np, plain forward mode) and the generic body over rotation.Jet (no recorder, no tape) deviate
    from the extended-precision value by at most 1 x bound on every residual and every Jacobian entry."""
    tape_ratios, jet_ratios = [], []
    for c in _kept():
        ref = c.reference()
        r, J = tr.run_np(c.tape, c.x, c.captured)
        tape_ratios.append(tr.worst_ratio(ref, r[0], J[0]))
        if c.tape is c.functor.tape():
            jet_ratios.append(tr.worst_ratio(ref, *tr.jet_twin(c.functor, c.x)))
    print("twin / bound: tape in float64 worst %.3f median %.3f; body over Jets worst %.3f median %.3f (%d cases)" %
          (max(tape_ratios), np.median(tape_ratios), max(jet_ratios), np.median(jet_ratios), len(tape_ratios)))
    assert max(tape_ratios) <= 1.0 and max(jet_ratios) <= 1.0


def test_the_bound_is_tight_enough_to_matter():
    """Relative size of the bound on the non-zero outputs: a 99th percentile above 1e-10 would mean that the generator produces
    cancellation, not coverage."""
    rel = []
    for c in _kept():
        ref = c.reference()
        v = np.concatenate([np.abs(ref.r), np.abs(ref.J).ravel()]).astype(np.float64)
        b = np.concatenate([ref.r_bound, ref.J_bound.ravel()])
        rel.append(b[v > 0] / v[v > 0])
    rel = np.concatenate(rel)
    print("bound / |value| over %d non-zero outputs: median %.2g, 99 %% %.2g, max %.2g" % (rel.size, np.median(rel), np.percentile(rel, 99), rel.max()))
    assert np.percentile(rel, 99) <= 1e-10


def test_the_pass_loop_and_a_renumbered_register_file_give_the_plain_twins_bits():
    checked = 0
    for c in _kept():
        r0, J0 = tr.run_np(c.tape, c.x, c.captured)
        for W in (3, 2, 1):
            r, J = tr.run_np(c.tape, c.x, c.captured, W=W)
            assert np.array_equal(r, r0, equal_nan=True) and np.array_equal(J, J0, equal_nan=True), (c.name, W)
        R = int(c.tape[2]) + 1 + checked % 7
        r, J = tr.run_np(tr.renumber(c.tape, R, seed=checked), c.x, c.captured, W=3)
        assert np.array_equal(r, r0, equal_nan=True) and np.array_equal(J, J0, equal_nan=True), (c.name, "renumbered", R)
        checked += 1
    assert checked >= 150


def test_the_long_double_model_agrees_with_the_mpmath_reference():
    """tests/step_check.py's TapeModel evaluates tapes with run_np in long double (2^-64): on a sample of the corpus it lies
    within 1 % of the float64 bound of the mpmath value."""
    worst = 0.0
    sample = _kept()[::3]
    for c in sample:
        r, J = tr.run_np(c.tape, c.x, c.captured, dtype=np.longdouble, W=3)
        worst = max(worst, tr.worst_ratio(c.reference(), r[0], J[0]))
    print("long double model / float64 bound: worst %.2e over %d cases" % (worst, len(sample)))
    assert worst <= 0.01


def test_singular_points_of_the_twin_are_those_of_the_body_over_jets():
    for name, f, x, expected in tr.singular_cases():
        r_j, J_j = expected if expected is not None else tr.jet_twin(f, np.asarray(x))
        for W in (None, 3, 2, 1):
            r, J = tr.run_np(f.tape(), x, f.captured, W=W)
            assert np.array_equal(r[0], r_j, equal_nan=True) and np.array_equal(J[0], J_j, equal_nan=True), (name, W, r, r_j, J, J_j)
            assert np.array_equal(np.signbit(r[0]), np.signbit(r_j)), name


def _opcodes_of_tape_py():
    kinds = {"REGISTER", "PARAMETER", "CAPTURED", "CONSTANT"}
    return {n: getattr(T, n) for n in dir(T) if n.isupper() and not n.startswith("_") and isinstance(getattr(T, n), int) and n not in kinds}


@functools.lru_cache(maxsize=None)
def _caught(defect):
    """number of corpus cases on which the twin with `defect` planted exceeds FACTOR x bound, and the smallest such ratio"""
    W = 3 if defect in ("last pass writes past dim", "register stride W") else None
    count, smallest = 0, np.inf
    for c in _kept():
        ref = c.reference()
        if not ref.ops & set(tr.DEFECTS[defect]):
            continue
        r, J = tr.run_np(c.tape, c.x, c.captured, W=W, defects=(defect,))
        w = tr.worst_ratio(ref, r[0], J[0])
        if w > FACTOR:
            count, smallest = count + 1, min(smallest, w)
    return count, smallest


@pytest.mark.parametrize("defect", sorted(tr.DEFECTS))
def test_a_planted_defect_exceeds_the_bound(defect):
    count, smallest = _caught(defect)
    print("%-34s caught on %3d cases, smallest ratio over the bound %.3g" % (defect, count, smallest))
    assert count >= MIN_CAUGHT


def test_every_opcode_is_hit_by_a_defect_that_is_caught():
    ops = _opcodes_of_tape_py()
    assert sorted(ops.values()) == list(range(20)) and [ops[n] for n in tr.OPCODE_NAMES] == list(range(20))
    for name, code in ops.items():
        own = [d for d, codes in tr.DEFECTS.items() if codes == (code,)]
        assert own and any(_caught(d)[0] >= MIN_CAUGHT for d in own), name


def test_pick_width_switches_where_the_register_file_crosses_72_and_144_kib():
    """registers x (W + 1) x threads x 8 bytes against 72 KiB, then 144 KiB: the register counts on both sides of every switch,
    for the 64 threads of a single evaluation, the 128 of the dense kernel and the 256 of the Schur path's."""
    for threads, steps in ((64, [(36, 3), (37, 2), (48, 2), (49, 1), (72, 1), (73, 2), (96, 2), (97, 1), (144, 1), (145, 0)]),
                           (128, [(18, 3), (19, 2), (24, 2), (25, 1), (36, 1), (37, 2), (48, 2), (49, 1), (72, 1), (73, 0)]),
                           (256, [(9, 3), (10, 2), (12, 2), (13, 1), (18, 1), (19, 2), (24, 2), (25, 1), (36, 1), (37, 0)])):
        for R, W in steps:
            assert tr.pick_width(R, threads)[0] == W, (threads, R)
            assert tr.pick_width(R, threads)[1] <= 144 * 1024


def test_the_step_check_model_of_a_tape_is_the_reference_block_by_block():
    """tests/step_check.py: TapeModel — residual blocks over parameter blocks at scattered offsets of one x, a held column — gives,
    block by block, the mpmath reference's residuals and Jacobian (to 1 % of the float64 bound), the held column zeroed."""
    import step_check as sc
    rng = np.random.default_rng(3)
    sizes, nres, count = (3, 2, 4), 2, 9
    f = tr.BodyFunctor(tr.Body(rng, sizes, nres, 12, 2, touch_all=True), captured=(0.0, 0.0))
    tape = tr.renumber(f.tape(), int(f.tape()[2]) + 5, seed=1)
    n = 40
    starts = {3: [0, 11, 30], 2: [3, 20, 38], 4: [5, 14, 24]}
    offs = np.array([[starts[s][int(rng.integers(3))] for s in sizes] for _ in range(count)], dtype=np.int64)
    cap = rng.normal(0, 1, (count, 2))
    x = rng.normal(0, 1, n)
    held = [11, 21]
    model = sc.TapeModel(n, [(tape, sizes, cap, offs, None)], held=held, chunk=4)
    seen = 0
    for r, terms in model.chunks(x):
        for b in range(r.shape[0]):
            o = offs[seen]
            try:
                ref = tr.reference(tape, np.concatenate([x[o[q]:o[q] + s] for q, s in enumerate(sizes)]), cap[seen])
            except tr.Undecided:
                seen += 1
                continue
            assert tr.ratio(r[b], ref.r, ref.r_bound) <= 0.01
            c0 = 0
            for q, s in enumerate(sizes):
                J, first = terms[q]
                assert first[b] == o[q]
                keep = np.array([o[q] + j not in held for j in range(s)])
                assert np.all(J[b][:, ~keep] == 0)
                assert tr.ratio(J[b][:, keep], ref.J[:, c0:c0 + s][:, keep], ref.J_bound[:, c0:c0 + s][:, keep]) <= 0.01
                c0 += s
            seen += 1
    assert seen == count
