"""The block envelope's arithmetic (chol_envelope.hpp: BlockEnvelope::active_rows / height, cholesky_row_first_cols, cholesky_plan_flops)
against a brute-force count over an explicit boolean block mask, on random envelopes — the one definition of "the active block rows of
a block column" that the factorisation's plans, the flop counts and the planner's chain model all read."""
import ctypes as C

import numpy as np

import skeres_amd as sk

_ip = C.POINTER(C.c_int)


def _probe(nblk, last, tail, ncols, tail_rows):
    fn = sk.lib().sk_envelope_probe
    fn.restype = None
    fn.argtypes = [C.c_int, _ip, _ip, C.c_int, C.c_int, _ip, _ip, _ip, C.POINTER(C.c_double)]
    active = np.zeros((nblk, nblk + 1), dtype=np.int32)
    height = np.zeros(nblk, dtype=np.int32)
    first = np.zeros(nblk, dtype=np.int32)
    flops = C.c_double(0.0)
    ptr = lambda a: a.ctypes.data_as(_ip) if a is not None else None
    fn(nblk, ptr(last), ptr(tail), ncols, tail_rows, ptr(active), ptr(height), ptr(first), C.byref(flops))
    return active, height, first, flops.value


def _mask(nblk, last, tail, tail_rows):
    """mask[r, c]: block (r, c) of the lower triangle is inside the envelope — in column c's contiguous run from the diagonal down to
    last[c] (every row without an envelope), or one of its tail rows: from tail[c] on, or the uniform last tail_rows rows."""
    m = np.zeros((nblk, nblk), dtype=bool)
    for c in range(nblk):
        run_end = nblk - 1 if last is None else min(int(last[c]), nblk - 1)
        tail_begin = nblk - tail_rows if tail is None else int(tail[c])
        for r in range(c, nblk):
            m[r, c] = r <= run_end or r >= tail_begin
    return m


def _random_envelope(rng):
    nblk = int(rng.integers(2, 40))
    partial = rng.random() < 0.5
    ncols = int(rng.integers(1, nblk)) if partial else nblk
    tail_rows = int(rng.integers(1, nblk - ncols + 1)) if partial else 1
    last = None
    if rng.random() < 0.85:  # non-decreasing, last[c] >= c
        last = np.maximum.accumulate(np.minimum(np.arange(nblk) + rng.integers(0, 8, nblk), nblk - 1)).astype(np.int32)
    tail = None
    if rng.random() < 0.5:   # non-increasing, tail[c] <= nblk - 1
        tail = np.sort(rng.integers(max(1, nblk // 2), nblk, nblk))[::-1].astype(np.int32).copy()
    return nblk, last, tail, ncols, tail_rows


def test_block_envelope_against_an_explicit_block_mask():
    rng = np.random.default_rng(20250)
    for _ in range(300):
        nblk, last, tail, ncols, tail_rows = _random_envelope(rng)
        active, height, first, flops = _probe(nblk, last, tail, ncols, tail_rows)
        m = _mask(nblk, last, tail, tail_rows)
        for c in range(nblk):
            for r in range(c, nblk + 1):
                assert active[c, r] == int(m[r:, c].sum()), (nblk, last, tail, ncols, tail_rows, c, r)
            assert height[c] == int(m[c + 1:, c].sum())
        # the first block column in which a block row is active (without an envelope: column 0 for every row)
        want_first = [0 if last is None else int(np.argmax(m[i, :i + 1])) for i in range(nblk)]
        assert list(first) == want_first, (nblk, last, tail, ncols, tail_rows)
        # 128^3 (1/3 + h + h^2) per factored block column of h active block rows below the diagonal
        want = sum(128.0 ** 3 * (1.0 / 3.0 + h + h * h) for h in (int(m[c + 1:, c].sum()) for c in range(ncols)))
        assert abs(flops - want) <= 1e-12 * want  # (a sum of at most 40 terms in double precision)


def test_a_full_matrix_sums_to_a_third_of_n_cubed():
    nblk = 24
    active, height, first, flops = _probe(nblk, None, None, nblk, 1)
    assert list(height) == [nblk - 1 - c for c in range(nblk)] and not first.any()
    n = 128.0 * nblk
    assert abs(flops - n ** 3 / 3.0) <= 1e-12 * flops
