"""The front layouts of sk_cholesky_solve* without a device (skeres_amd/csrc/chol_fronts.cpp): the argument errors through the ABI —
they are decided from host data, before a device is asked for, so the return code and the text of sk_last_error() are the same
with and without one — and the stand-alone layout check under the host sanitizers (tools/chol_fronts_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import skeres_amd as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _system(n):
    A = np.diag(np.full(n, 4.0))
    for i in range(1, n):
        A[i, i - 1] = 1.0
    return A, np.ones(n), np.full(n, np.nan)


def _refused(rc, text, x):
    assert rc == INVALID_ARGUMENT
    assert sk.lib().sk_last_error().decode() == text
    assert np.isnan(x).all()  # nothing was written


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def test_a_last_that_is_no_envelope_is_refused():
    A, b, x = _system(200)  # two block columns
    for last, column in (([1, 0], 1), ([2, 2], 0), ([-1, 1], 0), ([1, 2], 1)):
        keep, lp = _i(last)
        _refused(sk.lib().sk_cholesky_solve_ex(200, _d(A), _d(b), _d(x), _dp(), 0, lp, 0), "invalid block envelope at block column %d" % column, x)


def test_a_border_outside_the_matrix_is_refused():
    A, b, x = _system(8)
    for begin in (-1, 9):
        _refused(sk.lib().sk_cholesky_solve_bordered(8, _d(A), _d(b), _d(x), _dp(), 0, begin, 0), "invalid argument", x)


def test_a_tail_that_couples_with_the_head_is_refused():
    A, b, x = _system(8)
    A[6, 1] = 0.5
    _refused(sk.lib().sk_cholesky_solve_dissected(8, _d(A), _d(b), _d(x), 3, 5, 0, 0), "the tail couples with the head at (6, 1): not a separator", x)
    for head, tail_begin in ((-1, 5), (5, 3), (3, 9)):
        _refused(sk.lib().sk_cholesky_solve_dissected(8, _d(A), _d(b), _d(x), head, tail_begin, 0, 0), "invalid argument", x)


def test_overlapping_or_reversed_cuts_are_refused():
    A, b, x = _system(12)
    for cuts in ([3, 6, 5, 8], [4, 3, 7, 8], [3, 4, 7, 13], [-1, 2, 7, 8]):
        keep, cp = _i(cuts)
        _refused(sk.lib().sk_cholesky_solve_segments(12, _d(A), _d(b), _d(x), 3, cp, 0, 0), "invalid cuts", x)


def test_rows_that_couple_across_a_separator_are_refused():
    A, b, x = _system(12)
    A[9, 5] = 0.5  # behind separator 2 = rows [7, 8), before it — and not behind separator 1's reach
    keep, cp = _i([3, 4, 7, 8])
    _refused(sk.lib().sk_cholesky_solve_segments(12, _d(A), _d(b), _d(x), 3, cp, 0, 0),
             "rows behind separator 2 couple with rows before it at (9, 5): not a separator", x)
    A[9, 1] = 0.5
    _refused(sk.lib().sk_cholesky_solve_segments(12, _d(A), _d(b), _d(x), 3, cp, 0, 0),
             "rows behind separator 1 couple with rows before it at (9, 1): not a separator", x)


def test_fewer_than_two_segments_are_refused():
    A, b, x = _system(8)
    keep, cp = _i([3, 4])
    for num_segments in (1, 0, -2):
        _refused(sk.lib().sk_cholesky_solve_segments(8, _d(A), _d(b), _d(x), num_segments, cp, 0, 0), "invalid argument", x)
    _refused(sk.lib().sk_cholesky_solve_segments(8, _d(A), _d(b), _d(x), 2, _ip(), 0, 0), "invalid argument", x)


def test_front_layouts_under_the_host_sanitizers(tmp_path):
    """tools/chol_fronts_check.cpp is a stand-alone program over the host-only sources: address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "chol_fronts_check")
    srcs = [os.path.join(ROOT, "tools", "chol_fronts_check.cpp")] + [os.path.join(ROOT, "skeres_amd", "csrc", f) for f in ("chol_fronts.cpp", "chol_envelope.cpp")]
    out = subprocess.run(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "chol_fronts_check ok: 20 systems" in run.stdout
