"""The argument rules of the segmented entry points without a GPU: the gcc build of csrc/pglm_gof.h's pgl_gof_bad_count and
pgl_gof_bad_offsets (tests/csrc/gof_args_host.c).  The verdict and the reported position on the shapes a caller can get
wrong, and agreement with the loop pgl_ks_uniform carried before (written out in the C file as it stood) over a seeded
table of 200 offset vectors with planted faults -- one at every position of a vector of 8 segments among them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'gof_args_host.c')
MAXN = 40


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='gof_args_host_'), 'gof_args_host.so')
    subprocess.check_call(['gcc', '-O2', '-Wall', '-Werror', '-shared', '-fPIC', '-o', so, SRC, '-lm'])
    L = C.CDLL(so)
    L.gof_args_count.argtypes = [C.c_longlong]
    L.gof_args_offsets.argtypes = [C.c_void_p, C.c_longlong]
    L.gof_args_offsets.restype = C.c_longlong
    L.gof_args_old_ks.argtypes = [C.c_void_p, C.c_longlong]
    L.gof_args_table.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.gof_args_table.restype = None
    return L


def _offsets(lib, off):
    a = np.ascontiguousarray(off, dtype=np.int64)
    return int(lib.gof_args_offsets(a.ctypes.data, a.size - 1)), int(lib.gof_args_old_ks(a.ctypes.data, a.size - 1))


@pytest.mark.parametrize('off, want', [
    ([0, 0, 0, 0], 0),                       # empty segments
    ([0, 0], 0),
    ([0, 5], 0),                             # a single segment
    ([3, 3, 7], 0),                          # (a first offset above 0 is allowed)
    ([-1, 0, 3], 1),                         # a negative first offset
    ([-1, -1], 1),
    ([-2, -3], 1),                           # (the first fault is the one reported)
    ([2, 1, 3, 4], 2),                       # a decrease at the first,
    ([0, 2, 4, 3, 9], 4),                    # a middle
    ([0, 1, 5, 4], 4),                       # and the last position
    ([0, 1, 0, 5, 4], 3),
])
def test_offsets_verdict_and_position(lib, off, want):
    new, old = _offsets(lib, off)
    assert new == want
    assert old == (want != 0)


def test_segment_count(lib):
    for M, bad in ((0, 1), (1, 0), (-1, 1), (2 ** 31 - 1, 0), (2 ** 31, 1), (2 ** 31 - 2, 0), (2 ** 62, 1), (-2 ** 62, 1)):
        assert lib.gof_args_count(M) == bad, M


def test_new_rule_and_old_loop_agree_on_the_table(lib):
    assert lib.gof_args_ntable() == 200
    seen = set()
    n_fault = 0
    for k in range(200):
        off = np.full(MAXN + 1, -77, dtype=np.int64)
        n, want = C.c_longlong(), C.c_longlong()
        lib.gof_args_table(k, off.ctypes.data, C.byref(n), C.byref(want))
        n, want = n.value, want.value
        assert 1 <= n <= MAXN and 0 <= want <= n + 1
        if want:                             # the table's own claim, restated: the fault is where it says and the first
            p = want - 1
            assert (off[0] < 0) if p == 0 else (off[0] >= 0 and np.all(np.diff(off[:p]) >= 0) and off[p] < off[p - 1])
        else:
            assert off[0] >= 0 and np.all(np.diff(off[:n + 1]) >= 0)
        new, old = _offsets(lib, off[:n + 1])
        assert new == want, k
        assert old == (want != 0), k
        if n == 8 and k < 9:
            seen.add(want - 1)
        n_fault += want != 0
    assert seen == set(range(9))             # every position of the 8-segment vector
    assert 100 < n_fault < 200
