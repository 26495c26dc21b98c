"""The launch plan of the collapsed-Gibbs columns (theano_pyglm_amd/csrc/pglm_gibbs_plan.h, built for the host with gcc through
tests/csrc/gibbs_plan_host.c) against the independent statement of the same rule in tests/gibbs_reference.py (geometry,
dbg_nloop, update_geometry), field by field and on the CPU: the cases of tests/gibbs_cases.json, the debug words of the sweep,
and a grid of shapes that reaches the unforced loops above 1 which the case table never does."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import pytest

from tests import gibbs_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS_CASES = [c for c in GR.load_cases() if c['form'] == 'cols']
WORDS = [GR.dbg_word(n) for n in (16, 1, 8, 2, 3, 0)] + [15 << 8, 16 << 8, 31 << 16]
REGIME_KEYS = ('CP', 'nsplit', 'ygroups', 'nloop', 'nblk', 'sblk', 'same_pre', 'nsub', 'grid', 'hs_region', 'fs_stride', 'lds')
F64_KEYS = ('CP', 'ygroups', 'nblk', 'gtb', 'rows', 'lds')
OUT = ('path', 'CP', 'nsplit', 'ygroups', 'nloop', 'nblk', 'sblk', 'same_pre', 'gtb', 'rows', 'nsub', 'grid', 'hs_region',
       'fs_stride', 'lds', 'dbg')


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='gibbs_plan_host_'), 'gibbs_plan_host.so')
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'gibbs_plan_host.c')])
    Lb = C.CDLL(so)
    Lb.gp_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                           C.c_longlong, C.c_void_p]
    Lb.gp_update.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    return Lb


def _plan(lib, ncols, K, n_pre, nrows, max_ev, nlin, opt_gibbs, opt_dbg, R=179, B=5, num_cu=GR.NUM_CU, slots=GR.WG_PER_CU * GR.NUM_CU):
    out = (C.c_longlong * 16)()
    n_pre = list(n_pre)
    lib.gp_plan(ncols, K, int(all(j == n_pre[0] for j in n_pre)), nrows, max_ev, int(nlin == 'explinear'), opt_gibbs, opt_dbg, B, R,
                num_cu, slots, out)
    return dict(zip(OUT, out))


def _same(dev, g, what):
    """every field of the reference's statement against the compiled header; what a path does not use reads as the host reports it"""
    if g['path'] == 'regime':
        assert dev['path'] == 0 and dev['gtb'] == 0 and dev['rows'] == 0, what
        keys = REGIME_KEYS
    else:
        assert dev['path'] == 1 and (dev['nsplit'], dev['nloop'], dev['sblk'], dev['same_pre']) == (1, 1, 0, 0), what
        keys = F64_KEYS
    assert dict((k, dev[k]) for k in keys) == dict((k, int(g[k])) for k in keys), (what, dev, g)


def test_constants_are_the_references(lib):
    out = (C.c_int * 7)()
    lib.gp_consts(out)
    assert list(out) == [GR.KMAX, GR.GRB, GR.GQ, GR.GNL, GR.GECAP, GR.GECAP_R, GR.SPT_N]


def test_debug_word_decoder(lib):
    """ablation byte in bits 0..7, the 4-bit loop in 8..11, the same_pre switch in bit 12, the 5-bit loop in 16..20: the 5-bit
    field wins when it is non-zero, and 16 << 8 forces nothing"""
    out = (C.c_int * 3)()
    for n5, off, n4, ab in itertools.product(range(32), (0, 1), range(16), (0, 1, 0x5a, 0xff)):
        word = n5 << 16 | off << 12 | n4 << 8 | ab
        lib.gp_dbg(word, out)
        assert list(out) == [ab, off, GR.dbg_nloop(word)] and GR.dbg_nloop(word) == (n5 or n4), hex(word)
    lib.gp_dbg(16 << 8, out)
    assert list(out) == [0, 1, 0]
    for word in (0x2000, 0x8000, 1 << 21, 1 << 30):                # bits the Gibbs path does not read
        lib.gp_dbg(word, out)
        assert list(out) == [0, 0, 0], hex(word)


@pytest.mark.parametrize('c', COLS_CASES, ids=lambda c: c['name'])
def test_case_table(lib, c):
    p = GR.problem(c)
    t_lo, t_hi = GR.case_range(c)
    mx = GR.max_events(c, c['cols'], t_lo, t_hi)
    word = GR.dbg_word(c.get('nloop', 0))
    for kern in (0, 1):
        g = GR.case_geometry(c, kern)
        dev = _plan(lib, len(c['cols']), len(c['w']), c['pre'], t_hi - t_lo, mx, p.kind, kern, word, R=GR.taps(p), B=p.B)
        _same(dev, g, (c['name'], kern))
        assert dev['dbg'] == 0


def test_debug_words_with_equal_and_distinct_pre(lib):
    c = [c for c in COLS_CASES if c['name'] == 'nloop_3'][0]
    p = GR.problem(c)
    t_lo, t_hi = GR.case_range(c)
    mx = GR.max_events(c, c['cols'], t_lo, t_hi)
    ncols = len(c['cols'])
    assert ncols >= 2
    for word, pre, kern in itertools.product(WORDS, ([4] * ncols, list(range(ncols))), (0, 1)):
        g = GR.geometry(ncols, len(c['w']), pre, t_hi - t_lo, mx, p.kind, kern, R=GR.taps(p), opt_dbg=word, B=p.B)
        _same(_plan(lib, ncols, len(c['w']), pre, t_hi - t_lo, mx, p.kind, kern, word, R=GR.taps(p), B=p.B), g, (hex(word), pre, kern))
        if kern == 0:
            assert g['same_pre'] == (pre[0] == pre[-1] and not word & 0x1000)


def test_grid_of_shapes(lib):
    """ncols 1..20 x K 1..16 x nrows x max_ev x both nonlinearities x slots: with 4 slots the unforced nloop rises above 1, to
    its cap of 8"""
    loops = set()
    n = 0
    for ncols, K, nrows, max_ev, nlin, slots in itertools.product(range(1, 21), range(1, 17), (1, 37, 255, 256, 257, 768, 1892, 300000),
                                                                  (0, 1, 256, 257), ('explinear', 'exp'), (4, 1024)):
        pre = [3] * ncols if (ncols + K) % 2 else list(range(ncols))
        g = GR.geometry(ncols, K, pre, nrows, max_ev, nlin, slots=slots)
        _same(_plan(lib, ncols, K, pre, nrows, max_ev, nlin, 0, 0, slots=slots), g, (ncols, K, nrows, max_ev, nlin, slots))
        if g['path'] == 'regime':
            loops.add(g['nloop'])
        n += 1
    assert {1, 8} <= loops and n == 20 * 16 * 8 * 4 * 2 * 2
    # the loops in between: 24 k sub-blocks of one column group on 4 slots make a loop of k
    for k, ncols in itertools.product(range(1, 10), (1, 8, 9)):
        nrows = GR.GRB * 24 * k - 5
        g = GR.geometry(ncols, 11, range(ncols), nrows, 30, 'explinear', slots=4)
        _same(_plan(lib, ncols, 11, range(ncols), nrows, 30, 'explinear', 0, 0, slots=4), g, (k, ncols))
        loops.add(g['nloop'])
        assert ncols > 1 or g['nloop'] == min(k, 8)
    assert loops == set(range(1, 9))


def test_update_geometry(lib):
    out = (C.c_longlong * 5)()
    for ncols, nrows, (R, B) in itertools.product(list(range(1, 21)) + [255, 256, 257, 600], (1, 1023, 1024, 1025, 1892, 300000),
                                                  ((179, 5), (64, 3))):
        lib.gp_update(ncols, nrows, B, R, out)
        g = GR.update_geometry(ncols, nrows, R=R, B=B)
        assert dict(zip(('CP', 'ygroups', 'rows', 'nblk', 'lds'), out)) == g, (ncols, nrows)
