"""k_hess / k_hess_reduce over the shapes where their own geometry can break: tests/hessian_cases.json, one case per edge of
the 64-column blocking (B = 1 with 64 presynaptic neurons in a block, B = 7 straddling every boundary differently, K = 64,
K = 65, a block that starts exactly at Kimp, stimulus columns over two blocks), of the event staging (windows above and
below its 16 slots, explinear and exp), of the rows layout (sub-range and list off the 16 grid under a time range that
starts on an odd tile and ends inside one), of hess_plan's launches (72 rows of N = 256: 64 + 8) and of the slab layout
with exp.  tests/test_hessian_cases.py proves on the CPU that each case reaches what it names.

Per case: pgl_hvp_prepare_* + pgl_hess_dev over NaN, the launches the dry run names, and tests/hessian_reference.check:
finite, both triangles the same bits, max|dH| <= 1e-9 max|H_ref| per neuron, |dH[i,j]| <= gamma A[i,j] per element with
gamma = (bins + 4) 2^-53 + the curvature's own bound (derived there, not from k_hess), exact zeros where A == 0 -- the rows
and columns of a silent presynaptic neuron and of a zero in Weff among them, asserted by name as well.

Worst |dH| / (gamma A) per case on the MI355X: docs/NOTEBOOK.md, "Dense-Hessian sweep"."""
import numpy as np
import pytest

from tests import hessian_reference as HR
from tests.test_gpu_hessian import _dev_hess, _worst
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

CASES = HR.load_cases()
BIG_ROWS = (0, 7, 63, 64, 71)             # of the two-launch case: first and last row of either launch, the end of a group
_problems = {}


def _problem(c):
    key = tuple(repr(c[k]) for k in ('N', 'B', 'R', 'Dstim', 'nT', 'kind', 'rate_hz', 'burst', 'silent', 'seed'))
    if key not in _problems:
        _problems[key] = HR.problem(c)
    return _problems[key]


def _run(d, p, c, ids):
    if c['list']:
        outs, _ = _dev_hess(d, p.theta[ids], p.Weff, idx=ids)
    else:
        outs, _ = _dev_hess(d, p.theta[ids], p.Weff, int(ids[0]), int(ids[-1]) + 1)
    return outs[0]


def _assert_named_zeros(Hd, p, c, ids):
    """rows and columns of a silent presynaptic neuron / of Weff[n', n] == 0: exactly 0.0 (-0.0 passes, NaN does not)"""
    checked = 0
    for i, n in enumerate(ids):
        for m in list(c['silent']) + np.nonzero(p.Weff[:, n] == 0.0)[0].tolist():
            cols = slice(1 + c['Dstim'] + m * c['B'], 1 + c['Dstim'] + (m + 1) * c['B'])
            assert np.all(Hd[i, cols, :] == 0.0) and np.all(Hd[i, :, cols] == 0.0), (c['name'], int(n), int(m))
            checked += 1
    assert checked >= len(ids) * len(c['silent']) and checked > 0


def _two_launches(d, p, c, ids):
    """The output stays on the device (0.95 GB): finite and symmetric there for every row, BIG_ROWS held to the reference."""
    import torch
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W = t(p.theta[ids]), t(p.Weff)
    d_idx = torch.tensor(np.asarray(ids), dtype=torch.int32, device='cuda')
    d_H = torch.full((len(ids), p.P, p.P), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), d_idx=d_idx.data_ptr(), count=len(ids))
    d.hess(d_H.data_ptr(), p.P)
    d.sync()
    assert d.last_kernels() == [c['kernel']] * c['launches'], d.last_kernels()
    for r in range(len(ids)):
        assert bool(torch.isfinite(d_H[r]).all()), "row %d: not finite (never written?)" % r
        assert bool((d_H[r] == d_H[r].T).all()), "row %d: the two triangles differ" % r
    rows = list(BIG_ROWS)
    return d_H[rows].cpu().numpy(), ids[rows]


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_hessian_case(c):
    p = _problem(c)
    ids = HR.neurons(c)
    t_lo, t_hi = HR.time_range(c)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d.set_time_range(t_lo, t_hi)
        if c['launches'] >= 2:
            Hd, ids = _two_launches(d, p, c, ids)
        else:
            Hd = _run(d, p, c, ids)
            assert d.last_kernels() == [c['kernel']], d.last_kernels()
        Hr, A = HR.ref_hessian(p, ids, t_lo, t_hi)
        HR.check(Hd, Hr, A, t_hi - t_lo, c['name'])
        _assert_named_zeros(Hd, p, c, ids)
    finally:
        d.close()


def test_rows_layout_halves_of_a_split_recording_add_up():
    """The rows layout under pgl_set_time_range: [0, 400) (25 tiles) and [400, nT) of the rows-list case, each against its
    own reference, and their sum against the whole recording."""
    c = [c for c in CASES if c['name'] == 'rows-list'][0]
    p = _problem(c)
    ids = HR.neurons(c)
    split = c['t_lo']
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        parts = []
        for lo, hi in ((0, p.nT), (0, split), (split, p.nT)):
            d.set_time_range(lo, hi)
            Hd = _run(d, p, c, ids)
            assert d.last_kernels() == ['k_hess<0>']
            Hr, A = HR.ref_hessian(p, ids, lo, hi)
            HR.check(Hd, Hr, A, hi - lo, "rows-list [%d, %d)" % (lo, hi))
            parts.append(Hd)
        e = _worst(parts[1] + parts[2], parts[0])
        print("first + second against the whole: %.3e of max|H|" % e)
        assert e <= HR.TOL
    finally:
        d.close()
