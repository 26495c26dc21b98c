"""Dense per-neuron Hessians of ll on the device (pgl_hess_dev / pgl_hess) against the numpy float64 Gram matrix
F^T (c o F) built from tests/test_hvp_host.py's features and curvature (both held to the oracle's second derivative there).
Bound: the project's own for second-order quantities, max|H_dev - H_ref| <= 1e-9 max|H_ref| per neuron."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_hvp_host import features, curvature
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _torch():
    import torch
    return torch


def ref_hessian(p, neurons, t_lo=0, t_hi=None):
    t_hi = p.nT if t_hi is None else t_hi
    out = np.empty((len(neurons), p.P, p.P))
    for i, n in enumerate(neurons):
        F = features(p, n)
        c = curvature(F.dot(p.theta[n]), p.S[:, n].astype(float), p.kind, p.dt)
        F, c = F[t_lo:t_hi], c[t_lo:t_hi]
        out[i] = F.T @ (c[:, None] * F)
    return out


def _dev_hess(d, theta, Weff, n_lo=0, n_hi=None, idx=None, ld=None, ncalls=1, prepare=True):
    """prepare + pgl_hess_dev with device buffers (torch tensors as the allocator); the buffer is filled with NaN first.
    Returns the (rows, P, ld) results of `ncalls` calls after the one prepare, and the kernels of the prepare."""
    torch = _torch()
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(Weff)
    rows, P = theta.shape
    ld = P if ld is None else ld
    names = None
    if idx is not None:
        d_idx = torch.tensor(np.asarray(idx), dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), d_idx=d_idx.data_ptr(), count=len(idx))
    else:
        torch.cuda.synchronize()
        d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), n_lo, n_hi)
    try:
        names = d.last_kernels()
    except _lib.PglError:
        pass
    outs = []
    for _ in range(ncalls):
        d_H = torch.full((rows, P, ld), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        d.hess(d_H.data_ptr(), ld)
        d.sync()
        outs.append(d_H.cpu().numpy().copy())
    return outs, names


def _worst(Hd, Hr):
    return max(np.max(np.abs(a - b)) / np.max(np.abs(b)) for a, b in zip(Hd, Hr))


CASES = [
    # (name, N, nT, kind, problem kwargs, Dstim)
    ('N4-explinear', 4, 3000, 'explinear', {}, 0),                    # P = 21: one ragged column block
    ('N4-exp', 4, 3000, 'exp', {}, 0),
    ('N32-explinear', 32, 3000, 'explinear', {}, 0),                  # P = 161: one column past ten tiles
    ('N32-explinear-zero', 32, 3000, 'explinear', {'bias_mu': 1.0, 'w_scale': 0.5}, 0),
    ('N64-Dstim9', 64, 3000, 'explinear', {}, 9),                     # dense stimulus columns
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_hessian_matches_reference(case):
    name, N, nT, kind, kw, Dstim = case
    p = H.Problem(N, nT, H.std_ibasis(200), kind=kind, Dstim=Dstim, seed=17, weighted=True, **kw)
    ref = ref_hessian(p, range(N))
    d = p.device(0)
    try:
        Hh = d.hessian(p.theta, p.Weff)
        e1 = _worst(Hh, ref)
        Hd = _dev_hess(d, p.theta, p.Weff, 0, N)[0][0]
        e2 = _worst(Hd, ref)
        print("%s: one-shot %.3e, prepare + hess %.3e of max|H|" % (name, e1, e2))
        assert e1 <= TOL and e2 <= TOL
        assert np.array_equal(Hd, Hd.transpose(0, 2, 1))
    finally:
        d.close()


@pytest.fixture(scope='module')
def c3():
    """N = 128 at a short recording (4 800 bins = 300 tiles): the prepare leaves c in the accumulator-layout slab."""
    p = H.Problem(128, 4800, H.std_ibasis(200), kind='explinear', seed=29, weighted=True, bias_mu=1.0, w_scale=0.5)
    return p, ref_hessian(p, range(128))


def test_hessian_c3_class_reads_the_curvature_slab(c3):
    p, ref = c3
    N = p.N
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        outs, prep = _dev_hess(d, p.theta, p.Weff, 0, N, ncalls=2)
        print("N=128: worst %.3e of max|H|; prepare %s, hess %s" % (_worst(outs[0], ref), prep, d.last_kernels()))
        assert prep == ['k_hvp5<18, 22, 1>']
        assert d.last_kernels() == ['k_hess<1>']
        assert _worst(outs[0], ref) <= TOL
        assert np.array_equal(outs[0], outs[0].transpose(0, 2, 1))       # both triangles: the same bits
        assert np.array_equal(outs[0], outs[1])                           # two calls after one prepare
        # H v against the device product
        V = np.random.default_rng(31).standard_normal((N, p.P))
        hv = d.hvp(p.theta, V, p.Weff)
        Hv = np.einsum('nij,nj->ni', outs[0], V)
        e = np.max(np.abs(Hv - hv)) / np.max(np.abs(hv))
        print("H v against pgl_hvp: %.3e of max|H v|" % e)
        assert e <= 1e-9
        # a sub-range with a ragged last post tile, and a neuron list
        lo, hi = 40, 113
        o, prep = _dev_hess(d, p.theta[lo:hi], p.Weff, lo, hi)
        assert prep == ['k_hvp5<18, 22, 1>']
        print("sub-range: %.3e" % _worst(o[0], ref[lo:hi]))
        assert _worst(o[0], ref[lo:hi]) <= TOL
        idx = np.random.default_rng(37).permutation(N)[:70]
        o, prep = _dev_hess(d, p.theta[idx], p.Weff, idx=idx)
        assert prep == ['k_hvp5<18, 22, 1>']
        print("list: %.3e" % _worst(o[0], ref[idx]))
        assert _worst(o[0], ref[idx]) <= TOL
    finally:
        d.close()


def test_hessian_c3_time_ranges_and_padding(c3):
    """pgl_set_time_range takes t_lo on the 16-bin tile grid only, so the split of the recording is at bin 2000 (tile 125, on
    no coarser grid: the chunks of either part start and end off the other's); a range that ends inside a tile (t_hi =
    2007) is held to the reference on its own."""
    p, ref = c3
    N, nT = p.N, p.nT
    split, ragged = 2000, 2007
    sub = list(range(0, N, 9))
    d = p.device(0)
    try:
        # ld = P + 3: the padding columns stay NaN
        whole = _dev_hess(d, p.theta, p.Weff, 0, N, ld=p.P + 3)[0][0]
        assert np.all(np.isnan(whole[:, :, p.P:]))
        whole = whole[:, :, :p.P]
        assert _worst(whole, ref) <= TOL
        d.set_time_range(0, split)
        first = _dev_hess(d, p.theta, p.Weff, 0, N)[0][0]
        d.set_time_range(split, nT)
        second = _dev_hess(d, p.theta, p.Weff, 0, N)[0][0]
        print("time ranges: first + second against the whole %.3e, against the reference %.3e"
              % (_worst(first + second, whole), _worst(first + second, ref)))
        assert _worst(first + second, whole) <= TOL and _worst(first + second, ref) <= TOL
        d.set_time_range(0, ragged)
        part = _dev_hess(d, p.theta, p.Weff, 0, N)[0][0]
        e = _worst(part[sub], ref_hessian(p, sub, 0, ragged))
        print("range [0, %d): %.3e" % (ragged, e))
        assert e <= TOL
    finally:
        d.close()


def test_hessian_wide_population_list():
    """N = 144 (P = 721: the 3-phase prepare, c as rows), a list of 40 neurons."""
    p = H.Problem(144, 2000, H.std_ibasis(200), kind='explinear', seed=43, weighted=True)
    idx = np.random.default_rng(47).permutation(144)[:40]
    ref = ref_hessian(p, idx)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        o, _ = _dev_hess(d, p.theta[idx], p.Weff, idx=idx)
        assert d.last_kernels() == ['k_hess<0>']
        print("N=144 list: %.3e of max|H|" % _worst(o[0], ref))
        assert _worst(o[0], ref) <= TOL
        assert np.array_equal(o[0], o[0].transpose(0, 2, 1))
    finally:
        d.close()


def test_hessian_error_paths():
    torch = _torch()
    p = H.Problem(8, 2000, H.std_ibasis(200), seed=67)
    d = p.device(0)
    try:
        d_H = torch.empty((8, p.P, p.P), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        with pytest.raises(_lib.PglError, match="error -3"):          # before prepare
            d.hess(d_H.data_ptr(), p.P)
        d.hessian(p.theta, p.Weff)                                     # prepared now
        d.hess(d_H.data_ptr(), p.P)
        d.sync()
        with pytest.raises(_lib.PglError, match="error -1"):          # ld < P
            d.hess(d_H.data_ptr(), p.P - 1)
        d.set_time_range(0, 1600)
        with pytest.raises(_lib.PglError, match="error -3"):          # the time range changed
            d.hess(d_H.data_ptr(), p.P)
        d.set_time_range(0, p.nT)
        d.hess(d_H.data_ptr(), p.P)
        d.sync()
        stim = np.random.default_rng(71).standard_normal((20, 6))
        d.set_stimulus_separable(stim, 0.1, H.std_ibasis(200)[:, :3])
        with pytest.raises(_lib.PglError, match="error -4.*separable"):
            d.hess(d_H.data_ptr(), d.P)
        with pytest.raises(_lib.PglError, match="error -4.*separable"):
            d.hessian(np.zeros((8, d.P)), p.Weff)
    finally:
        d.close()
