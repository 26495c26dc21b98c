"""k_filter_bands on the device against the gcc build of its rule (tests/csrc/filters_host.c over csrc/pglm_filters.h), bit for
bit, over tests/filter_cases.json; two calls, a group alone, the host-pointer form, the refusals, the host route above the cap,
and the samplers' 'filters' against filter_bands of the returned draws."""
import ctypes as C

import numpy as np
import pytest

from tests import filter_reference as FR
from tests import helpers as H
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e250
CASES = FR.load()


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)      # (the handle supplies the stream only)
    yield h
    h.close()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _run(handle, x, n_chains, first, G, basis, c, level):
    """pgl_filter_bands_dev through the tensor form; the outputs have a sentinel row in front and behind, and the draws must
    come back unchanged"""
    import torch
    n, M = x.shape[0], x.shape[1] // n_chains
    R = basis.shape[0]
    d = _t(x)
    out = _t(np.full((M + 2, G, R, 5), SENTINEL))
    grp = _t(np.full((M + 2, G, 8), SENTINEL))
    torch.cuda.synchronize()                                 # (the handle's stream does not wait for torch's)
    handle.filter_bands(d, n_chains, first, G, _t(basis), _t(c), level, out=out[1:-1], grp=grp[1:-1])
    handle.sync()
    o, g = out.cpu().numpy(), grp.cpu().numpy()
    for a in (o, g):
        assert np.all(a[0] == SENTINEL) and np.all(a[-1] == SENTINEL)
    assert np.array_equal(d.cpu().numpy(), x, equal_nan=True)
    return o[1:-1], g[1:-1]


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_case_equals_the_gcc_mirror_bit_for_bit(handle, c):
    a = FR.args(c)
    out, grp = _run(handle, *a)
    want_out, want_grp = FR.host_bands(*a)
    assert FR.same_bits(grp, want_grp), np.argwhere(~(np.isclose(grp, want_grp, rtol=0, atol=0, equal_nan=True)))[:5]
    assert FR.same_bits(out, want_out), np.argwhere(~(np.isclose(out, want_out, rtol=0, atol=0, equal_nan=True)))[:5]
    for m in range(c['M']):
        for g in range(c['G']):
            assert grp[m, g, 7] == (1.0 if FR.bad_group(c, m, g) else 0.0)
    again = _run(handle, *a)                                                          # two calls: equal bits
    assert FR.same_bits(again[0], out) and FR.same_bits(again[1], grp)


def test_a_group_alone_equals_itself_among_5_groups_and_3_rows(handle):
    c = [c for c in CASES if c['name'] == 's63'][0]
    assert (c['G'], c['M']) == (5, 3)
    x, nc, first, G, basis, cc, level = FR.args(c)
    out, grp = _run(handle, x, nc, first, G, basis, cc, level)
    for m, g in ((0, 0), (1, 3), (2, 4)):
        o1, g1 = _run(handle, np.ascontiguousarray(x[:, m:m + 1]), nc, first + g * c['B'], 1, basis, cc, level)
        assert FR.same_bits(o1[0, 0], out[m, g]) and FR.same_bits(g1[0, 0], grp[m, g])


def test_host_pointer_form_is_the_same_call(handle):
    c = [c for c in CASES if c['name'] == 's1000_c4_nan_inf'][0]
    a = FR.args(c)
    out, grp = _run(handle, *a)
    ho, hg = handle.filter_bands_host(*a)
    assert FR.same_bits(ho, out) and FR.same_bits(hg, grp)


def test_refusals_launch_nothing(handle):
    import torch
    assert _lib.FILT_MAX_DRAWS == FR.lib().filters_max_draws() and _lib.FILT_MAX_B == FR.lib().filters_max_b()
    x = torch.zeros((8, 2, 40), dtype=torch.float64, device='cuda')
    basis = torch.ones((3, 17), dtype=torch.float64, device='cuda')
    cc = torch.ones(17, dtype=torch.float64, device='cuda')
    out = torch.full((2, 2, 3, 5), SENTINEL, dtype=torch.float64, device='cuda')
    grp = torch.full((2, 2, 8), SENTINEL, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    lib, p = handle.lib, lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(xs=x, n=8, Cn=1, M=2, P=40, first=1, G=2, B=5, bs=basis, R=3, c=cc, level=0.95, o=out, g=grp, h=handle.h):
        return lib.pgl_filter_bands_dev(h, p(xs), n, Cn, M, P, first, G, B, p(bs), R, p(c), level, p(o), p(g))

    ARG, UNSUPPORTED = -1, -4
    assert call(B=17, G=2) == UNSUPPORTED and "PGL_FILT_MAX_B" in _lib.load().pgl_last_error().decode()
    assert call(n=_lib.FILT_MAX_DRAWS + 1) == UNSUPPORTED and "PGL_FILT_MAX_DRAWS" in _lib.load().pgl_last_error().decode()
    assert call(n=1025, Cn=4) == UNSUPPORTED
    assert call(M=65536) == UNSUPPORTED
    for kw in (dict(n=1), dict(n=0), dict(Cn=0), dict(M=0), dict(G=0), dict(B=0), dict(R=0), dict(first=-1), dict(first=31),
               dict(level=0.0), dict(level=1.0), dict(level=float('nan')), dict(xs=None), dict(bs=None), dict(c=None), dict(o=None),
               dict(g=None), dict(h=None)):
        assert call(**kw) == ARG, kw
    assert lib.pgl_filter_bands(handle.h, None, 8, 1, 2, 40, 1, 2, 5, None, 3, None, 0.95, None, None) == ARG
    with pytest.raises(ValueError):
        handle.filter_bands(x.cpu(), 1, 1, 2, basis[:, :5].contiguous(), cc[:5].contiguous(), 0.95)
    with pytest.raises(ValueError):
        handle.filter_bands(x, 3, 1, 2, basis[:, :5].contiguous(), cc[:5].contiguous(), 0.95)
    handle.sync()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(grp.cpu().numpy() == SENTINEL)


def _same_result(a, b):
    for k in ('c_sim', 'weight_mean', 'weight_sd', 'weight_q_lo', 'weight_median', 'weight_q_hi', 'p_pos'):
        assert FR.same_bits(a[k], b[k]), k
    for k in ('mean', 'sd', 'q_lo', 'median', 'q_hi'):
        assert FR.same_bits(a['impulse'][k], b['impulse'][k]), k
    assert np.array_equal(a['info'], b['info']) and np.array_equal(a['excl_zero'], b['excl_zero'])
    assert np.array_equal(a['lags'], b['lags']) and ('stim' in a) == ('stim' in b)
    if 'stim' in a:
        for k in ('mean', 'sd', 'q_lo', 'median', 'q_hi', 'c_sim', 'weight_mean', 'p_pos'):
            assert FR.same_bits(a['stim'][k], b['stim'][k]), k


@pytest.mark.parametrize('sampler', ['hmc', 'nuts'])
def test_sampler_filters_equal_filter_bands_of_the_draws(sampler):
    """N = 4, 3 000 bins, 2 chains, 64 kept draws: 'filters' of the sampler = filter_bands of the returned samples (numpy and
    torch input), bit for bit; 'samples' = the filters=False run, which has no 'filters'; 4 097 draws take the host route."""
    import torch
    from tests.test_gpu_hvp import _std_population
    from theano_pyglm_amd.inference import filters as F
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc
    from theano_pyglm_amd.inference.batched_nuts import sample_glms_nuts
    popn = _std_population(4, 3.0, 31, basis_stim=(sampler == 'nuts'), nlin='exp', bias_mu=3.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        if sampler == 'hmc':
            run = lambda **kw: sample_glms_hmc(popn, x, n_samples=64, n_warmup=20, n_chains=2, n_leapfrog=3, step_sz=0.02,
                                               seed=4, **kw)
        else:
            run = lambda **kw: sample_glms_nuts(popn, x, n_samples=64, n_warmup=20, n_chains=2, max_depth=4, step_sz=0.02,
                                                seed=4, **kw)
        plain, with_f = run(), run(filters=True)
        assert 'filters' not in plain and 'filters' not in run(filters=False)
        assert np.array_equal(plain['samples'], with_f['samples'])
        f = with_f['filters']
        N, R = popn.N, popn.glm.imp_model.ibasis.shape[0]
        assert f['route'] == 'device' and f['impulse']['mean'].shape == (N, N, R) and f['c_sim'].shape == (N, N)
        assert f['lags'].shape == (R,) and f['excl_zero'].dtype == bool and np.all(f['info'] == 0)
        assert ('stim' in f) == (sampler == 'nuts')
        if 'stim' in f:
            assert f['stim']['mean'].shape == (N, 2, popn.glm.bkgd_model.ibasis.shape[0])
        for inp in (with_f, with_f['samples'], torch.tensor(with_f['samples'], dtype=torch.float64, device='cuda')):
            d = F.filter_bands(popn, inp)
            assert d['route'] == 'device'
            _same_result(d, f)
        host = F.filter_bands(popn, with_f['samples'], device=False)
        assert host['route'] == 'host'
        _same_result(host, f)
        if sampler == 'hmc':
            big = np.random.default_rng(0).normal(size=(_lib.FILT_MAX_DRAWS + 1, 1, popn.glm.P))
            b = F.filter_bands(popn, big)
            assert b['route'] == 'host'
            spec = F.filter_specs(popn)[0]
            o, g = F.filter_bands_numpy(big, 1, spec[1], spec[2], spec[3], spec[4], 0.95)
            assert FR.same_bits(b['impulse']['mean'], o[..., 0]) and FR.same_bits(b['c_sim'], g[..., 0])
            text = F.band_table(f, truth=np.eye(N, dtype=bool))
            print(text)
            assert text.startswith("filter bands (level 0.95, device)") and "simultaneous band" in text
    finally:
        popn.release_data()
