"""k_diag_column (pgl_chain_diag_dev) over the case table of tests/diag_reference.py -- every n, C, S and h at which the
kernel's loops, its batches of lags and its thread groups change, K = 1, 3, 161, the contents that reach each branch of the
rule -- against the longdouble reference: the sums at the derived bound 8 n 2^-53 sum |terms|, the composed rows at 100 e0,
the truncation lags and the NaN / zero patterns exactly (tests/test_diag_host.py proves on the CPU that the reference keeps
every case and rejects five defects).  Padded input with sentinels, bit reproducibility, the refusals, diagnose on numpy and
torch input, and one run through sample_glms_hmc(..., diagnostics=True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import diag_reference as R
from tests import helpers as H
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
SENTINEL = -7.25e250


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)      # (the handle supplies the stream only)
    yield h
    h.close()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _run(handle, x, pad=0):
    """x (C, n, K) through pgl_chain_diag_dev in the samplers' layout, ld = K + pad with NaN padding; out (15, K).  The output
    buffer has a sentinel row in front and behind, and the input must come back unchanged."""
    Cn, n, K = x.shape
    a = R.device_layout(x, pad)
    d = _t(a)
    out = _t(np.full((_lib.DIAG_NOUT + 2, K), SENTINEL))
    import torch
    torch.cuda.synchronize()                                 # (the handle's stream does not wait for torch's)
    rc = handle.lib.pgl_chain_diag_dev(handle.h, C.c_void_p(d.data_ptr()), n, Cn, K, K + pad, C.c_void_p(out[1].data_ptr()))
    assert rc == 0, _lib.load().pgl_last_error()
    handle.sync()
    o = out.cpu().numpy()
    assert np.all(o[0] == SENTINEL) and np.all(o[-1] == SENTINEL)
    assert np.array_equal(d.cpu().numpy(), a, equal_nan=True)
    return o[1:-1]


@pytest.mark.parametrize('c', R.CASES, ids=[c['name'] for c in R.CASES])
def test_diag_case(handle, c):
    x, ref, margin = R.case_reference(c)
    out = _run(handle, x)
    e = R.errors(out, ref)
    print(c['name'], e, "ratio to the bounds", R.ratios(out, ref, x))
    assert np.array_equal(out[11:], ref[11:].astype(float), equal_nan=True)           # the truncation lags, exactly
    assert np.array_equal(np.isnan(out), np.isnan(ref.astype(float))) and np.array_equal(out == 0, ref.astype(float) == 0)
    assert R.within(out, ref, x), e
    assert np.array_equal(_run(handle, x), out, equal_nan=True)                       # two calls: equal bits
    padded = _run(handle, x, pad=3)                                                   # ld > K, the padding full of NaN
    assert np.array_equal(padded, out, equal_nan=True)


def test_host_pointer_form_is_the_same_call(handle):
    c = [c for c in R.CASES if c['name'] == 'ar50'][0]
    x, ref, _ = R.case_reference(c)
    out = _run(handle, x)
    host = handle.chain_diag_host(R.device_layout(x), n_chains=c['C'])
    assert host.shape == (_lib.DIAG_NOUT, 1, c['K']) and np.array_equal(host[:, 0], out, equal_nan=True)
    dev = handle.chain_diag(_t(R.device_layout(x)), n_chains=c['C'])
    handle.sync()
    assert np.array_equal(dev.cpu().numpy()[:, 0], out, equal_nan=True)


def test_a_column_alone_equals_itself_among_161(handle):
    c = [c for c in R.CASES if c['name'] == 'K161'][0]
    x, _, _ = R.case_reference(c)
    out = _run(handle, x)
    for j in (0, 77, 160):
        assert np.array_equal(_run(handle, x[:, :, j:j + 1])[:, 0], out[:, j], equal_nan=True)


def test_a_zero_order_statistic_is_plus_zero(handle):
    from tests.test_diag_host import zero_sign_draws
    x = zero_sign_draws()
    out = _run(handle, x)
    assert np.array_equal(out, R.host_mirror(x), equal_nan=True) and not np.any(np.signbit(out[[2, 3, 4], 1]))
    assert out[2, 0] == 0 and not np.signbit(out[2, 0])


def test_non_finite_column_touches_no_other(handle):
    c = [c for c in R.CASES if c['name'] == 'nonfinite'][0]
    x, _, _ = R.case_reference(c)
    out = _run(handle, x)
    clean = np.where(np.isfinite(x), x, 0.25)
    want = _run(handle, clean)
    bad = ~np.all(np.isfinite(x), axis=(0, 1))
    assert bad.sum() == 9 and np.all(np.isnan(out[:, bad])) and np.array_equal(out[:, ~bad], want[:, ~bad])


def test_refusals_launch_nothing(handle):
    import torch
    assert _lib.DIAG_MAX_DRAWS == R.MAX_DRAWS
    buf = torch.zeros((R.MAX_DRAWS + 8, 4), dtype=torch.float64, device='cuda')
    out = torch.full((_lib.DIAG_NOUT, 4), SENTINEL, dtype=torch.float64, device='cuda')
    p, o, lib = buf.data_ptr(), out.data_ptr(), handle.lib
    torch.cuda.synchronize()                                 # (the handle's stream does not wait for torch's)
    assert lib.pgl_chain_diag_dev(handle.h, p, R.MAX_DRAWS + 1, 1, 4, 4, o) == -4              # PGL_ERR_UNSUPPORTED
    assert lib.pgl_chain_diag_dev(handle.h, p, (R.MAX_DRAWS + 8) // 8, 8, 4, 4, o) == -4
    assert "PGL_DIAG_MAX_DRAWS" in _lib.load().pgl_last_error().decode()
    for args in ((p, 7, 1, 4, 4, o), (p, 8, 1, 4, 3, o), (p, 8, 0, 4, 4, o), (p, 8, 1, 0, 4, o), (None, 8, 1, 4, 4, o),
                 (p, 8, 1, 4, 4, None)):
        assert lib.pgl_chain_diag_dev(handle.h, *args) == -1                                   # PGL_ERR_ARG
    assert lib.pgl_chain_diag_dev(None, p, 8, 1, 4, 4, o) == -1
    assert lib.pgl_chain_diag(handle.h, None, 8, 1, 4, o) == -1
    with pytest.raises(_lib.PglError, match="PGL_DIAG_MAX_DRAWS"):
        handle.chain_diag(buf)
    with pytest.raises(_lib.PglError, match="PGL_DIAG_MAX_DRAWS"):
        handle.chain_diag_host(np.zeros((R.MAX_DRAWS + 1, 1)))
    with pytest.raises(ValueError):
        handle.chain_diag(buf[:16].cpu())
    with pytest.raises(ValueError):
        handle.chain_diag(buf[:16], n_chains=3)
    handle.sync()
    assert np.all(out.cpu().numpy() == SENTINEL) and float(buf.abs().sum()) == 0.0


def test_sampler_summary_and_diagnose():
    """2 neurons, 400 bins, 2 chains, 16 kept draws: 'summary' of sample_glms_hmc(..., diagnostics=True) = diagnose of the
    returned samples (numpy and torch input), bit for bit; 'samples' = the diagnostics=False run, bit for bit; above the cap
    diagnose runs the numpy statement."""
    import torch
    from tests.test_gpu_hvp import _std_population
    from theano_pyglm_amd.inference import diagnostics as D
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc
    popn = _std_population(2, 0.4, 31, nlin='exp', bias_mu=3.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        kw = dict(n_warmup=10, n_leapfrog=3, step_sz=0.02, seed=4, n_chains=2, init_jitter=0.1)
        plain = sample_glms_hmc(popn, x, 16, **kw)
        diag = sample_glms_hmc(popn, x, 16, diagnostics=True, **kw)
        assert 'summary' not in plain and np.array_equal(plain['samples'], diag['samples'])
        for k in ('accept_rate', 'step_sz'):
            assert np.array_equal(plain[k], diag[k])
        s = diag['summary']
        assert s['route'] == 'device' and set(s) == set(_lib.DIAG_ROWS) | {'route'}
        assert s['rhat'].shape == diag['samples'].shape[2:] == (2, popn.glm.P)
        for inp in (diag['samples'], torch.tensor(diag['samples'], dtype=torch.float64, device='cuda')):
            d = D.diagnose(popn, inp)
            assert d['route'] == 'device'
            for k in _lib.DIAG_ROWS:
                assert np.array_equal(d[k], s[k], equal_nan=True), k
        ref = D.chain_diagnostics(diag['samples'])
        for k in ('rhat', 'ess_bulk', 'ess_tail', 'mcse_mean'):
            assert np.allclose(s[k], ref[k], rtol=1e-10, equal_nan=True), k
        for k in R.LAGS:
            assert np.array_equal(s[k], ref[k]), k
        one = D.diagnose(popn, diag['samples'][0], chains=False)
        assert one['route'] == 'device' and np.allclose(one['ess_bulk'], D.chain_diagnostics(diag['samples'][0], chains=False)['ess_bulk'])
        big = np.random.default_rng(0).normal(size=(1, R.MAX_DRAWS + 2, 2))
        host = D.diagnose(popn, big)
        assert host['route'] == 'host' and np.array_equal(host['ess_bulk'], D.chain_diagnostics(big)['ess_bulk'])
        with pytest.raises(ValueError, match="8 kept draws"):
            sample_glms_hmc(popn, x, 4, diagnostics=True, **kw)
        text = D.worst_table(s, 2)
        print(text)
        assert text.startswith("convergence (2 chains, device)") and "parameters flagged" in text
    finally:
        popn.release_data()


def test_diag_kernel_is_built_without_scratch():
    """(No GPU needed: the code object's metadata.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_diag'))
    print(built)
    assert sorted(built) == ['k_diag_column']
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0, (n, r)
        assert r['lds'] == 3168                               # PGL_DIAG_STATIC_LDS: the launch's 64 KiB test counts it
    assert _lib.load().pgl_version() >= 112                  # (111: the version before the diagnostics entry points)
