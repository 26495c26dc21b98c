"""k_psis_column (pgl_psis_loo_dev) over the case table of tests/psis_reference.py -- every S at which the tail length, the
padding of a wave or the kernel's loops change, C = 1, 3, 65, the contents that reach each branch of the rule -- against the
longdouble reference at the bound 100 max(e0, 1e-13) recorded there (tests/test_psis_host.py proves on the CPU that the
cases reach what they name and that the bound rejects three defects).  Strided input, the weights on and off, non-finite
columns, bit reproducibility, the draw cap, and one run through loo_glms and the harness table."""
import os
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import psis_reference as R
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = R.ROOT


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)      # (the handle supplies the stream only)
    yield h
    h.close()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _run(handle, ll, weights=True):
    d = _t(ll)
    r = handle.psis_loo(d, weights=weights)
    handle.sync()
    return (r[0].cpu().numpy(), r[1].cpu().numpy()) if weights else (r.cpu().numpy(), None)


@pytest.mark.parametrize('c', R.CASES, ids=[c['name'] for c in R.CASES])
def test_psis_case(handle, c):
    ll, ref_out, ref_lw = R.case_reference(c)
    out, lw = _run(handle, ll)
    e = R.errors(out, lw, ref_out, ref_lw)
    print(c['name'], e, "ratio to the bound", dict((q, e[q] / R.BOUND[q]) for q in R.QUANTITIES))
    assert R.within(e), e
    out2, lw2 = _run(handle, ll)                                   # two calls: equal bits
    assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(lw, lw2, equal_nan=True)
    off, _ = _run(handle, ll, weights=False)                       # the weights off: the same four planes
    assert np.array_equal(out, off, equal_nan=True)
    host = handle.psis_loo_host(ll, weights=True)                  # the host-pointer form is the same call
    assert np.array_equal(host[0], out, equal_nan=True) and np.array_equal(host[1], lw, equal_nan=True)


def test_strided_slice_leaves_the_gaps_alone(handle):
    import torch
    c = [c for c in R.CASES if c['name'] == 'S65'][0]
    ll, _, _ = R.case_reference(c)
    S, C, ld = ll.shape[0], ll.shape[1], ll.shape[1] + 4
    want, want_lw = _run(handle, ll)
    full = torch.full((S, ld), -1.0e300, dtype=torch.float64, device='cuda')
    full[:, 2:2 + C] = _t(ll)
    lw_full = torch.full((S, ld), 777.0, dtype=torch.float64, device='cuda')
    before = full.cpu().numpy().copy()
    out = handle.psis_loo(full[:, 2:2 + C], weights=lw_full[:, 2:2 + C])[0]
    handle.sync()
    assert np.array_equal(out.cpu().numpy(), want)
    got = lw_full.cpu().numpy()
    assert np.array_equal(got[:, 2:2 + C], want_lw) and np.all(got[:, :2] == 777.0) and np.all(got[:, 2 + C:] == 777.0)
    assert np.array_equal(full.cpu().numpy(), before)
    r3 = handle.psis_loo(_t(np.stack([ll, ll], axis=1)))           # trailing axes are flattened: (S, 2, C) -> (4, 2, C)
    handle.sync()
    assert tuple(r3.shape) == (4, 2, C) and np.array_equal(r3.cpu().numpy()[:, 1], want)
    with pytest.raises(ValueError):
        handle.psis_loo(full[:, ::2])
    with pytest.raises(ValueError):
        handle.psis_loo(full.cpu())


def test_non_finite_column_touches_no_other(handle):
    c = [c for c in R.CASES if c['name'] == 'S64'][0]
    ll, _, _ = R.case_reference(c)
    clean, clean_lw = _run(handle, ll)
    for bad in (np.nan, np.inf, -np.inf):
        a = ll.copy()
        a[17, 1] = bad
        out, lw = _run(handle, a)
        assert np.all(np.isnan(out[:, 1])) and np.all(np.isnan(lw[:, 1]))
        assert np.array_equal(out[:, [0, 2]], clean[:, [0, 2]]) and np.array_equal(lw[:, [0, 2]], clean_lw[:, [0, 2]])


def test_a_column_alone_equals_itself_among_65(handle):
    c = [c for c in R.CASES if c['name'] == 'C65'][0]
    ll, _, _ = R.case_reference(c)
    out, lw = _run(handle, ll)
    for j in (0, 31, 64):
        o1, w1 = _run(handle, ll[:, j:j + 1])
        assert np.array_equal(o1[:, 0], out[:, j]) and np.array_equal(w1[:, 0], lw[:, j])


def test_draw_cap_and_arguments(handle):
    import torch
    assert _lib.PSIS_MAX_DRAWS == R.MAX_DRAWS
    buf = torch.zeros((R.MAX_DRAWS + 1, 2), dtype=torch.float64, device='cuda')
    p = buf.data_ptr()
    lib = handle.lib
    assert lib.pgl_psis_loo_dev(handle.h, p, R.MAX_DRAWS + 1, 2, 2, p, None) == -4          # PGL_ERR_UNSUPPORTED
    with pytest.raises(_lib.PglError, match="PGL_PSIS_MAX_DRAWS"):
        handle.psis_loo(buf)
    with pytest.raises(_lib.PglError, match="PGL_PSIS_MAX_DRAWS"):
        handle.psis_loo_host(np.zeros((R.MAX_DRAWS + 1, 1)))
    for args in ((p, 1, 2, 2, p, None), (p, 8, 0, 2, p, None), (p, 8, 2, 1, p, None), (None, 8, 2, 2, p, None), (p, 8, 2, 2, None, None)):
        assert lib.pgl_psis_loo_dev(handle.h, *args) == -1                                    # PGL_ERR_ARG
    assert lib.pgl_psis_loo_dev(None, p, 8, 2, 2, p, None) == -1
    assert lib.pgl_psis_loo(handle.h, None, 8, 2, p, None) == -1
    handle.sync()
    assert float(buf.abs().sum()) == 0.0


def test_loo_glms_end_to_end():
    """4 neurons, 3000 + 2200 bins in two data sequences, 40 draws jittered around a fit: loo_glms (the matrix on the device) =
    the numpy statement on the matrix pointwise_ll_draws returns, at the bound; a neuron subset = the matching columns bit for
    bit; the harness table is the LOO table."""
    from tests.test_gpu_hvp import _std_population
    from theano_pyglm_amd.harness import synth_map
    from theano_pyglm_amd.inference import model_compare as MC
    popn = _std_population(4, 3.0, 31, nlin='exp', bias_mu=3.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        S2 = np.minimum(np.random.default_rng(8).poisson(0.02, size=(2200, 4)), 10).astype(np.uint8)
        popn.add_data({'S': S2, 'N': 4, 'dt': 0.001, 'T': 2.2, 'stim': None, 'dt_stim': 0.1})
        P = popn.glm.P
        rng = np.random.RandomState(3)
        smp = popn.theta_matrix(x)[None] + 0.02 * rng.standard_normal((40, 4, P))
        for bc in (1, 2):
            res = MC.loo_glms(popn, x, smp, block_chunks=bc)
            r = MC.pointwise_ll_draws(popn, x, smp, block_chunks=bc, pointwise=True)
            assert set(r) == {'acc', 'n_draws', 'block_chunks', 'blocks_per_sequence', 'll'}
            ref = MC.loo_from_columns(MC.psis_loo_from_pointwise(r['ll']), MC.log_mean_exp(r['ll']), 40)
            assert res['route'] == 'device' and res['n_blocks'] == r['ll'].shape[1] == sum(r['blocks_per_sequence'])
            assert np.all(np.abs(res['elpd_b'] - ref['elpd_b']) <= R.BOUND['elpd'] * np.maximum(1.0, np.abs(ref['elpd_b'])))
            assert np.all(np.abs(res['khat_b'] - ref['khat_b']) <= R.BOUND['khat'])
            assert np.all(np.abs(res['n_eff_b'] - ref['n_eff_b']) <= R.BOUND['n_eff'] * ref['n_eff_b'])
            assert np.all(np.abs(res['p_loo'] - ref['p_loo']) <= 1e-9 * np.maximum(1.0, np.abs(ref['p_loo'])))
            assert np.array_equal(res['n_khat_bad'], ref['n_khat_bad'])
            sub = MC.loo_glms(popn, x, smp[:, 1:3], block_chunks=bc, n_lo=1)
            for k in ('elpd_b', 'khat_b', 'n_eff_b', 'elpd_loo', 'se'):
                assert np.array_equal(sub[k], res[k][..., 1:3]), k
            assert sub['n_lo'] == 1 and res['block_bins'] == 256 * bc
        text = synth_map.loo_table(popn, x, smp, block_chunks=2)
        print(text)
        assert text.startswith("PSIS-LOO (40 draws, %d blocks of 512 bins, device)" % res['n_blocks']) and 'max khat' in text
        wa = MC.waic_glms(popn, x, smp, block_chunks=2)
        d = MC.elpd_diff(res, res)
        assert np.all(d['elpd_diff'] == 0) and wa['elpd_b'].shape == res['elpd_b'].shape
    finally:
        popn.release_data()


def test_psis_kernel_is_built_without_scratch():
    """(No GPU needed: the code object's metadata.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_psis'))
    print(built)
    assert sorted(built) == ['k_psis_column']
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0, (n, r)
    assert _lib.load().pgl_version() >= 110                  # (109: the version before the PSIS entry points)
