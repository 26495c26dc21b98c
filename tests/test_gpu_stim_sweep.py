"""The stimulus-preparation kernels (pglm_stim.hip.h) over the case tables of tests/stim_reference.py, each against its
longdouble reference at the bound derived there (tests/test_stim_cases.py proves on the CPU that the cases reach what they
name and that the bounds reject emulated defects): the five thin GEMMs one launch at a time through pgl_gemm_dev, the feature
build through pgl_set_stimulus, both forms of pgl_sta, and pgl_leading_singular_pairs.  Every run prints its worst ratio to
the bound, checks what must stay untouched and that a second run (and a batch element alone) gives equal bits."""
import numpy as np
import pytest

from tests import helpers as H
from tests import stim_reference as R
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu
OPT_SEPF = 94                     # dev option: 7 = pgl_sta in its bin-rate form


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)      # (the GEMMs and the singular pairs need the stream only)
    yield h
    h.close()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- the thin GEMMs --------------------------------------------------------------------------------------------------
def _gemm(handle, d, element=None):
    """run the case (element: that batch element alone, as a batch of one) -> (flat C, A and B images after the run)"""
    import torch
    A, B = _t(d['Abuf']), _t(d['Bbuf'])
    C = torch.full((d['c_size'],), R.SENTINEL, dtype=torch.float64, device='cuda')
    e = 0 if element is None else element
    torch.cuda.synchronize()                                        # (the handle launches on a stream of its own)
    handle.gemm_dev(R.KERNELS.index(d['kernel']), A.data_ptr() + 8 * (d['a_off'] + e * d['sa'][2]), d['sa'],
                    B.data_ptr() + 8 * (d['b_off'] + e * d['sb'][2]), d['sb'],
                    C.data_ptr() + 8 * (d['c_off'] + e * d['sc'][2]), d['sc'], d['M'], d['N'], d['K'],
                    d['batch'] if element is None else 1)
    handle.sync()
    return C.cpu().numpy(), A.cpu().numpy(), B.cpu().numpy()


@pytest.mark.parametrize('c', R.GEMM_CASES, ids=[c['name'] for c in R.GEMM_CASES])
def test_gemm_case(handle, c):
    d = R.gemm_case(c)
    Cb, Ab, Bb = _gemm(handle, d)
    C, untouched = R.gemm_result(d, Cb)
    r = R.gemm_ratio(d, C)
    print(c['name'], "ratio to the bound %.3f" % r)
    assert untouched, "written outside the M x N result"
    assert _same(Ab, d['Abuf']) and _same(Bb, d['Bbuf'])           # operands and their NaN gaps as they were
    assert r <= 1.0, r
    assert _same(_gemm(handle, d)[0], Cb)                           # a second run: equal bits
    if d['batch'] > 1:
        for e in range(d['batch']):                                 # each element alone: the bits it has in the batch
            Ce, _, _ = _gemm(handle, d, element=e)
            Cel, clean = R.gemm_result(d, Ce)
            assert _same(Cel[e], C[e])
            other = np.delete(Cel, e, axis=0)
            assert clean and np.all(other == R.SENTINEL)


def _refusal(handle, d, **kw):
    import torch
    A, B = _t(d['Abuf']), _t(d['Bbuf'])
    C = torch.full((d['c_size'],), R.SENTINEL, dtype=torch.float64, device='cuda')
    a = dict(kernel=R.KERNELS.index(d['kernel']), a_off=d['a_off'], b_off=d['b_off'], sa=d['sa'], sb=d['sb'], sc=d['sc'],
             M=d['M'], N=d['N'], K=d['K'], batch=1)
    a.update(kw)
    torch.cuda.synchronize()
    with pytest.raises(_lib.PglError, match='error -1: pgl_gemm_dev'):           # PGL_ERR_ARG
        handle.gemm_dev(a['kernel'], A.data_ptr() + 8 * a['a_off'], a['sa'], B.data_ptr() + 8 * a['b_off'], a['sb'],
                        C.data_ptr() + 8 * d['c_off'], a['sc'], a['M'], a['N'], a['K'], a['batch'])
    handle.sync()
    assert np.all(C.cpu().numpy() == R.SENTINEL), kw


def test_gemm_refuses_what_a_kernel_cannot_take(handle):
    def case(kernel):
        mn = 65 if kernel == 'nt' else 17
        return R.gemm_case([c for c in R.GEMM_CASES if c['kernel'] == kernel and c['M'] == mn and c['N'] == mn and c['K'] in (66, 33)][0])
    for kernel in ('kc418', 'kc1016'):
        d = case(kernel)
        sam, sak, sAb = d['sa']
        sbn, sbk, sBb = d['sb']
        _refusal(handle, d, K=d['K'] - 1)                           # K odd
        _refusal(handle, d, a_off=d['a_off'] + 1)                   # A not 16-byte aligned
        _refusal(handle, d, sa=(sam + 1, sak, sAb))                 # lda odd
        _refusal(handle, d, sa=(sam, 2, sAb))                       # A not k-contiguous
        _refusal(handle, d, batch=2)
        if kernel == 'kc418':
            _refusal(handle, d, b_off=d['b_off'] + 1)
            _refusal(handle, d, sb=(sbn + 1, sbk, sBb))
            _refusal(handle, d, sb=(sbn, 2, sBb))
        else:
            _refusal(handle, d, sb=(2, sbk, sBb))                   # B not n-contiguous
    d = case('nt')
    _refusal(handle, d, sa=(d['sa'][0], 2, d['sa'][2]))
    _refusal(handle, d, sb=(d['sb'][0], 2, d['sb'][2]))
    _refusal(handle, d, sc=(d['sc'][0], 2, d['sc'][2]))
    _refusal(handle, d, batch=2)
    _refusal(handle, d, kernel=5)
    _refusal(handle, d, M=0)
    _refusal(handle, d, K=0)


# ---- the feature build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.FEATURE_CASES, ids=[c['name'] for c in R.FEATURE_CASES])
def test_feature_case(c):
    d = R.feature_case(c)
    dev = _lib.DeviceGlm(1, c['nT'], 1, 1, 'exp', R.DT, 0)
    try:
        dev.set_stimulus(d['stim'], c['dt_stim'], d['basis_t'], d['basis_x'], c['layout'])
        F = dev.get_stim_features()
        dev.set_stimulus(d['stim'], c['dt_stim'], d['basis_t'], d['basis_x'], c['layout'])
        F2 = dev.get_stim_features()
    finally:
        dev.close()
    assert F.shape == d['ref'].shape
    r = R.feature_ratio(d, F)
    print(c['name'], "ratio to the bound %.3f" % r)
    assert r <= 1.0, r
    assert _same(F, F2)


# ---- the spike-triggered average -------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.STA_CASES, ids=[c['name'] for c in R.STA_CASES])
def test_sta_case(c):
    d = R.sta_case(c)
    forms = (0, 7) if R.sta_facts(c)['frame_rate'] else (0,)       # 0: what the library picks; 7: the bin-rate form
    dev = _lib.DeviceGlm(len(R.STA_EVENTS), c['nT'], 1, 1, 'exp', R.DT, 0)
    try:
        dev.set_spikes(d['S'])
        for form in forms:
            dev.set_option(OPT_SEPF, form)
            A = dev.sta(d['stim'], d['dt_stim'], c['L'], Ns=np.array(c['sel']))
            r = R.sta_ratio(d, A)                                   # each form against the reference, never against the other
            print(c['name'], "form %d" % form, "ratio to the bound %.3f" % r)
            assert r <= 1.0, (form, r)
            assert _same(dev.sta(d['stim'], d['dt_stim'], c['L'], Ns=np.array(c['sel'])), A)
            rows = dict()
            for i, n in enumerate(c['sel']):                        # a repeated neuron: the same row; each neuron alone: its row
                assert _same(rows.setdefault(n, A[i]), A[i])
            if form == 0 and R.sta_facts(c)['frame_rate']:          # (the bin-rate form splits a neuron's events by the selection's size)
                n = c['sel'][-1]
                assert _same(dev.sta(d['stim'], d['dt_stim'], c['L'], Ns=np.array([n]))[0], rows[n])
    finally:
        dev.close()


# ---- leading singular pairs ------------------------------------------------------------------------------------------
def _lsp_check(c, A, b, u, s, v):
    ref, bv, bs = R.lsp_bounds(c, A[b])
    ev, es = R.lsp_errors(u, s, v, ref)
    return ev / bv, es / bs


@pytest.mark.parametrize('c', R.LSP_CASES, ids=[c['name'] for c in R.LSP_CASES])
def test_lsp_case(handle, c):
    assert c['ratio'] <= 0.98
    A, _ = R.lsp_matrices(c)
    U, S, V = handle.leading_singular_pairs(A)
    worst = (0.0, 0.0)
    for b in range(c['n']):
        rv, rs = _lsp_check(c, A, b, U[b], S[b], V[b])
        worst = (max(worst[0], rv), max(worst[1], rs))
    print(c['name'], "ratio to the bound: vectors %.3f sigma %.3f" % worst)
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    U2, S2, V2 = handle.leading_singular_pairs(A)
    assert _same(U, U2) and _same(S, S2) and _same(V, V2)
    if c['n'] > 1:
        for b in range(c['n']):                                     # each matrix alone: the bits it has in the batch
            u, s, v = handle.leading_singular_pairs(A[b:b + 1])
            assert _same(u[0], U[b]) and _same(s[0], S[b]) and _same(v[0], V[b])


@pytest.mark.parametrize('shape', [(17, 33), (65, 16), (64, 300)])
def test_lsp_zero_and_nan_matrices_touch_no_other(handle, shape):
    L, D = shape
    c = dict(L=L, D=D, ratio=0.9, n=5, seed=77)
    A, _ = R.lsp_matrices(c)
    U0, S0, V0 = handle.leading_singular_pairs(A)
    B = A.copy()
    B[1] = 0.0
    B[3, L // 2, D // 3] = np.nan
    U, S, V = handle.leading_singular_pairs(B)
    for b in (0, 2, 4):
        assert _same(U[b], U0[b]) and _same(S[b], S0[b]) and _same(V[b], V0[b])
    assert S[1] == 0.0 and np.all(U[1] == 0.0) and np.all(V[1] == 0.0)          # the zero matrix: include/pyglm_hip.h
    assert np.isnan(S[3]) and np.all(np.isnan(U[3])) and np.all(np.isnan(V[3]))
