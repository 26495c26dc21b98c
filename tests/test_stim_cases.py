"""The tables of tests/stim_reference.py do what they claim (no GPU): every case reaches the branch it is named for, the
longdouble references agree with the float64 oracle, the float64 numpy result of every case lies inside its bound, and
the bounds reject emulated defects of a numpy mirror of each kernel's blocking."""
import numpy as np
import pytest

from oracle import glm_oracle as O
from tests import stim_reference as R


def _by(kernel, **kw):
    return [c for c in R.GEMM_CASES if c['kernel'] == kernel and all(c[k] == v for k, v in kw.items())]


# ---- GEMM ------------------------------------------------------------------------------------------------------------
def test_gemm_table_covers_the_shapes_and_branches():
    for kernel, Ns, Ks in (('mfma1', (1, 15, 16, 17), R.K_MFMA), ('mfma4', (1, 48, 63, 64, 65, 80), R.K_MFMA4),
                           ('kc1016', (1, 15, 16, 17), R.K_KC), ('kc418', (1, 15, 16, 17, 63, 64, 65), R.K_KC)):
        got = set((c['M'], c['N'], c['K']) for c in _by(kernel))
        for M in R.M_TAILS:
            for N in Ns:
                for K in Ks:
                    if kernel.startswith('kc') and K in (576, 1088):
                        continue
                    assert (M, N, K) in got, (kernel, M, N, K)
        assert set(Ks) <= set(k for _, _, k in got)
    assert set((c['M'], c['N'], c['K']) for c in _by('nt')) == set((m, n, k) for m in (1, 63, 64, 65) for n in (1, 63, 64, 65)
                                                                    for k in (1, 31, 32, 33, 65))
    f = dict((K, R.gemm_facts(dict(kernel='mfma1', K=K))) for K in R.K_MFMA)
    assert [f[K]['nU'] for K in R.K_MFMA] == [1, 1, 1, 1, 1, 2, 7, 8, 9, 18]
    assert f[224]['idle'] == 1 and f[256]['idle'] == 0 and not f[256]['prefetch'] and not f[256]['ktail']
    assert f[257]['prefetch'] and f[257]['rounds'] == 2 and f[545]['rounds'] == 3 and f[545]['ktail']
    assert f[1]['idle'] == 7 and f[33]['idle'] == 6
    for kernel, NB in (('kc418', 8), ('kc1016', 16)):
        f = dict((K, R.gemm_facts(dict(kernel=kernel, K=K))) for K in R.K_KC)
        assert set(f[K]['ktail'] for K in R.K_KC) == {0, 2, 4, 6}
        assert f[2]['nC'] == 1 and f[2]['idle'] == 7 and f[8]['nC'] == 1 and f[8]['ktail'] == 0
        assert f[72]['nC'] == 9 and f[72]['cpw'] == 2 and f[72]['idle'] == 3 and f[72]['short']     # waves 5 - 7 idle, wave 4 short
        assert f[64]['nC'] == 8 and f[64]['cpw'] == 1 and f[64]['idle'] == 0 and f[66]['nC'] == 9
        assert f[576]['cpw'] == 9 and f[1088]['cpw'] == 17
        assert f[1088]['batches'] == (3 if NB == 8 else 2) and f[1088]['partial_batch']             # one chunk past NB
        assert f[576]['batches'] == (2 if NB == 8 else 1) and f[576]['partial_batch']
        assert f[64]['cpw'] < NB
    for kernel in ('mfma1', 'mfma4'):                               # the four stride patterns, batches of 1 and 3
        for pat in ('rm', 'tr', 'bvec', 'trbvec', 'ct'):
            assert set(c['batch'] for c in _by(kernel, pat=pat)) >= {1, 3}, (kernel, pat)
    for c in R.GEMM_CASES:
        d = R.gemm_case(c)
        if c['kernel'].startswith('kc'):                            # preconditions of the kc kernels hold by construction
            assert c['K'] % 2 == 0 and d['sa'][0] % 2 == 0 and d['a_off'] % 2 == 0 and d['sa'][1] == 1 and c['batch'] == 1
            assert d['sa'][0] >= c['K']
            if c['kernel'] == 'kc418':
                assert d['sb'][0] % 2 == 0 and d['sb'][1] == 1 and d['b_off'] % 2 == 0
            else:
                assert d['sb'][0] == 1
        if c['kernel'] == 'nt':
            assert d['sa'][1] == d['sb'][1] == d['sc'][1] == 1 and d['sa'][0] > c['K'] and d['sc'][0] > c['N']
    assert any(R.gemm_case(c)['sa'][0] > c['K'] for c in _by('kc418')) and any(R.gemm_case(c)['sb'][1] > c['N'] for c in _by('kc1016'))


def test_gemm_inputs_span_six_orders_with_a_scale_per_chunk():
    d = R.gemm_case(_by('kc418', M=17, N=65, K=1088)[0])
    a = np.abs(d['A'][0, 0])
    assert a.max() / a.min() > 1e5
    sc = np.array([np.exp(np.mean(np.log(a[8 * j:8 * j + 8]))) for j in range(136)])
    ratio = np.sort(sc)[1:] / np.sort(sc)[:-1]
    assert np.all(np.sort(sc)[1:] > np.sort(sc)[:-1]) and np.median(ratio) > 1.05
    assert (d['A'] < 0).any() and (d['A'] > 0).any() and (d['B'] < 0).any()
    assert np.isnan(d['Abuf']).any() and np.isnan(d['Bbuf']).any()


@pytest.mark.parametrize('kernel', R.KERNELS)
def test_gemm_numpy_inside_the_bound_and_defects_outside(kernel):
    worst, rejected = 0.0, dict((f, 0) for f in R.FAULTS)
    applicable = dict((f, 0) for f in R.FAULTS)
    for c in _by(kernel):
        d = R.gemm_case(c)
        C, clean = R.gemm_result(d, R.gemm_mirror(d))
        assert clean, c['name']
        r = R.gemm_ratio(d, C)
        assert r <= 1.0, (c['name'], r)
        worst = max(worst, r)
        plain = np.einsum('bmk,bnk->bmn', d['A'], d['B'])           # float64, numpy's own order
        assert R.gemm_ratio(d, plain) <= 1.0, c['name']
        f = R.gemm_facts(c)
        tile_m = 64 if kernel == 'nt' else 16
        for fault in R.FAULTS:
            if fault == 'ktail' and not f['ktail']:
                continue
            if fault == 'clamp_write' and (c['M'] % tile_m == 0 or c['M'] == 1):
                continue
            applicable[fault] += 1
            Cf, cleanf = R.gemm_result(d, R.gemm_mirror(d, fault))
            try:
                bad = (not cleanf) or R.gemm_ratio(d, Cf) > 1.0
            except AssertionError:                                   # (the zero row no longer zero)
                bad = True
            assert bad, (c['name'], fault)
            rejected[fault] += 1
    print(kernel, "worst mirror ratio %.3f" % worst, rejected)
    assert all(applicable[f] > 0 for f in R.FAULTS) and rejected == applicable


# ---- features --------------------------------------------------------------------------------------------------------
def test_feature_table_covers_the_shapes():
    C = R.FEATURE_CASES
    assert set(c['nT'] for c in C) >= {1, 255, 256, 257, 513} and set(c['Rt'] for c in C) >= {1, 2, 255, 256, 257, 300}
    assert set((c['Bt'], c['Bx'], c['ident'], c['layout']) for c in C) >= set(
        (bt, bx, i, l) for bt in (1, 3, 4) for bx in (1, 3) for i in (True, False) for l in (0, 1))
    assert set(c['Tstim'] for c in C) >= {1, 2} and any(c['Rt'] > c['nT'] for c in C)
    assert any((c['Tstim'] - 1) * c['dt_stim'] < (c['nT'] - 1) * R.DT * 0.5 and c['Tstim'] > 2 for c in C)     # a short stimulus
    ratios = set(round(c['dt_stim'] / R.DT, 6) for c in C)
    assert ratios >= {1.0, 7.0, 100.0, 3.3}
    for c in C:
        assert c['ident'] == (c['Bx'] == c['D'] and R.feature_case(c)['basis_x'] is None) or not c['ident']
        assert (c['Rt'] + 256 + c['Rt'] * c['Bt']) * 8 <= 64 * 1024


@pytest.mark.parametrize('c', R.FEATURE_CASES, ids=[c['name'] for c in R.FEATURE_CASES])
def test_feature_reference_oracle_and_defect(c):
    d = R.feature_case(c)
    bx = np.eye(c['D']) if d['basis_x'] is None else d['basis_x']
    if c['layout'] == 0:
        orc = O.spatiotemporal_stim_features(d['stim'], c['dt_stim'], R.DT, c['nT'], bx, d['basis_t'])
    else:
        s = O.interp_stim(d['stim'], c['dt_stim'], R.DT, c['nT'])
        orc = O.convolve_with_basis(s.dot(bx), d['basis_t']).reshape(c['nT'], -1)
    assert orc.shape == d['ref'].shape
    assert R.feature_ratio(d, orc) <= 1.0, R.feature_ratio(d, orc)       # the oracle at its own (float64) accuracy
    r = R.feature_ratio(d, R.feature_numpy(d))
    assert r <= 1.0, r
    if c['nT'] > 1:
        assert R.feature_ratio(d, R.feature_numpy(d, shift=1)) > 1.0     # a window one bin off


# ---- STA -------------------------------------------------------------------------------------------------------------
def test_sta_table_covers_the_shapes():
    C = R.STA_CASES
    assert set(c['L'] * c['D'] for c in C) >= {1, 255, 256, 257, 600}
    assert set(c['Tstim'] for c in C) == {2, 3, 24, 25} and set(c['q'] for c in C) == {1, 7, 100}
    assert set(R.STA_EVENTS) == {0, 1, 255, 256, 257, 700}
    assert list(R.STA_SEL) != sorted(R.STA_SEL) and len(set(R.STA_SEL)) < len(R.STA_SEL)
    forms = set()
    for c in C:
        f, d = R.sta_facts(c), R.sta_case(c)
        forms.add(f['frame_rate'])
        assert f['frame_rate'] == (c['Tstim'] in (2, 24))
        assert c['nT'] <= 3000 and d['S'].max() > 1
        ev = np.count_nonzero(d['S'], axis=0)
        assert tuple(ev) == R.STA_EVENTS
        for n in range(2, 6):                                        # events at t < L, on the last bin, behind the last frame
            t = np.nonzero(d['S'][:, n])[0]
            assert t[0] == 0 and t[-1] == c['nT'] - 1 and np.any(t > (c['Tstim'] - 1) * c['q'])
    assert forms == {True, False}
    f = R.sta_facts([c for c in C if c['sel'] == (1,)][0])
    assert f['echunks'] == 64 and f['empty'] == [63]
    f = R.sta_facts([c for c in C if c['sel'] == (4, 0, 5)][0])
    assert f['echunks'] == 64 and f['per'] == [5, 0, 11] and f['empty'] == [12, 64, 0]


@pytest.mark.parametrize('c', R.STA_CASES, ids=[c['name'] for c in R.STA_CASES])
def test_sta_reference_oracle_and_defects(c):
    d = R.sta_case(c)
    with np.errstate(invalid='ignore', divide='ignore'):
        orc = O.sta(d['stim'], d['S'].astype(float), R.DT, d['dt_stim'], c['L'], list(c['sel']))
    assert R.sta_ratio(d, orc) <= 1.0, R.sta_ratio(d, orc)
    assert R.sta_ratio(d, R.sta_numpy(d)) <= 1.0
    if c['L'] > 1 and any(R.STA_EVENTS[n] > 1 for n in c['sel']):
        assert R.sta_ratio(d, R.sta_numpy(d, 'neg_tt')) > 1.0
    if any(R.STA_EVENTS[n] > 0 for n in c['sel']):
        assert R.sta_ratio(d, R.sta_numpy(d, 'no_hold')) > 1.0


# ---- singular pairs --------------------------------------------------------------------------------------------------
def test_lsp_table_and_reference():
    C = R.LSP_CASES
    shapes = set((min(c['L'], c['D']), max(c['L'], c['D'])) for c in C)
    assert shapes == set((s, l) for s in R.LSP_SMALL for l in R.LSP_LARGE if s <= l)
    for s, l in shapes:
        if s != l:
            assert set(c['L'] <= c['D'] for c in C if (min(c['L'], c['D']), max(c['L'], c['D'])) == (s, l)) == {True, False}
    assert set(c['ratio'] for c in C) == {0.0, 0.1, 0.9, 0.98} and set(c['n'] for c in C) == {1, 5}
    for c in C:
        assert c['ratio'] <= 0.98
        A, s1 = R.lsp_matrices(c)
        for b in range(c['n']):
            ref, bv, bs = R.lsp_bounds(c, A[b])
            sv = np.linalg.svd(A[b], compute_uv=False)
            assert abs(float(ref[1]) - s1[b]) <= 1e-13 * s1[b] and abs(sv[0] - s1[b]) <= 1e-13 * s1[b]
            if len(sv) > 1:
                assert abs(sv[1] / sv[0] - c['ratio']) < 1e-12
            U, s, Vt = np.linalg.svd(A[b], full_matrices=False)
            ev, es = R.lsp_errors(U[:, 0], s[0], Vt[0], ref)          # LAPACK itself passes; a pair one power step short does not
            assert ev <= bv and es <= bs
            if c['ratio'] >= 0.9 and min(c['L'], c['D']) > 2:
                u = (U[:, 0] + 1e-9 * U[:, 1]) / np.sqrt(1 + 1e-18)
                assert R.lsp_errors(u, s[0], Vt[0], ref)[0] > bv
