"""Host side of the clamped simulation: the numpy statements of inference/predictive.py against the gcc mirror of
csrc/pglm_condsim.h (currents bit for bit, chains spike for spike), the currents against a longdouble reference, the
reproduction theorem, the accumulators, the helpers of the binding, synth_map's flag, the new symbols and the kernels'
resources."""
import os

import numpy as np
import pytest

from tests import condsim_reference as CR
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import predictive as P

NAMES = [c['name'] for c in CR.CASES]
U = 2.0 ** -53


@pytest.mark.parametrize('name', NAMES)
def test_currents_numpy_statement_equals_mirror_bit_for_bit(name):
    X0, AW, S_obs = CR.make_case(name)
    assert P.cond_currents_numpy(X0, AW, S_obs).tobytes() == CR.mirror(name)['Xc'].tobytes()


@pytest.mark.parametrize('name', NAMES)
def test_currents_against_longdouble(name):
    """Two bounds per element, A the sum of the absolute terms of the element (|X0| and every |AW| added), u = 2^-53:
    |Xc - reference| <= 16 u A: "a few ulps of the sum of absolute terms", a few read as at most 8 and ulp(A) <= 2 u A.  This is
        the accuracy the rule's order must keep where an element has many additions (m up to ~1600 in this table): a change
        of how the additions are ordered or carried out that loses accuracy there fails it;
    |Xc - reference| <= gamma_m A, gamma_m = m u / (1 - m u), m the number of the element's additions: the bound of a serial
        sum of m + 1 terms (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), the sharper one where m is
        small; an element without an addition is exact.
    Printed: the largest error of the case in units of u A, the largest m, the largest ratio to the second bound."""
    X0, AW, S_obs = CR.make_case(name)
    ref, A, M = CR.currents_longdouble(X0, AW, S_obs)
    err = np.abs(CR.mirror(name)['Xc'].astype(np.longdouble) - ref)
    bound = (M * U / (1.0 - M * U)) * A
    print(name, 'max |err| / (u A) = %.3f, max m = %d, max err / bound = %.3f'
          % (float(np.max(err / A) / U), M.max(), float(np.max(err[M > 0] / bound[M > 0])) if np.any(M > 0) else 0.0))
    assert np.all(err <= 16 * U * A)
    assert np.all(err <= bound)


@pytest.mark.parametrize('name', ['n1', 'n3_silent', 'nt1_win_gt_nt', 'nt_lt_r', 'r1', 'burst', 'exceptions'])
def test_chain_numpy_statement_equals_mirror(name):
    c = CR.BY_NAME[name]
    _, AW, _ = CR.make_case(name)
    m = CR.mirror(name)
    n_rep = min(c['n_rep'], 3)
    S, exc = P.simulate_cond_numpy(m['Xc'], AW, c['nlin'], CR.DT, n_rep, seed=c['seed'], rep0=c['rep0'])
    assert S.dtype == np.uint8 and np.array_equal(S, m['S'][:n_rep])
    if n_rep == c['n_rep']:
        assert np.array_equal(exc, m['exceptions'])


# ---- the reproduction theorem -------------------------------------------------------------------------------------------
#          nlin         seed  stream
THEOREM = [('explinear', 61,  0), ('explinear', 62,  7), ('exp', 63, 3)]


def _coupled(nlin, seed, N=3, R=20, nT=5000):
    rng = np.random.RandomState(3000 + seed)
    X0 = (np.log(40.0) if nlin == 'exp' else 40.0) + (0.3 if nlin == 'exp' else 10.0) * rng.randn(nT, N)
    W = rng.randn(N, N) * ((0.4 if nlin == 'exp' else 8.0) / np.sqrt(N))
    AW = W[:, None, :] * np.exp(-np.arange(R) / (0.3 * R))[None, :, None] * (1.0 + 0.2 * rng.rand(N, R, N))
    return X0, AW


@pytest.mark.parametrize('nlin,seed,r', THEOREM)
def test_clamping_a_free_run_at_its_own_spikes_reproduces_it(nlin, seed, r):
    """A free run of the coupled population at stream r is its own clamped simulation at rep0 = r: the other neurons' spikes
    are the recorded ones, the own spikes come back one by one.  Xc plus the self terms re-associates the sum the free run
    made (~1e-13 relative), so the run must keep its decisions 1e-9 clear of the thresholds: a condition on the inputs,
    asserted first."""
    X0, AW = _coupled(nlin, seed)
    S, X, exc, closest = _lib.simulate_streams(X0, AW, nlin, CR.DT, rep=r, seed=seed)
    print(nlin, seed, r, 'closest', closest, 'spikes', S.sum(axis=0))
    assert closest >= 1e-9 and exc == 0 and S.sum(axis=0).min() > 50 and X0.shape == (5000, 3)
    assert np.abs(X - X0).max() > 1.0                                  # the coupling matters
    for currents, run in ((CR.host_currents, lambda Xc: CR.host_run(Xc, AW, nlin, CR.DT, 1, seed, r)[0][0]),
                          (P.cond_currents_numpy, lambda Xc: P.simulate_cond_numpy(Xc, AW, nlin, CR.DT, 1, seed=seed, rep0=r)[0][0])):
        Xc = currents(X0, AW, S)
        assert np.array_equal(run(Xc), S)
    # (another stream does not reproduce it)
    assert not np.array_equal(CR.host_run(Xc, AW, nlin, CR.DT, 1, seed, r + 1)[0][0], S)


# ---- accumulators -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n3_silent', 'n64_win1', 'rep130', 'nt1_win_gt_nt', 'nt_lt_r'])
def test_planes_equal_a_plain_reduction_and_continue(name):
    c = CR.BY_NAME[name]
    m = CR.mirror(name)
    S, obs, win = m['S'], m['obs'], c['win']
    nT = c['nT']
    n_win = -(-nT // win)
    assert obs.shape == (n_win, c['N'])
    cnt = np.stack([[S[i, w * win:(w + 1) * win].sum(axis=0, dtype=np.int64) for w in range(n_win)] for i in range(S.shape[0])])
    want = np.stack([cnt.sum(axis=0), (cnt ** 2).sum(axis=0), (cnt < obs).sum(axis=0), (cnt == obs).sum(axis=0),
                     cnt.min(axis=0), cnt.max(axis=0)])
    assert m['acc'].dtype == np.int64 and np.array_equal(m['acc'], want)
    assert np.array_equal(P.cond_accumulate_numpy(S, obs, win), want)
    k = max(1, S.shape[0] // 3)
    for fold in (CR.host_fold, P.cond_accumulate_numpy):
        assert np.array_equal(fold(S[k:], obs, win, fold(S[:k], obs, win)), want)


def test_summary_of_the_planes():
    m = CR.mirror('rep130')
    c = CR.BY_NAME['rep130']
    res = P.cond_summary(m['acc'], m['obs'], c['n_rep'])
    cnt = np.stack([_lib.window_counts(s, c['win']) for s in m['S']]).astype(float)
    assert np.allclose(res['mean'], cnt.mean(axis=0), rtol=1e-14) and np.allclose(res['sd'], cnt.std(axis=0, ddof=1), rtol=1e-12)
    assert np.array_equal(res['min'], cnt.min(axis=0)) and np.array_equal(res['max'], cnt.max(axis=0))
    pit = ((cnt < m['obs']).sum(axis=0) + 0.5 * (cnt == m['obs']).sum(axis=0)) / c['n_rep']
    assert np.array_equal(res['pit'], pit) and np.all((0 <= pit) & (pit <= 1))
    zero = res['sd'] == 0
    assert np.all(np.isnan(res['pearson'][zero])) and np.all(np.isfinite(res['pearson'][~zero]))
    assert res['pit_ks'].shape == (c['N'],) and res['pit_ks'][0] == P.ks_uniform(pit[:, 0])
    one = P.cond_summary(CR.host_fold(m['S'][:1], m['obs'], c['win']), m['obs'], 1)
    assert np.all(np.isnan(one['sd'])) and np.all(np.isnan(one['pearson']))


def test_spike_events_and_window_counts():
    S = np.array([[0, 2, 0], [0, 0, 0], [1, 0, 3], [0, 0, 0], [0, 1, 0]])
    pre, cnt, off = _lib.spike_events(S)
    assert pre.dtype == np.int32 and cnt.dtype == np.uint8 and off.dtype == np.int64
    assert pre.tolist() == [1, 0, 2, 1] and cnt.tolist() == [2, 1, 3, 1] and off.tolist() == [0, 1, 1, 3, 3, 4]
    assert _lib.window_counts(S, 2).tolist() == [[0, 2, 0], [1, 0, 3], [0, 1, 0]]
    assert _lib.window_counts(S, 7).tolist() == [[1, 3, 3]]
    with pytest.raises(ValueError):
        _lib.spike_events(np.full((2, 2), 256))
    assert _lib.simulate_cond_workspace(128, 200, 256) == 128 * 200 * 256 * 8


def test_bad_arguments_and_no_device():
    c = CR.BY_NAME['n3_silent']
    _, AW, S_obs = CR.make_case('n3_silent')
    m = CR.mirror('n3_silent')
    run = lambda **kw: _lib.simulate_cond(m['Xc'], AW, c['nlin'], CR.DT, kw.pop('obs', m['obs']), kw.pop('win', c['win']),
                                          kw.pop('n_rep', 1), **kw)
    with pytest.raises(_lib.PglError, match='argument'):
        run(n_rep=0)
    with pytest.raises(_lib.PglError, match='argument'):
        run(rep0=-1)
    with pytest.raises(ValueError):
        run(win=0)
    with pytest.raises(_lib.PglError, match='taps'):
        _lib.simulate_cond(np.zeros((4, 1)), np.zeros((1, _lib.CS_MAX_R + 1, 1)), 1, CR.DT, np.zeros((1, 1)), 50, 1)
    with pytest.raises(_lib.PglError, match='workgroups'):             # 1024 * ceil(n_rep / 64) > 2^31 - 1: no wrapped grid
        _lib.simulate_cond_dev(1024, 4, 1, 1, CR.DT, 8, 8, 8, 50, 2 ** 27 + 1, 8, 8, 8)
    # the host reference refuses what the device entries refuse
    with pytest.raises(_lib.PglError, match='taps'):
        _lib.simulate_cond_streams(np.zeros((4, 1)), np.zeros((1, _lib.CS_MAX_R + 1, 1)), 1, CR.DT)
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_cond_streams(m['Xc'], AW, c['nlin'], 0.0)
    with pytest.raises(_lib.PglError, match='1024'):
        _lib.simulate_cond_streams(np.zeros((2, 1025)), np.zeros((1025, 1, 1025)), 1, CR.DT)
    pre, cnt, off = _lib.spike_events(S_obs)
    with pytest.raises(_lib.PglError, match='sorted'):
        _lib.cond_currents(CR.make_case('n3_silent')[0], AW, np.where(np.arange(pre.size) == 0, c['N'], pre), cnt, off)
    if _lib.device_count() == 0:                                       # no quiet fall-back to the host loop
        with pytest.raises(_lib.PglError, match='device'):
            run()
        with pytest.raises(_lib.PglError, match='device'):
            _lib.cond_currents(CR.make_case('n3_silent')[0], AW, pre, cnt, off)


def test_synth_map_flag_and_table(tmp_path, monkeypatch):
    import pickle
    from theano_pyglm_amd.harness import synth_map
    data = tmp_path / 'data.pkl'
    data.write_bytes(pickle.dumps({'N': 2}))
    seen = {}
    monkeypatch.setattr(synth_map, 'run_synth_test', lambda *a, **kw: seen.update(kw))
    synth_map.main(['-d', str(data), '-r', str(tmp_path), '--cond-ppc', '64', '25'])
    assert seen['cond_ppc'] == [64, 25] and '--cond-ppc N [WIN]' in synth_map.__doc__
    ap = synth_map.parser()
    assert ap.parse_args(['-d', 'x', '--cond-ppc', '64']).cond_ppc == [64]
    assert ap.parse_args(['-d', 'x', '--cond-ppc', '64', '25']).cond_ppc == [64, 25]
    assert ap.parse_args(['-d', 'x']).cond_ppc is None
    for bad in (['64', '25', '3'], ['0'], ['64', '-5']):
        with pytest.raises(SystemExit):
            ap.parse_args(['-d', 'x', '--cond-ppc'] + bad)
    m = CR.mirror('rep130')
    c = CR.BY_NAME['rep130']
    res = P.cond_summary(m['acc'], m['obs'], c['n_rep'])
    res.update({'t0': np.arange(m['obs'].shape[0]) * 0.02, 'win': c['win'], 'exceptions': m['exceptions']})
    lines = P.format_cond_table(res).split('\n')
    assert len(lines) == 2 + c['N'] + 1 and 'max|pearson|' in lines[1] and 'conditional' in lines[-1]


def test_new_symbols_and_kernel_resources():
    import sys
    import __graft_entry__ as ge
    ge.build_hip()
    for s in ('pgl_cond_currents_dev', 'pgl_cond_currents', 'pgl_simulate_cond_dev', 'pgl_simulate_cond',
              'pgl_simulate_cond_streams', 'pgl_simulate_cond_workspace'):
        assert s in _lib.SYMBOLS and hasattr(_lib.load(), s)
    assert _lib.ABI_VERSION >= 118
    sys.path.insert(0, os.path.join(CR.ROOT, 'tools'))
    import reachable_kernels as RK
    built = RK.built_fused()
    names = [n for n in built if n.startswith(('k_cond_currents', 'k_simulate_cond<', 'k_cond_acc_init'))]
    assert len(names) == 4, names
    for n in names:
        r = built[n]
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0, (n, r)
        if n.startswith('k_simulate_cond<'):                           # queue 8 KiB + two tiles; the self-history is dynamic
            assert r['lds'] == _lib.CS_QUEUE * 64 * 4 + 2 * 64 * 8 and r['vgpr'] <= 128, (n, r)
