"""k_cond_currents and k_simulate_cond against the gcc mirror of csrc/pglm_condsim.h over tests/condsim_cases.json: the clamped
currents bit for bit, spikes byte for byte, counts, exceptions and the six planes exact; determinism; the route the library had
(pgl_simulate_batch_dev on a diagonal-only AW); the driver's two routes; synth_map's table.

tests/test_condsim_cases.py asserts on the CPU that no chain of these cases decides closer than 1e-9 (relative) to a threshold:
the device's exp / log may differ from the host's in the last place without flipping a spike."""
import numpy as np
import pytest

from tests import condsim_reference as CR
from tests import test_simulate_host as SH
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = [c['name'] for c in CR.CASES]


def _currents(name):
    X0, AW, S_obs = CR.make_case(name)
    return _lib.cond_currents(X0, AW, *_lib.spike_events(S_obs))


def _run(name, **kw):
    c = CR.BY_NAME[name]
    _, AW, _ = CR.make_case(name)
    m = CR.mirror(name)
    kw.setdefault('n_rep', c['n_rep'])
    kw.setdefault('rep0', c['rep0'])
    return _lib.simulate_cond(kw.pop('Xc', m['Xc']), kw.pop('AW', AW), c['nlin'], CR.DT, kw.pop('obs', m['obs']), c['win'],
                              kw.pop('n_rep'), seed=c['seed'], counts=True, spikes=True, **kw)


@pytest.mark.parametrize('name', NAMES)
def test_both_kernels_equal_the_mirror(name):
    m = CR.mirror(name)
    Xc = _currents(name)
    assert Xc.tobytes() == m['Xc'].tobytes()
    for flags in (0, 1):                                               # the queue (and its fallback), every chain on the ring
        out = _run(name, Xc=Xc, flags=flags)
        assert out['S'].dtype == np.uint8 and np.array_equal(out['S'], m['S']), flags
        assert np.array_equal(out['counts'], m['counts']) and np.array_equal(out['exceptions'], m['exceptions'])
        assert out['acc'].dtype == np.int64 and np.array_equal(out['acc'], m['acc'])
        if flags == 0:
            print(name, 'fallbacks', out['fallbacks'])
            assert (out['fallbacks'] > 0) == (name == 'burst')
    if name == 'exceptions':
        assert out['exceptions'].min() >= 1 and out['S'].max() == 10


def test_two_calls_give_the_same_bits_and_a_batch_equals_its_replicates():
    name = 'rep130'
    c = CR.BY_NAME[name]
    a, b = _run(name), _run(name)
    for k in ('S', 'counts', 'exceptions', 'acc'):
        assert a[k].tobytes() == b[k].tobytes()
    assert _currents(name).tobytes() == _currents(name).tobytes()
    acc = exc = fb = None
    for i in range(c['n_rep']):                                        # all 130, one at a time, continuing one accumulator
        one = _run(name, n_rep=1, rep0=c['rep0'] + i, acc=acc, exceptions=exc, fallbacks=fb)
        assert one['S'][0].tobytes() == a['S'][i].tobytes() and np.array_equal(one['counts'][0], a['counts'][i])
        acc, exc, fb = one['acc'], one['exceptions'], one['fallbacks']
    assert np.array_equal(acc, a['acc']) and np.array_equal(exc, a['exceptions'])
    # a call over a range followed by a continuing call over the next range equals one call over both
    first = _run(name, n_rep=70)
    both = _run(name, n_rep=60, rep0=c['rep0'] + 70, acc=first['acc'], exceptions=first['exceptions'], fallbacks=first['fallbacks'])
    assert np.array_equal(both['acc'], a['acc']) and np.array_equal(both['exceptions'], a['exceptions'])


@pytest.mark.parametrize('name,n', [('n65', 64), ('n3_silent', 0), ('burst', 1)])
def test_a_neuron_alone_equals_itself_among_others(name, n):
    """A chain's bits do not depend on the chains beside it.  The stream of a chain is (seed, r, n), so neuron n alone keeps
    its stream only at its own index: column n among silent neurons against column n of the full call; and for n = 0, whose
    index an N = 1 call has, the literal N = 1 call on that column."""
    c = CR.BY_NAME[name]
    _, AW, _ = CR.make_case(name)
    m = CR.mirror(name)
    full = _run(name)
    Xc = np.full_like(m['Xc'], -40.0)
    Xc[:, n] = m['Xc'][:, n]
    alone = _run(name, Xc=Xc)
    assert alone['S'][:, :, n].tobytes() == full['S'][:, :, n].tobytes()
    assert np.array_equal(alone['acc'][:, :, n], full['acc'][:, :, n]) and alone['exceptions'][n] == full['exceptions'][n]
    others = np.arange(c['N']) != n
    assert alone['S'][:, :, others].sum() == 0
    if n == 0:                                                         # .. and literally alone: N = 1 is stream (seed, r, 0)
        one = _lib.simulate_cond(np.ascontiguousarray(m['Xc'][:, :1]), np.ascontiguousarray(AW[:1, :, :1]), c['nlin'], CR.DT,
                                 np.ascontiguousarray(m['obs'][:, :1]), c['win'], c['n_rep'], seed=c['seed'], rep0=c['rep0'],
                                 counts=True, spikes=True)
        assert one['S'][:, :, 0].tobytes() == full['S'][:, :, 0].tobytes()
        assert np.array_equal(one['acc'][:, :, 0], full['acc'][:, :, 0])


@pytest.mark.parametrize('name', ['n3_silent', 'n65', 'long_r200'])
def test_counts_equal_the_batched_simulation_on_diagonal_only_couplings(name):
    c = CR.BY_NAME[name]
    _, AW, _ = CR.make_case(name)
    m = CR.mirror(name)
    assert np.all(m['exceptions'] == 0)
    n_rep = min(c['n_rep'], 4)
    old = _lib.simulate_batch(m['Xc'], CR.diagonal_only(AW), c['nlin'], CR.DT, n_rep, seed=c['seed'], rep0=c['rep0'], spikes=False)
    new = _run(name, n_rep=n_rep)
    assert np.all(old['exceptions'] == 0) and np.array_equal(new['counts'], old['counts'])


def test_device_pointer_form_counts_only():
    import torch
    name = 'n64_win1'
    c = CR.BY_NAME[name]
    X0, AW, S_obs = CR.make_case(name)
    m = CR.mirror(name)
    nT, N, R = c['nT'], c['N'], c['R']
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    pre, cnt, off = _lib.spike_events(S_obs)
    d_X0, d_AW, d_pre, d_cnt, d_off, d_obs = t(X0), t(AW), t(pre), t(cnt), t(off), t(m['obs'])
    d_Xc = torch.empty((nT, N), dtype=torch.float64, device='cuda')
    d_acc = torch.empty((6,) + m['obs'].shape, dtype=torch.int64, device='cuda')
    d_exc = torch.empty(N, dtype=torch.int64, device='cuda')
    d_ws = torch.empty(_lib.simulate_cond_workspace(N, R, c['n_rep']) // 8, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.cond_currents_dev(N, nT, R, d_X0, d_AW, d_pre, d_cnt, d_off, d_Xc)
    _lib.simulate_cond_dev(N, nT, R, c['nlin'], CR.DT, d_Xc, d_AW, d_obs, c['win'], c['n_rep'], d_acc, d_exc, d_ws, seed=c['seed'],
                           rep0=c['rep0'])
    torch.cuda.synchronize()
    assert d_Xc.cpu().numpy().tobytes() == m['Xc'].tobytes()
    assert np.array_equal(d_acc.cpu().numpy(), m['acc']) and np.array_equal(d_exc.cpu().numpy(), m['exceptions'])
    with pytest.raises(_lib.PglError, match='argument'):               # the workspace is required
        _lib.simulate_cond_dev(N, nT, R, c['nlin'], CR.DT, d_Xc, d_AW, d_obs, c['win'], c['n_rep'], d_acc, d_exc, 0)


@pytest.fixture(scope='module')
def recorded():
    """an N = 4 population with 3 000 bins of its own simulation as the recording"""
    N, nT = 4, 3000
    popn, x = SH.population(N, 5)
    S = popn.simulate_batch(x, (0, nT * SH.DT), SH.DT, None, 0.1, 1, seed=33, rep0=1000)['S'][0]
    popn.add_data({'S': S.astype(np.float64), 'N': N, 'dt': SH.DT, 'T': nT * SH.DT, 'stim': None, 'dt_stim': 0.1})
    yield popn, x, S
    popn.release_data()


def _same(a, b):
    for k in ('obs', 'mean', 'sd', 'min', 'max', 'pit', 'pearson', 'pit_ks', 'acc', 'exceptions', 't0', 'width', 'counts'):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in a['total']:
        assert np.array_equal(a['total'][k], b['total'][k]), k
    assert a['n_rep'] == b['n_rep'] and a['n_draws'] == b['n_draws']


def test_driver_device_equals_host_route(recorded):
    from theano_pyglm_amd.inference.predictive import conditional_counts, format_cond_table
    popn, x, S = recorded
    X0, AW = popn._simulation_inputs(x, (0.0, 3.0), SH.DT, None, 0.1, nT=3000)
    AW = np.ascontiguousarray(np.transpose(AW, (0, 2, 1)))
    closest = CR.host_run(CR.host_currents(X0, AW, S), AW, popn.glm.nlin_model.kind, SH.DT, 8, 3, 2)[2]
    assert closest > 1e-9                                              # the condition of an exact comparison of the two routes
    dev = conditional_counts(popn, x, n_rep=8, win=70, seed=3, rep0=2, keep_counts=True)
    host = conditional_counts(popn, x, n_rep=8, win=70, seed=3, rep0=2, keep_counts=True, device=False)
    _same(dev, host)
    print(format_cond_table(dev))
    n_win = -(-3000 // 70)
    assert dev['obs'].shape == (n_win, 4) and np.array_equal(dev['obs'].sum(axis=0), S.sum(axis=0))
    assert dev['counts'].shape == (8, 4) and np.array_equal(dev['acc'][0].sum(axis=0), dev['counts'].sum(axis=0))
    assert dev['width'][-1] == pytest.approx((3000 - (n_win - 1) * 70) * SH.DT) and dev['fallbacks'] == 0
    assert np.all((dev['pit'] >= 0) & (dev['pit'] <= 1)) and dev['n_rep'] == 8
    popn.set_time_shard(0, 2)
    try:
        with pytest.raises(ValueError, match='time-sharded'):
            conditional_counts(popn, x, n_rep=2)
    finally:
        popn.set_time_shard(None)


def test_driver_with_samples(recorded):
    from theano_pyglm_amd.inference.predictive import conditional_counts
    popn, x, _ = recorded
    theta = np.asarray(popn.theta_matrix(x), dtype=np.float64)
    rng = np.random.RandomState(9)
    samples = theta[None] + 0.02 * rng.standard_normal((5,) + theta.shape)
    dev = conditional_counts(popn, x, n_rep=4, win=100, samples=samples, n_draws=3, seed=3, keep_counts=True)
    host = conditional_counts(popn, x, n_rep=4, win=100, samples={'samples': samples}, n_draws=3, seed=3, keep_counts=True,
                              device=False)
    _same(dev, host)
    assert dev['n_draws'] == 3 and dev['n_rep'] == 12 and dev['counts'].shape == (12, 4)
    assert np.array_equal(dev['acc'][2] + dev['acc'][3] <= 12, np.ones_like(dev['acc'][2], dtype=bool))


def test_synth_map_prints_the_table(recorded, capsys):
    from theano_pyglm_amd.harness import synth_map
    popn, x, _ = recorded
    print(synth_map.cond_ppc_table(popn, x, [16]))                     # --cond-ppc 16: WIN defaults to 50
    out = capsys.readouterr().out
    assert 'clamped predictive residuals (16 replicates, 60 windows of 50 bins)' in out and 'pit KS' in out
    assert len(out.strip().split('\n')) == 2 + 4 + 1
