"""pgl_simulate_batch on the device against the host reference pgl_simulate_streams with the same (seed, replicate): spikes
byte for byte, counts and exceptions exact, total currents at rtol 1e-12 of each replicate's largest |X|.

The cases and their seeds come from tests/test_simulate_host.py, which asserts on the CPU that no spike decision of these
seeds is closer than 1e-9 (relative) to its threshold: the device's exp / log may differ from the host's in the last place
without flipping a spike."""
import numpy as np
import pytest

from tests import test_simulate_host as SH
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

DT = SH.DT
#         case, n_rep, flags (bit 0: the ring in global memory)
RUNS = [(name, n_rep, flags) for name in ('small_exp', 'small_expl') for n_rep in (1, 5) for flags in (0, 1)] + \
       [('n70', 2, 0), ('n130', 2, 0), ('high_rate', 2, 0), ('high_rate', 2, 1), ('tail', 1, 0), ('tail', 1, 1)] + \
       [(name, SH.CASES[name][5], flags) for name in sorted(SH.PLAN) for flags in sorted(SH.PLAN[name])]


def _run(name, n_rep, flags=0, rep0=0, **kw):
    X0, AW, nlin, seed = SH.case(name)
    return _lib.simulate_batch(X0, AW, nlin, SH.case_dt(name), n_rep, seed=seed, rep0=rep0, flags=flags, currents=True, **kw)


def _check(out, name, i, rep):
    S, X, exc, _ = SH.host_reference(name, rep)
    assert out['S'].dtype == np.uint8 and np.array_equal(out['S'][i], S)
    assert np.array_equal(out['counts'][i], S.sum(axis=0, dtype=np.int64))
    assert out['exceptions'][i] == exc
    err = np.max(np.abs(out['X'][i] - X)) / np.max(np.abs(X))
    print(name, rep, 'max |dX| / max |X| = %.3g' % err)
    assert err <= 1e-12


@pytest.mark.parametrize('name,n_rep,flags', RUNS)
def test_device_equals_host_reference(name, n_rep, flags):
    N, R = SH.CASES[name][:2]
    in_lds, _ = _lib.simulate_batch_plan(N, R, flags)
    assert in_lds == (flags == 0 and name != 'n130')
    if name in SH.PLAN:
        assert in_lds == SH.PLAN[name][flags][0]
    out = _run(name, n_rep, flags)
    for i in range(n_rep):
        _check(out, name, i, i)
    if name == 'high_rate':
        assert out['exceptions'].min() >= 1 and out['S'].max() == 10
    if name == 'tail':
        assert out['S'][0, -R:-1].sum() > 0


@pytest.mark.parametrize('flags', (0, 1))
def test_batch_equals_singles_and_is_deterministic(flags):
    batch = _run('small_expl', 5, flags)
    again = _run('small_expl', 5, flags)
    for k in ('S', 'X', 'counts', 'exceptions'):
        assert batch[k].tobytes() == again[k].tobytes()
    for i in range(5):
        one = _run('small_expl', 1, flags, rep0=i)
        for k in ('S', 'X', 'counts', 'exceptions'):
            assert one[k][0].tobytes() == batch[k][i].tobytes()
    # rep0 shifts the stream index: replicate 1 of a batch from rep0 = 2 is stream 3
    _check(_run('small_expl', 2, flags, rep0=2), 'small_expl', 1, 3)


def test_counts_only_and_device_pointer_form():
    import torch
    name = 'n70'
    X0, AW, nlin, seed = SH.case(name)
    nT, N = X0.shape
    R = AW.shape[1]
    ref = _run(name, 2)
    out = _lib.simulate_batch(X0, AW, nlin, DT, 2, seed=seed, spikes=False)
    assert out['S'] is None and out['X'] is None
    assert np.array_equal(out['counts'], ref['counts']) and np.array_equal(out['exceptions'], ref['exceptions'])
    for flags in (0, 1):
        d_X0, d_AW = torch.from_numpy(np.array(X0)).cuda(), torch.from_numpy(np.array(AW)).cuda()
        d_c = torch.zeros((2, N), dtype=torch.int64, device='cuda')
        d_e = torch.zeros(2, dtype=torch.int64, device='cuda')
        d_ws = torch.empty(2 * R * N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        _lib.simulate_batch_dev(N, nT, R, nlin, DT, d_X0.data_ptr(), d_AW.data_ptr(), 2, d_c.data_ptr(), d_e.data_ptr(),
                                seed=seed, flags=flags, d_workspace=d_ws.data_ptr() if flags else 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_c.cpu().numpy(), ref['counts']) and np.array_equal(d_e.cpu().numpy(), ref['exceptions'])
    # a global ring without a workspace, a missing output: refused before anything is launched
    with pytest.raises(_lib.PglError, match='workspace'):
        _lib.simulate_batch_dev(N, nT, R, nlin, DT, d_X0.data_ptr(), d_AW.data_ptr(), 2, d_c.data_ptr(), d_e.data_ptr(), flags=1)
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_batch_dev(N, nT, R, nlin, DT, d_X0.data_ptr(), d_AW.data_ptr(), 2, 0, d_e.data_ptr())


def test_simulated_currents_are_the_currents_the_likelihood_kernels_see():
    """The reference's own consistency invariant (the one generate_synth_data asserts): on data simulated from x, the rate
    eval_state(x) computes from the spikes equals f_nlin of the simulation's total current."""
    N, pseed, nT, seed = SH.POP
    popn, x = SH.population(N, pseed)
    out = popn.simulate_batch(x, (0, nT * DT), DT, None, 0.1, 1, seed=seed, currents=True)
    S, X = out['S'][0], out['X'][0]
    assert S.shape == (nT, N) and S.sum() > 20
    host = popn.simulate_batch(x, (0, nT * DT), DT, None, 0.1, 1, seed=seed, currents=True, device=False)
    assert np.array_equal(host['S'][0], S)
    popn.add_data({'S': S.astype(np.float64), 'N': N, 'dt': DT, 'T': nT * DT, 'stim': None, 'dt_stim': 0.1})
    try:
        state = popn.eval_state(x)
        for n in range(N):
            assert np.allclose(state['glms'][n]['lam'], popn.glm.nlin_model.f_nlin(X[:, n]))
    finally:
        popn.release_data()


def test_predictive_counts():
    from theano_pyglm_amd.inference.predictive import predictive_counts, format_table
    N, nT, n_rep = 4, 5000, 64
    popn, x = SH.population(N, 5)
    # the "recording" is itself a draw from x, on a stream index the replicates (0 .. 63) do not use
    data_rep = popn.simulate_batch(x, (0, nT * DT), DT, None, 0.1, 1, seed=33, rep0=1000)
    S = data_rep['S'][0]
    popn.add_data({'S': S.astype(np.float64), 'N': N, 'dt': DT, 'T': nT * DT, 'stim': None, 'dt_stim': 0.1})
    try:
        res = predictive_counts(popn, x, n_rep, seed=33)
        print(format_table(res))
        c = res['counts']
        assert c.shape == (n_rep, N) and c.dtype == np.int64
        assert np.array_equal(res['observed'], S.sum(axis=0))
        assert np.all(res['observed'] >= c.min(axis=0)) and np.all(res['observed'] <= c.max(axis=0))
        assert np.array_equal(res['mean'], c.mean(axis=0)) and np.array_equal(res['std'], c.std(axis=0))
        lo, hi = np.percentile(c, [2.5, 97.5], axis=0)
        assert np.array_equal(res['lo'], lo) and np.array_equal(res['hi'], hi)
        le, ge = np.mean(c <= res['observed'], axis=0), np.mean(c >= res['observed'], axis=0)
        assert np.array_equal(res['p_value'], np.minimum(1.0, 2.0 * np.minimum(le, ge)))
        # the replicates are the batch's: the same counts as simulate_batch with the same seed
        same = popn.simulate_batch(x, (0, nT * DT), DT, None, 0.1, n_rep, seed=33, spikes=False)
        assert np.array_equal(same['counts'], c)
        popn.set_time_shard(0, 2)
        with pytest.raises(ValueError, match='time-sharded'):
            predictive_counts(popn, x, 2)
        popn.set_time_shard(None)
    finally:
        popn.release_data()
