"""The case table of the clamped simulation (tests/condsim_cases.json): the gcc mirror of the chain rule against the existing
host reference pgl_simulate_streams fed the clamped currents and the diagonal-only AW, spike for spike; what each case is in
the table for; the decision margin of the stream indices the GPU test runs."""
import numpy as np
import pytest

from tests import condsim_reference as CR
from theano_pyglm_amd import _lib

NAMES = [c['name'] for c in CR.CASES]
PLAIN = [n for n in NAMES if not CR.BY_NAME[n].get('exceptions')]


def _streams(name):
    """the stream indices compared with pgl_simulate_streams: the first, the last and up to two in between"""
    c = CR.BY_NAME[name]
    return sorted(set(int(i) for i in np.linspace(0, c['n_rep'] - 1, 4).round()))


@pytest.mark.parametrize('name', PLAIN)
def test_mirror_equals_simulate_streams_on_the_diagonal_only_couplings(name):
    c = CR.BY_NAME[name]
    X0, AW, _ = CR.make_case(name)
    m = CR.mirror(name)
    D = CR.diagonal_only(AW)
    for i in _streams(name):
        S, _, exc, closest = _lib.simulate_streams(m['Xc'], D, c['nlin'], CR.DT, rep=c['rep0'] + i, seed=c['seed'])
        assert exc == 0, (name, i)                                     # the condition of the comparison: asserted, never skipped
        assert S.dtype == np.uint8 and np.array_equal(S, m['S'][i]), (name, i)
        assert np.array_equal(S.sum(axis=0, dtype=np.int64), m['counts'][i])
        assert closest >= m['closest']                                 # the mirror's margin is over all replicates
    assert np.all(m['exceptions'] == 0)


@pytest.mark.parametrize('name', PLAIN)
def test_decision_margin_of_the_gpu_cases(name):
    """No comparison acc > thr of any chain the GPU test runs comes closer than 1e-9 (relative): a last-place difference
    between the device's and the host's exp / log cannot flip a spike."""
    print(name, CR.mirror(name)['closest'])
    assert CR.mirror(name)['closest'] > 1e-9


def test_library_host_reference_is_the_mirror():
    for name in ('n3_silent', 'burst', 'exceptions'):
        c = CR.BY_NAME[name]
        _, AW, _ = CR.make_case(name)
        m = CR.mirror(name)
        exc = np.zeros(c['N'], dtype=np.int64)
        for i in range(min(c['n_rep'], 3)):
            S, e, closest = _lib.simulate_cond_streams(m['Xc'], AW, c['nlin'], CR.DT, rep=c['rep0'] + i, seed=c['seed'])
            assert np.array_equal(S, m['S'][i]) and closest >= m['closest']
            exc += e
        if c['n_rep'] <= 3:
            assert np.array_equal(exc, m['exceptions'])
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_cond_streams(m['Xc'], AW, c['nlin'], CR.DT, rep=-1)


def test_cases_reach_what_they_are_for():
    by = CR.BY_NAME
    assert set((1, 3, 64, 65, 130)) <= set(c['N'] for c in CR.CASES)
    assert set((1, 64, 65, 130)) <= set(c['n_rep'] for c in CR.CASES)
    assert all(by[n]['rep0'] != 0 for n in ('n3_silent', 'n64_win1', 'rep130'))
    assert by['nt1_win_gt_nt']['nT'] == 1 < by['nt1_win_gt_nt']['win'] and by['nt_lt_r']['nT'] < by['nt_lt_r']['R']
    assert by['n3_silent']['nT'] % by['n3_silent']['win'] != 0 and by['n64_win1']['win'] == 1
    assert by['r1']['R'] == 1 and by['long_r200']['R'] == 200 and max(c['nT'] for c in CR.CASES) == 4096
    for name in PLAIN:
        m = CR.mirror(name)
        assert m['S'].sum() > 0, name
        # the recorded spikes did add currents (not where there is one bin, or no other neuron)
        assert np.any(m['Xc'] != CR.make_case(name)[0]) != (by[name]['nT'] == 1 or by[name]['N'] == 1), name
    c = by['n3_silent']
    m = CR.mirror('n3_silent')
    S_obs = CR.make_case('n3_silent')[2]
    assert m['S'][:, :, c['silent']].sum() == 0 and S_obs[:, c['silent_pre']].sum() == 0
    assert all(CR.make_case(n)[2].max() >= 2 for n in PLAIN if by[n]['nT'] > 100)        # recorded counts above 1 in a bin
    assert CR.mirror('nt_lt_r')['S'][:, :4].sum(axis=(0, 2)).min() > 0               # impulses cut by the end
    # the burst: more own spike bins inside R + 1 bins than the device's queue holds, and no exception
    m = CR.mirror('burst')
    assert CR.longest_own_spike_run(m['S'], by['burst']['R'] + 1) > CR.lib().condsim_queue() + 1 == _lib.CS_QUEUE + 1
    assert CR.longest_own_spike_run(CR.mirror('long_r200')['S'], 201) <= _lib.CS_QUEUE     # .. and a case that stays on the queue
    assert m['S'].max() >= 2
    # the exceptions case: the neuron's own cap
    m = CR.mirror('exceptions')
    assert m['exceptions'].min() >= 1 and m['S'].max() == 10 == CR.lib().condsim_cap()


def test_exceptions_are_per_neuron():
    """One neuron at the cap drops the round of ALL in pgl_simulate_streams; in the clamped rule it is that neuron's alone:
    with the capped bins in one column only, the other columns equal their 0-exception reference."""
    c = CR.BY_NAME['exceptions']
    X0, AW, S_obs = CR.make_case('exceptions')
    Xc = np.array(CR.mirror('exceptions')['Xc'])
    calm = np.array(X0[:, 1:])
    calm[50::40] = calm[51::40]
    Xc[:, 1:] += calm - X0[:, 1:]                                      # only neuron 0 keeps the bins with rate * dt = 14
    S, exc, _ = CR.host_run(Xc, AW, c['nlin'], CR.DT, 1, c['seed'], 3)
    assert exc[0] >= 1 and np.all(exc[1:] == 0) and S[0, :, 0].max() == 10
    ref, _, n_exc, _ = _lib.simulate_streams(Xc, CR.diagonal_only(AW), c['nlin'], CR.DT, rep=3, seed=c['seed'])
    assert n_exc >= 1
    alone = Xc.copy()
    alone[:, 0] = -40.0                                                # neuron 0 silenced: the others' 0-exception reference
    ref1, _, n_exc1, _ = _lib.simulate_streams(alone, CR.diagonal_only(AW), c['nlin'], CR.DT, rep=3, seed=c['seed'])
    assert n_exc1 == 0 and np.array_equal(S[0, :, 1:], ref1[:, 1:])
    # the capped bin records 10 spikes and scatters 9: the spikes up to the first capped bin agree with the reference
    t_cap = int(np.argmax(S[0, :, 0] == 10))
    assert np.array_equal(S[0, :t_cap + 1, 0], ref[:t_cap + 1, 0])
