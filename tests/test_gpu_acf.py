"""k_acf_segment on the GPU over tests/acf_cases.json, outputs filled with NaN beforehand: two calls give equal bits; the device's
scores against the longdouble reference (4e-15 relative); the statistics the host mirror computes from the device's OWN scores
equal the device's bit for bit (this pins the summation rule and keeps libm out of it); r_k and Q against the reference within
the bounds of tests/acf_reference.py; the void rules; a segment alone and among 300; max_lag 64 and 1 give the same r_1.  Then
end to end: the device route of independence_time_rescaling against the host route on two data sequences, and
independence_time_rescaling_draws against a loop of single points."""
import copy

import numpy as np
import pytest

from tests import acf_reference as AR
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu
SEED = 5
CASES = AR.load()


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


@pytest.fixture(scope='module')
def dev():
    d = _lib.DeviceGlm(4, 2000, 5, 200, 'explinear', 0.001, 0)
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    yield d
    d.close()


def _acf(dev, tau, segs, L):
    import torch
    run_off, seg_run = AR.offsets(segs)
    out = torch.full((len(segs), AR.NHEAD + L), float('nan'), dtype=torch.float64, device='cuda')
    g = torch.full((max(tau.size, 1),), float('nan'), dtype=torch.float64, device='cuda')
    dev.rescale_acf(_t(tau), _t(run_off, torch.int64), _t(seg_run, torch.int64), L, out=out, scores=g)
    dev.sync()
    assert dev.last_kernels()[-1] == 'k_acf_segment'
    return out.cpu().numpy(), g.cpu().numpy()[:tau.size]


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_acf_case(dev, c):
    tau, runs, L = AR.case_tau(c), c['runs'], c['L']
    out, g = _acf(dev, tau, [runs], L)
    out2, g2 = _acf(dev, tau, [runs], L)
    assert out.tobytes() == out2.tobytes() and g.tobytes() == g2.tobytes()
    mirror = AR.host_from_scores(tau, g, [runs], L)
    assert mirror.tobytes() == out.tobytes(), (c['name'], mirror, out)
    es, er = AR.check_against_reference(c['name'], out[0], g, tau, runs, L)
    print("%-14s scores %.2e relative, r %.2e absolute" % (c['name'], es, er))
    if 'void_tau' in c['expect']:
        assert np.all(np.isnan(out[0, 1:])) and out[0, 0] == tau.size
    if 'void_n' in c['expect'] or 'void_c0' in c['expect']:
        assert np.all(np.isnan(out[0, AR.NHEAD:])) and np.isnan(out[0, 3]) and out[0, 4] == 0.0
    if 'lag_ge_n' in c['expect']:
        nk = AR.pair_counts(runs, L)
        assert np.array_equal(np.isnan(out[0, AR.NHEAD:]), nk == 0) and out[0, 4] == np.sum(nk > 0)


def test_a_segment_alone_and_among_300(dev):
    by = dict((c['name'], c) for c in CASES)
    c = by['runs3_short']
    tau, segs, at = AR.crowd(c)
    out, g = _acf(dev, tau, segs, c['L'])
    run_off, seg_run = AR.offsets(segs)
    assert AR.host_from_scores(tau, g, segs, c['L']).tobytes() == out.tobytes()
    alone, g1 = _acf(dev, AR.case_tau(c), [c['runs']], c['L'])
    a = int(run_off[seg_run[at]])
    assert out[at].tobytes() == alone[0].tobytes() and g[a:a + g1.size].tobytes() == g1.tobytes()
    for m in (0, 7, 8, 300):
        lo, hi = int(run_off[seg_run[m]]), int(run_off[seg_run[m + 1]])
        AR.check_against_reference("segment %d" % m, out[m], g[lo:hi], tau[lo:hi], segs[m], c['L'])
    # max_lag = 64 and max_lag = 1: the same r_1, mean and c_0
    wide, _ = _acf(dev, AR.case_tau(c), [c['runs']], 64)
    one, _ = _acf(dev, AR.case_tau(c), [c['runs']], 1)
    assert wide[0, AR.NHEAD] == one[0, AR.NHEAD] == alone[0, AR.NHEAD] and wide[0, :3].tobytes() == one[0, :3].tobytes()
    assert wide[0, AR.NHEAD:AR.NHEAD + 20].tobytes() == alone[0, AR.NHEAD:].tobytes()
    # the host-pointer form
    ho, hg = dev.rescale_acf_host(tau, run_off, seg_run, c['L'], scores=True)
    assert ho.tobytes() == out.tobytes() and hg.tobytes() == g.tobytes()
    with pytest.raises(_lib.PglError):
        dev.rescale_acf_host(tau, run_off, seg_run, 65)
    with pytest.raises(_lib.PglError):
        dev.rescale_acf_dev(1, 1, 1, 1, 0, 1, 1)


def _population(nTs, seed):
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
    from theano_pyglm_amd.population import Population
    N = 4
    popn = Population(stabilize_sparsity(make_model('standard_glm', N=N, dt=0.001)))
    x = popn.sample(np.random.RandomState(seed))
    for i, nT in enumerate(nTs):
        S, _ = popn.simulate(x, (0, nT * 0.001), 0.001, None, 0.1, rng=np.random.RandomState(seed + 1 + i))
        popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': nT * 0.001, 'stim': None, 'dt_stim': 0.1})
    return popn, x


def test_device_route_equals_host_route_on_two_sequences():
    from theano_pyglm_amd.inference.gof import independence_time_rescaling, format_independence_table
    popn, x = _population((2048, 2048), 5)
    try:
        for correct in (False, True):
            a = independence_time_rescaling(popn, x, max_lag=20, correct=correct, seed=SEED, device=False)
            b = independence_time_rescaling(popn, x, max_lag=20, correct=correct, seed=SEED, device=True)
            assert a['route'] == 'host' and b['route'] == 'device' and a['r'].shape == (4, 20)
            assert np.array_equal(a['n_intervals'], b['n_intervals']) and np.all(a['n_intervals'] >= 3)
            assert np.array_equal(a['dof'], b['dof']) and np.array_equal(a['r_band'], b['r_band'], equal_nan=True)
            assert np.array_equal(np.isnan(a['r']), np.isnan(b['r']))
            ok = ~np.isnan(a['r'])
            # (the two routes differ in libm and in the rounding of the intervals themselves: the reference's bounds)
            assert np.all(np.abs(a['r'][ok] - b['r'][ok]) <= AR.R_TOL), np.max(np.abs(a['r'][ok] - b['r'][ok]))
            assert np.all(np.abs(a['Q'] - b['Q']) <= AR.Q_RTOL * np.abs(a['Q']))
            assert np.all(np.abs(a['p_value'] - b['p_value']) <= 1e-8)
            assert np.all(np.abs(a['mean_score'] - b['mean_score']) <= 1e-12)
        assert "neurons pass" in format_independence_table(b)
    finally:
        popn.release_data()


def test_draws_equal_a_loop_of_single_points():
    from theano_pyglm_amd.inference.gof import (independence_time_rescaling, independence_time_rescaling_draws,
                                                format_independence_draws_table)
    popn, x = _population((4096,), 7)
    try:
        th = popn.theta_matrix(x)
        rng = np.random.default_rng(3)
        samples = np.repeat(th[None, 1:3, :], 3, axis=0)              # the draws differ in the bias: x takes them back
        samples[:, :, 0] += 0.05 * rng.standard_normal((3, 2))
        res = independence_time_rescaling_draws(popn, x, samples, max_lag=20, seed=SEED, n_lo=1)
        assert res['Q'].shape == (3, 2) and res['r1'].shape == (3, 2) and res['n_draws'] == 3
        for s in range(3):
            y = copy.deepcopy(x)
            for i, n in enumerate((1, 2)):
                y['glms'][n]['bias']['bias'] = np.array([samples[s, i, 0]])
            assert np.array_equal(popn.theta_matrix(y)[1:3], samples[s])
            one = independence_time_rescaling(popn, y, max_lag=20, correct=True, seed=SEED, device=True, draw=s)
            assert one['Q'][1:3].tobytes() == res['Q'][s].tobytes(), s
            assert one['r'][1:3, 0].tobytes() == res['r1'][s].tobytes(), s
            assert one['p_value'][1:3].tobytes() == res['p_value'][s].tobytes(), s
        assert np.array_equal(res['n_intervals'], one['n_intervals'][1:3])
        assert np.all((res['pass_share'] >= 0) & (res['pass_share'] <= 1)) and np.all(res['r1_q05'] <= res['r1_q95'])
        assert "posterior draws" in format_independence_draws_table(res)
    finally:
        popn.release_data()
