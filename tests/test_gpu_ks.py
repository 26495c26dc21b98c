"""The goodness of fit on the device over tests/ks_cases.json (tests/test_ks_cases.py proves on the CPU that every case reaches
what it names and that the checks reject five emulated defects; tests/gof_reference.py has the references).

Corrected intervals (pgl_rescale_corr_dev), per (case, range): over NaN-filled outputs, twice (identical bits);
|tau' - ref| <= 1e-10 ref + 1e-12 Lambda_ref against the longdouble reference; stats = pgl_rescale_dev's, bit for bit, column
3 zero; draw 0 and draw 1 differ; every sub-range, on the 256-bin chunk grid or not, gives the whole range's intervals that
lie inside it bit for bit -- also where the explinear rate's series vote of a wave falls otherwise in the sub-range than in the
whole range (the case explinear_vote: other chunks share a wave, currents on both sides of 2.3 and 9.25).
KS (pgl_ks_uniform_dev) per case: zsorted is sorted and within 2 ulp of numpy's sorted z; the three distances recomputed in
numpy from the device's zsorted equal the device's bit for bit; |D - D_ref| <= 1e-14 (z <= 1, so a few ulp of expm1, one
division and one subtraction stay below 1e-15, and D is 1-Lipschitz in the sup norm of the sample); the NaN and n < 2 rules;
a segment alone and among 300 gives the same bits.
End to end at N = 4, nT = 4096: the device route of ks_time_rescaling against the host route, and ks_time_rescaling_draws
against a loop of single-point calls."""
import copy

import numpy as np
import pytest

from tests import gof_reference as GR
from tests import rescale_reference as RR
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

T = GR.load()
SEED = 5


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _corr(d, p, off, d_th, d_W, draw, corr=True):
    import torch
    d_off = _t(off, torch.int64)
    d_tau = torch.full((max(int(off[-1]), 1),), float('nan'), dtype=torch.float64, device='cuda')
    d_st = torch.full((p.N, 4), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    if corr:
        d.rescale_corr_dev(d_th, d_W, d_tau, d_off, d_st, seed=SEED, draw=draw)
    else:
        d.rescale_dev(d_th.data_ptr(), d_W.data_ptr(), d_tau.data_ptr(), d_off.data_ptr(), d_st.data_ptr())
    d.sync()
    return d_tau.cpu().numpy()[:int(off[-1])].copy(), d_st.cpu().numpy().copy()


@pytest.mark.parametrize('c', T['corr'], ids=[c['name'] for c in T['corr']])
def test_corrected_intervals(c):
    p = GR.problem(c)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d_th, d_W = _t(p.theta), _t(p.Weff)
        whole = None
        for t_lo, t_hi, hits in GR.corr_ranges(c):
            label = "%s [%d, %d)" % (c['name'], t_lo, t_hi)
            ref = GR.corr_reference(c, t_lo, t_hi, SEED, 1)
            d.set_time_range(t_lo, t_hi)
            off = d.rescale_count()
            assert np.array_equal(off, RR.offsets(ref[0])), label
            tau, st = _corr(d, p, off, d_th, d_W, 1)
            names = d.last_kernels()
            nl = int(c['kind'] == 'explinear')
            if t_lo % GR.L == 0:
                assert names[-3:] == ['k_rcorr_chunk<%d>' % nl, 'k_rescale_scan', 'k_rcorr_finish'], names
            else:                                      # a range that starts mid-chunk: the expected count by the sum from t_lo
                assert names[-4:] == ['k_rescale_chunk<%d>' % nl, 'k_rescale_scan', 'k_rcorr_chunk<%d>' % nl, 'k_rcorr_finish'], names
            tau2, st2 = _corr(d, p, off, d_th, d_W, 1)
            assert tau.tobytes() == tau2.tobytes() and st.tobytes() == st2.tobytes(), label + ": two calls differ"
            assert np.all(np.isfinite(tau)) and np.all(tau > 0.0), label
            r = GR.corr_ratio(tau, off, ref)
            print("%s: worst |dtau'| / (1e-10 tau' + 1e-12 Lambda) = %.3e  (%d intervals)" % (label, r, int(off[-1])))
            assert r <= 1.0, label
            tau_u, st_u = _corr(d, p, off, d_th, d_W, 0, corr=False)
            assert st.tobytes() == st_u.tobytes() and np.all(st[:, 3] == 0.0), label + ": stats"
            tau0, _ = _corr(d, p, off, d_th, d_W, 0)
            assert np.all(tau0 != tau) and np.all(tau0 < tau_u) and np.all(tau < tau_u), label + ": draws"
            assert GR.corr_ratio(tau0, off, GR.corr_reference(c, t_lo, t_hi, SEED, 0)) <= 1.0
            if whole is None:
                whole = (tau, off)
                continue
            for n in range(p.N):                       # the sub-range's intervals inside the whole range's
                j0, k = GR.first_index(p, n, t_lo), int(off[n + 1] - off[n])
                w = whole[0][whole[1][n] + j0:whole[1][n] + j0 + k]
                s = tau[off[n]:off[n + 1]]
                assert w.tobytes() == s.tobytes(), label + ": neuron %d differs from the whole range" % n
    finally:
        d.close()


@pytest.fixture(scope='module')
def dev():
    d = _lib.DeviceGlm(4, 2000, 5, 200, 'explinear', 0.001, 0)
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    yield d
    d.close()


def _ks(dev, tau, off):
    import torch
    ks, z = dev.ks_uniform(_t(tau), _t(off, torch.int64), zsorted=True)
    dev.sync()
    assert dev.last_kernels()[-1] == 'k_ks_segment'
    return ks.cpu().numpy(), z.cpu().numpy()


def _check_segment(label, tau, ks, z):
    ref = GR.ks_reference(tau)
    n = tau.size
    assert ks[3] == n, label
    if np.isnan(ref[0]):
        assert np.all(np.isnan(ks[:3])), label + ": the NaN / n < 2 rule"
        return
    assert np.all(np.diff(z) >= 0.0), label + ": zsorted is not sorted"
    zn = np.sort(-np.expm1(-tau))
    assert np.all(np.abs(z - zn) <= 2.0 * np.spacing(zn)), label + ": zsorted is no permutation of z"
    D, dp, dm = GR.ks_from_sorted(z)
    assert (ks[0], ks[1], ks[2]) == (D, dp, dm), label + ": distances of the device's own zsorted"
    err = np.max(np.abs(ks[:3] - ref[:3]))
    print("%s: n = %d, D = %.6g, max |D, D+, D- - ref| = %.2e" % (label, n, ks[0], err))
    assert err <= GR.KS_TOL, label


@pytest.mark.parametrize('c', T['ks'], ids=[c['name'] for c in T['ks']])
def test_ks_case(dev, c):
    tau = GR.ks_tau(c)
    ks, z = _ks(dev, tau, np.array([0, tau.size]))
    _check_segment(c['name'], tau, ks[0], z)
    ks2, z2 = _ks(dev, tau, np.array([0, tau.size]))
    assert ks.tobytes() == ks2.tobytes() and z.tobytes() == z2.tobytes()


def test_ks_300_segments_and_a_segment_alone(dev):
    import torch
    tau, off = GR.multi()
    ks, z = _ks(dev, tau, off)
    for m in range(off.size - 1):
        _check_segment("segment %d" % m, tau[off[m]:off[m + 1]], ks[m], z[off[m]:off[m + 1]])
    for m in (1, 4, 8, 10, 299):
        one, z1 = _ks(dev, tau[off[m]:off[m + 1]], np.array([0, off[m + 1] - off[m]]))
        assert one[0].tobytes() == ks[m].tobytes() and z1.tobytes() == z[off[m]:off[m + 1]].tobytes(), m
    # the handle's own buffer instead of zsorted, and the host-pointer form
    own = dev.ks_uniform(_t(tau), _t(off, torch.int64))
    dev.sync()
    assert own.cpu().numpy().tobytes() == ks.tobytes()
    hk, hz = dev.ks_uniform_host(tau, off, zsorted=True)
    assert hk.tobytes() == ks.tobytes() and hz.tobytes() == z.tobytes()


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


@pytest.mark.parametrize('nTs', [(4096,), (2048, 2048)], ids=['one-sequence', 'two-sequences'])
def test_device_route_equals_host_route(nTs):
    from theano_pyglm_amd.inference.gof import ks_time_rescaling
    popn, x = _population(nTs, 5)
    try:
        for correct in (False, True):
            a = ks_time_rescaling(popn, x, correct=correct, seed=SEED, device=False)
            b = ks_time_rescaling(popn, x, correct=correct, seed=SEED, device=True)
            assert a['route'] == 'host' and b['route'] == 'device'
            assert np.all(a['n_intervals'] >= 2)
            for key in ('D', 'D_plus', 'D_minus'):
                assert np.all(np.abs(a[key] - b[key]) <= 1e-14), (key, a[key], b[key])
            for key in ('n_intervals', 'expected_count', 'observed_count', 'multi_spike_bins', 'band', 'passed'):
                assert np.array_equal(a[key], b[key]), key
        u = ks_time_rescaling(popn, x)
        assert sorted(u) == sorted(b) and np.any(u['D'] != b['D'])
    finally:
        popn.release_data()


def test_draws_equal_a_loop_of_single_points():
    from theano_pyglm_amd.inference.gof import ks_time_rescaling, ks_time_rescaling_draws
    popn, x = _population((4096,), 7)
    try:
        th = popn.theta_matrix(x)
        rng = np.random.default_rng(3)
        samples = np.repeat(th[None, 1:3, :], 3, axis=0)              # the draws differ in the bias: x takes them back
        samples[:, :, 0] += 0.05 * rng.standard_normal((3, 2))
        res = ks_time_rescaling_draws(popn, x, samples, seed=SEED, n_lo=1)
        assert res['D'].shape == (3, 2) and res['n_draws'] == 3
        for s in range(3):
            y = copy.deepcopy(x)
            for i, n in enumerate((1, 2)):
                y['glms'][n]['bias']['bias'] = np.array([samples[s, i, 0]])
            assert np.array_equal(popn.theta_matrix(y)[1:3], samples[s])
            one = ks_time_rescaling(popn, y, correct=True, seed=SEED, device=True, draw=s)
            assert one['D'][1:3].tobytes() == res['D'][s].tobytes(), s
        assert np.array_equal(res['band'], one['band'][1:3]) and np.array_equal(res['n_intervals'], one['n_intervals'][1:3])
        assert np.allclose(res['D_mean'], res['D'].mean(axis=0)) and np.all((res['pass_share'] >= 0) & (res['pass_share'] <= 1))
        assert np.all(res['D_q05'] <= res['D_q95'])
        # with a chain axis: (2 chains, 3 draws) flatten to 6 draws, the first three as above
        both = ks_time_rescaling_draws(popn, x, np.stack([samples, samples[::-1]]), seed=SEED, n_lo=1)
        assert both['D'].shape == (6, 2) and both['D'][:3].tobytes() == res['D'].tobytes()
    finally:
        popn.release_data()
