"""Time-rescaling goodness of fit on the device (pgl_rescale_count / pgl_rescale_dev / pgl_rescale) against a reference
built independently of the device: currents x = feature_rows(fS, fstim, Weff[:, n]) . theta_n from the oracle's features,
rates from the oracle's nonlinearity, np.cumsum in np.longdouble, intervals by the definition in include/pyglm_hip.h.

Bound: |tau_dev - tau_ref| <= 1e-10 tau_ref + 1e-12 Lambda_ref (the project's rate parity, plus the f64 summation error
n eps Lambda of n <= 8192 bins); the same for Lambda; event counts exact; two calls bit-identical."""
import numpy as np
import pytest

from oracle import glm_oracle as O
from tests import helpers as H
from tests import hvp_reference as R
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

NT = 5000                       # 19.5 chunks of 256 bins
RANGE = (1616, 4200)            # t_lo = 16 * 101: chunks of the sub-range start at 1616 + 256 k
L = _lib.RESCALE_CHUNK


def _edit_spikes(S):
    """Neuron 0: no event.  Neuron 1: exactly one event.  Neuron 2: events on the first and the last bin of a chunk (of the
    whole recording: chunk 3; of RANGE: its chunk 2), on the bin behind each (neighbouring chunks), on the last bin of both
    ranges, and a two-spike bin on a chunk edge."""
    S[:, 0] = 0
    S[:, 1] = 0
    S[2000, 1] = 1
    for t in (3 * L, 4 * L - 1, 4 * L, RANGE[0] + 2 * L, RANGE[0] + 3 * L - 1, RANGE[0] + 3 * L, RANGE[1] - 1, NT - 1):
        S[t, 2] = max(S[t, 2], 1)
    S[4 * L - 1, 2] = 2
    S[RANGE[0], 3] = 1                                        # an event on the first bin of the sub-range
    S[0, 3] = 3


def _reference(S, x_of, theta, kind, dt, t_lo, t_hi):
    """(taus list, stats (N, 3)) by the definition; x_of(n) = bias-free or full current of neuron n over [t_lo, t_hi)."""
    N = S.shape[1]
    taus, stats = [], np.zeros((N, 3))
    for n in range(N):
        lam = O.nlin(x_of(n), kind)
        cum = np.cumsum(lam.astype(np.longdouble))
        ev = np.flatnonzero(S[t_lo:t_hi, n])
        taus.append(np.asarray(dt * (cum[ev[1:]] - cum[ev[:-1]]), dtype=np.float64) if ev.size > 1 else np.zeros(0))
        stats[n] = (float(dt * cum[-1]), ev.size, int(np.sum(S[t_lo:t_hi, n] > 1)))
    return taus, stats


_cache = {}


def _case(N, kind, Dstim):
    """The problem of a case and its references over the whole recording and over RANGE (built once, shared)."""
    key = (N, kind, Dstim)
    if key not in _cache:
        p = H.Problem(N, NT, H.std_ibasis(200), kind=kind, Dstim=Dstim, seed=101 + N + Dstim, weighted=True, rate_hz=50.0)
        _edit_spikes(p.S)
        refs = {}
        for t_lo, t_hi in ((0, NT), RANGE):
            x_of = lambda n: R.feature_rows(p.fS, p.fstim, p.Weff[:, n], t_lo, t_hi).dot(p.theta[n])
            refs[(t_lo, t_hi)] = _reference(p.S, x_of, p.theta, kind, p.dt, t_lo, t_hi)
        _cache[key] = (p, refs)
    return _cache[key]


def _check(tau, off, stats, ref, label):
    taus_ref, stats_ref = ref
    N = len(taus_ref)
    assert off.shape == (N + 1,) and off[0] == 0
    assert list(np.diff(off)) == [t.size for t in taus_ref]
    assert tau.shape == (int(off[-1]),)
    worst = 0.0
    for n in range(N):
        lam_ref = stats_ref[n, 0]
        d = np.abs(tau[off[n]:off[n + 1]] - taus_ref[n])
        bound = 1e-10 * taus_ref[n] + 1e-12 * lam_ref
        if d.size:
            worst = max(worst, float(np.max(d / bound)))
        assert np.all(d <= bound), (label, n, float(np.max(d / bound)))
        assert abs(stats[n, 0] - lam_ref) <= (1e-10 + 1e-12) * lam_ref, (label, n, stats[n, 0], lam_ref)
    print("%s: worst |tau_dev - tau_ref| / bound = %.3e, max |dLambda| / Lambda = %.3e"
          % (label, worst, float(np.max(np.abs(stats[:, 0] - stats_ref[:, 0]) / stats_ref[:, 0]))))
    assert np.array_equal(stats[:, 1], stats_ref[:, 1])
    assert np.array_equal(stats[:, 2], stats_ref[:, 2])
    assert np.all(stats[:, 3] == 0.0)


@pytest.mark.parametrize('rng_', [(0, NT), RANGE], ids=['whole', 'range'])
@pytest.mark.parametrize('Dstim', [0, 2])
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
@pytest.mark.parametrize('N', [8, 20])
def test_rescaled_intervals_match_reference(N, kind, Dstim, rng_):
    p, refs = _case(N, kind, Dstim)
    taus_ref, stats_ref = refs[rng_]
    # what the case is there for
    assert stats_ref[0, 1] == 0 and taus_ref[0].size == 0
    assert taus_ref[1].size == 0 and stats_ref[1, 1] == (1 if rng_[0] <= 2000 < rng_[1] else 0)
    assert np.sum(stats_ref[:, 2]) >= 2                      # two-spike bins
    d = p.device(0)
    try:
        if rng_ != (0, NT):
            d.set_time_range(*rng_)
        tau, off, stats = d.rescale(p.theta, p.Weff)
        assert np.array_equal(off, d.rescale_count())
        _check(tau, off, stats, refs[rng_], "N=%d %s Dstim=%d [%d, %d)" % ((N, kind, Dstim) + tuple(rng_)))
    finally:
        d.close()


def test_rescale_dev_twice_gives_identical_bits_and_records_its_kernels():
    import torch
    p, refs = _case(20, 'explinear', 2)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        off = d.rescale_count()
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
        d_th, d_W = t(p.theta), t(p.Weff)
        d_off = torch.tensor(off, dtype=torch.int64, device='cuda')
        outs = []
        for _ in range(2):
            d_tau = torch.full((int(off[-1]),), float('nan'), dtype=torch.float64, device='cuda')
            d_st = torch.full((p.N, 4), float('nan'), dtype=torch.float64, device='cuda')
            torch.cuda.synchronize()
            d.rescale_dev(d_th.data_ptr(), d_W.data_ptr(), d_tau.data_ptr(), d_off.data_ptr(), d_st.data_ptr())
            d.sync()
            outs.append((d_tau.cpu().numpy().copy(), d_st.cpu().numpy().copy()))
        names = d.last_kernels()
        print(names)
        assert names[-3:] == ['k_rescale_chunk<1>', 'k_rescale_scan', 'k_rescale_finish'] and len(names) > 3
        assert not any(n.startswith('k_rescale') for n in names[:-3])
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
        _check(outs[0][0], off, outs[0][1], refs[(0, NT)], "device pointers")
        tau, off2, stats = d.rescale(p.theta, p.Weff)          # the host form gives the same bits
        assert tau.tobytes() == outs[0][0].tobytes() and stats.tobytes() == outs[0][1].tobytes()
    finally:
        d.close()


def test_rescale_with_a_separable_stimulus():
    """Set up like tests/test_gpu_hvp.py's separable case; the dense host features do not exist there, so the reference
    currents are pgl_gibbs_currents'."""
    N = 8
    p = H.Problem(N, NT, H.std_ibasis(200), kind='explinear', seed=67, weighted=True, rate_hz=50.0)
    _edit_spikes(p.S)
    d = p.device(0)
    try:
        stim = np.random.default_rng(71).standard_normal((50, 6))
        d.set_stimulus_separable(stim, 0.1, H.std_ibasis(200)[:, :3])
        rng = np.random.default_rng(73)
        theta = np.zeros((N, d.P))
        theta[:, 0] = 20.0 + 0.3 * rng.standard_normal(N)
        theta[:, 1:1 + d.Dstim] = 0.3 * rng.standard_normal((N, d.Dstim))
        theta[:, 1 + d.Dstim:] = 2.0 * rng.standard_normal((N, N * p.B))
        for t_lo, t_hi in ((0, NT), RANGE):
            d.set_time_range(t_lo, t_hi)
            d.gibbs_prepare_all(theta, p.Weff)
            xs = [d.gibbs_currents(n, t_hi - t_lo) for n in range(N)]
            assert np.std(xs[3]) > 0
            ref = _reference(p.S, lambda n: theta[n, 0] + xs[n], theta, 'explinear', p.dt, t_lo, t_hi)
            tau, off, stats = d.rescale(theta, p.Weff)
            _check(tau, off, stats, ref, "separable [%d, %d)" % (t_lo, t_hi))
    finally:
        d.close()


def test_rescale_errors():
    import torch
    d = _lib.DeviceGlm(4, 2000, 5, 200, 'explinear', 0.001, 0)
    try:
        off = np.zeros(5, dtype=np.int64)
        with pytest.raises(_lib.PglError, match="error -3"):
            d.rescale_count()
        with pytest.raises(_lib.PglError, match="error -3"):
            d.rescale(np.zeros((4, d.P)), np.ones((4, 4)))
        buf = torch.zeros(64, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        with pytest.raises(_lib.PglError, match="error -3"):
            d.rescale_dev(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
        d.set_spikes(np.zeros((2000, 4), dtype=np.uint8))
        d.set_basis(H.std_ibasis(200))
        assert list(d.rescale_count()) == [0] * 5
        assert d.lib.pgl_rescale_count(d.h, None) == -1
        for k in range(5):
            args = [buf.data_ptr()] * 5
            args[k] = None
            assert d.lib.pgl_rescale_dev(d.h, *args) == -1
        # an all-silent population: no interval, zero events, a positive expected count
        theta = np.zeros((4, d.P))
        theta[:, 0] = 1.0
        tau, off, stats = d.rescale(theta, np.ones((4, 4)))
        assert tau.size == 0 and np.all(stats[:, 1:] == 0.0)
        assert np.allclose(stats[:, 0], 2000 * 0.001 * O.nlin(np.array(1.0), 'explinear'), rtol=1e-12)
    finally:
        d.close()


def test_population_intervals_and_ks_on_data_simulated_from_the_model():
    from theano_pyglm_amd.inference.gof import ks_time_rescaling, ks_from_intervals
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
    from theano_pyglm_amd.population import Population
    N, T = 4, 10.0
    popn = Population(stabilize_sparsity(make_model('standard_glm', N=N, dt=0.001)))
    x = popn.sample(np.random.RandomState(5))
    S, _ = popn.simulate(x, (0, T), 0.001, None, 0.1, rng=np.random.RandomState(6))
    data = {'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': None, 'dt_stim': 0.1}
    popn.add_data(data)
    try:
        taus, stats = popn.compute_rescaled_intervals(x)
        tau, off, st = popn._handle(data).rescale(popn.theta_matrix(x), popn.W_eff(x))
        assert len(taus) == N and np.array_equal(stats, st)
        for n in range(N):
            assert np.array_equal(taus[n], tau[off[n]:off[n + 1]])
        res = ks_time_rescaling(popn, x)
        D, band, passed, cnt = ks_from_intervals(taus)
        assert np.array_equal(res['D'], D, equal_nan=True) and np.array_equal(res['passed'], passed)
        assert np.array_equal(res['band'], band, equal_nan=True) and np.array_equal(res['n_intervals'], cnt)
        assert np.array_equal(res['observed_count'], np.count_nonzero(S, axis=0))
        assert np.array_equal(res['n_intervals'], np.maximum(res['observed_count'] - 1, 0))
        assert np.array_equal(res['expected_count'], stats[:, 0])
        print(res)
        # a sanity bound, not a statistical claim: the expected count within 5 sigma of the observed one
        assert np.all(res['observed_count'] > 20)
        assert np.all(np.abs(res['expected_count'] - res['observed_count']) <= 5.0 * np.sqrt(res['expected_count']))
    finally:
        popn.release_data()
