"""k_rw_piece / k_rw_window (pgl_rate_windows_dev) through the C ABI on the cases of tests/rate_cases.json: N = 3 (one padded
post tile) and N = 17 (two tiles), nT = 1003, window lengths 1, 7, 256, 300 and 10 000 (>= the range), the whole recording
and a range [48, 981) whose windows start off the 16-bin grid of the event tables and whose last window and last piece are
short (pgl_set_time_range itself takes no t_lo off the 16-bin grid), a silent neuron, bins holding two and three spikes,
events in the first and in the last bin of a window and right behind t_hi, both nonlinearities, one case with dense stimulus
columns.  tests/test_rate_cases.py proves on the CPU that the table holds what it names.

Per (case, range, win): NaN-filled outputs, two calls with identical bits, nothing left NaN; obs exactly; Lam within the
bound of the pointwise block sums (tests/pointwise_reference.py: REL |Lam_ref| + ABS_A A_w, A_w = Lam_ref) of the longdouble
reference; the recorded launches end in the two kernels and equal the dry run of path 8; the host-pointer form is the same
call.  Per case: 5 jittered draws folded on the device against the host build of the rule fed the device's own Lam -- mean,
M2, min, max to the bit, pit to 1e-12 (the bound tests/test_gpu_pointwise.py puts on m + log e) --, d_lam only, d_acc only and
both together, one draw with a NaN bias.  A window's bits do not depend on its neighbours: win = 7 on [t_lo, t_hi) and on
[t_lo, t_lo + 7 k).  Every error code.  Population.compute_expected_counts and predictive.rate_bands end to end."""
import numpy as np
import pytest

from tests import rate_reference as R
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

CASES = R.load_cases()
PIT_REL = 1e-12


def _codes():
    import os
    import re
    src = open(os.path.join(R.ROOT, 'include', 'pyglm_hip.h')).read()
    return dict((k, int(v)) for k, v in re.findall(r'#define (PGL_ERR_[A-Z]+) \((-\d+)\)', src))


ERR = _codes()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _nan(*shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def _run(d, d_th, d_W, win, nw, N):
    import torch
    d_lam, d_obs = _nan(nw, N), _nan(nw, N)
    torch.cuda.synchronize()
    d.rate_windows_dev(d_th.data_ptr(), d_W.data_ptr(), win, d_lam.data_ptr(), d_obs.data_ptr())
    d.sync()
    return d_lam.cpu().numpy().copy(), d_obs.cpu().numpy().copy()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_rate_windows_case(c):
    p = R.problem(c)
    N = p.N
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d_th, d_W = _t(p.theta), _t(p.Weff)
        piece = 'k_rw_piece<%d>' % (c['kind'] == 'explinear')
        if c['Dstim'] == 0:
            plan = _lib.plan_kernels(N, B=p.B, R=p.R, Dstim=0, nT=p.nT, n_lo=0, count=N, path=8)
            assert plan[-2:] == ['k_rw_piece<0>', 'k_rw_window'], plan         # (the dry run's context has nlin = exp)
            assert plan[:-2] == _lib.plan_kernels(N, B=p.B, R=p.R, Dstim=0, nT=p.nT, n_lo=0, count=N, path=2)
        for t_lo, t_hi in R.ranges(c):
            d.set_time_range(t_lo, t_hi)
            for win in c['wins']:
                label = "%s [%d, %d) win %d" % (c['name'], t_lo, t_hi, win)
                ref_Lam, ref_obs = R.reference(c, t_lo, t_hi, win)
                nw = d.rate_windows_count(win)
                assert nw == ref_Lam.shape[0] == R.n_windows(t_hi - t_lo, win), label
                Lam, obs = _run(d, d_th, d_W, win, nw, N)
                names = d.last_kernels()
                assert names[-2:] == [piece, 'k_rw_window'], names
                if c['Dstim'] == 0 and (t_lo, t_hi) == (0, p.nT):
                    assert names[:-2] == plan[:-2], (names, plan)
                Lam2, obs2 = _run(d, d_th, d_W, win, nw, N)
                assert Lam.tobytes() == Lam2.tobytes() and obs.tobytes() == obs2.tobytes(), label + ": two calls differ"
                assert np.all(np.isfinite(Lam)) and np.all(np.isfinite(obs)), label + ": an output was never written"
                assert np.array_equal(obs, ref_obs), label
                r = R.ratio(Lam, ref_Lam)
                print("%s: worst |dLam| / ((1e-10 + 1e-12) Lam) = %.3e  (%d windows)" % (label, r, nw))
                assert r <= 1.0, label
                hl, ho = d.rate_windows(p.theta, p.Weff, win)                     # the host-pointer form is the same call
                assert np.array_equal(hl, Lam) and np.array_equal(ho, obs), label
            assert np.all(obs[:, c['silent']] == 0)
    finally:
        d.close()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_fold_over_draws(c):
    """5 jittered draws folded in on the device, each draw's Lam requested too; the final state against the host build of
    the rule fed those Lam.  Draw 2 carries a NaN bias in neuron 1: that neuron's planes are NaN, nothing else is."""
    import torch
    p = R.problem(c)
    N = p.N
    t_lo, t_hi = R.ranges(c)[-1]
    S = R.N_DRAWS
    sp, jp = 2, 1
    d = p.device(0)
    try:
        d.set_time_range(t_lo, t_hi)
        d_W = _t(p.Weff)
        th = np.array(R.draws(c))
        th[sp, jp, 0] = np.nan
        d_th = _t(th)
        for win in c['wins']:
            nw = d.rate_windows_count(win)

            def fold(fill, want_lam, want_acc):
                d_acc = torch.full((R.NACC, nw, N), fill, dtype=torch.float64, device='cuda')   # (draw 0 must initialise it)
                d_lam, d_obs = _nan(S, nw, N), _nan(nw, N)
                torch.cuda.synchronize()
                for s in range(S):
                    d.rate_windows_dev(d_th[s].data_ptr(), d_W.data_ptr(), win, d_lam[s].data_ptr() if want_lam else 0,
                                       d_obs.data_ptr() if s == 0 else 0, d_acc.data_ptr() if want_acc else 0, s)
                d.sync()
                return d_acc.cpu().numpy(), d_lam.cpu().numpy(), d_obs.cpu().numpy()

            acc, lam, obs = fold(4321.5, True, True)                  # both together
            acc_only = fold(-1.0, False, True)                        # the accumulator alone: the same state
            lam_only = fold(-1.0, True, False)                        # Lam alone: the same values, the state untouched
            assert acc_only[0].tobytes() == acc.tobytes() and np.all(np.isnan(acc_only[1]))
            assert lam_only[1].tobytes() == lam.tobytes() and np.all(lam_only[0] == -1.0)
            assert np.array_equal(obs, R.reference(c, t_lo, t_hi, win)[1])
            bad = np.zeros((nw, N), dtype=bool)
            bad[:, jp] = True
            assert np.array_equal(np.isnan(lam), np.broadcast_to(bad[None] & (np.arange(S) == sp)[:, None, None], lam.shape))
            host = R.host_fold(lam, obs)
            pit_nan = np.isnan(host[4]) & ~bad
            assert np.array_equal(np.isnan(acc[:4]), np.broadcast_to(bad[None], acc[:4].shape)), "NaN beyond the poisoned neuron"
            assert np.array_equal(np.isnan(acc[4]), bad | pit_nan)
            ok = ~bad
            for k, name in enumerate(('mean', 'M2', 'min', 'max')):
                assert np.array_equal(acc[k][ok], host[k][ok]), "%s win %d: %s differs from the host mirror" % (c['name'], win, name)
            fin = ok & ~pit_nan
            r_pit = float(np.max(np.abs(acc[4][fin] - host[4][fin]) / np.abs(host[4][fin])))
            print("%s win %5d: pit %.2e relative to the host mirror; %d of %d without a pit" % (c['name'], win, r_pit,
                                                                                           int(pit_nan.sum()), int(ok.sum())))
            assert r_pit <= PIT_REL
            assert np.all((acc[4][fin] > 0.0) & (acc[4][fin] <= 1.0))
    finally:
        d.close()


@pytest.mark.parametrize('c', CASES[:2], ids=[c['name'] for c in CASES[:2]])
def test_a_window_does_not_depend_on_its_neighbours(c):
    """win = 7 on [t_lo, t_hi) and on [t_lo, t_lo + 7 k): the first k windows have the same bits (Lam, obs and the planes)"""
    import torch
    p = R.problem(c)
    N = p.N
    t_lo, t_hi = 48, 981
    d = p.device(0)
    try:
        d_W = _t(p.Weff)
        d_th = _t(R.draws(c))
        res = []
        for hi in (t_hi, t_lo + 7 * 40, t_lo + 7 * 3):
            d.set_time_range(t_lo, hi)
            nw = d.rate_windows_count(7)
            d_acc, d_lam, d_obs = _nan(R.NACC, nw, N), _nan(nw, N), _nan(nw, N)
            torch.cuda.synchronize()
            for s in range(3):
                d.rate_windows_dev(d_th[s].data_ptr(), d_W.data_ptr(), 7, d_lam.data_ptr(), d_obs.data_ptr(), d_acc.data_ptr(), s)
            d.sync()
            res.append((d_lam.cpu().numpy(), d_obs.cpu().numpy(), d_acc.cpu().numpy()))
        assert res[0][0].shape[0] == 134 and res[1][0].shape[0] == 40 and res[2][0].shape[0] == 3
        for lam, obs, acc in res[1:]:
            k = lam.shape[0]
            assert res[0][0][:k].tobytes() == lam.tobytes() and res[0][1][:k].tobytes() == obs.tobytes()
            assert np.ascontiguousarray(res[0][2][:, :k]).tobytes() == acc.tobytes()
    finally:
        d.close()


def test_argument_and_state_errors():
    import torch
    buf = torch.zeros(4 * 200, dtype=torch.float64, device='cuda')
    d = _lib.DeviceGlm(4, 600, 5, 32, 'explinear', 0.001, 0)
    try:
        with pytest.raises(_lib.PglError, match="pgl_set_spikes"):
            d.rate_windows_dev(buf.data_ptr(), buf.data_ptr(), 50, buf.data_ptr())
        assert _lib.load().pgl_rate_windows_dev(d.h, buf.data_ptr(), buf.data_ptr(), 50, buf.data_ptr(), None, None, 0) == ERR['PGL_ERR_STATE']
        with pytest.raises(_lib.PglError, match="pgl_set_spikes"):
            d.rate_windows(np.zeros((4, 21)), np.zeros((4, 4)), 50)
        assert d.rate_windows_count(50) == 12 and d.rate_windows_count(600) == 1 and d.rate_windows_count(1 << 40) == 1
        d.set_spikes(np.zeros((600, 4), dtype=np.uint8))
        with pytest.raises(_lib.PglError, match="pgl_set_basis"):
            d.rate_windows_dev(buf.data_ptr(), buf.data_ptr(), 50, buf.data_ptr())
    finally:
        d.close()
    # n_win * N beyond the 32-bit grids: a property of the shape, refused before anything is looked at or launched
    d = _lib.DeviceGlm(3, 1 << 30, 5, 32, 'explinear', 0.001, 0)
    try:
        assert d.rate_windows_count(1) == 1 << 30
        with pytest.raises(_lib.PglError, match="too many windows") as e:
            d.rate_windows_dev(buf.data_ptr(), buf.data_ptr(), 1, buf.data_ptr())
        assert _lib.load().pgl_rate_windows_dev(d.h, buf.data_ptr(), buf.data_ptr(), 1, buf.data_ptr(), None, None, 0) == ERR['PGL_ERR_UNSUPPORTED']
        with pytest.raises(_lib.PglError, match="pgl_set_spikes"):                    # (a window length that fits: the state speaks)
            d.rate_windows_dev(buf.data_ptr(), buf.data_ptr(), 50, buf.data_ptr())
    finally:
        d.close()
    c = CASES[0]
    p = R.problem(c)
    d = p.device(0)
    try:
        d_th, d_W = _t(p.theta), _t(p.Weff)
        out = torch.zeros((R.NACC, 21, p.N), dtype=torch.float64, device='cuda')
        L = _lib.load()
        args = lambda **kw: dict(dict(d_theta=d_th.data_ptr(), d_Weff=d_W.data_ptr(), win=50, d_lam=out.data_ptr()), **kw)
        for kw, what in ((dict(win=0), "win"), (dict(win=-3), "win"), (dict(draw=-1, d_acc=out.data_ptr()), "draw"),
                         (dict(d_lam=0), "none of"), (dict(d_theta=0), "null"), (dict(d_Weff=0), "null")):
            with pytest.raises(_lib.PglError, match=what):
                d.rate_windows_dev(**args(**kw))
            a = args(**kw)
            rc = L.pgl_rate_windows_dev(d.h, a['d_theta'] or None, a['d_Weff'] or None, a['win'], a['d_lam'] or None, None,
                                        a.get('d_acc') or None, a.get('draw', 0))
            assert rc == ERR['PGL_ERR_ARG'], (kw, rc)
        with pytest.raises(_lib.PglError, match="win"):
            d.rate_windows_count(0)
        # every single output alone is a valid call
        for k in ('d_lam', 'd_obs', 'd_acc'):
            d.rate_windows_dev(d_th.data_ptr(), d_W.data_ptr(), 50, **{k: out.data_ptr()})
        d.sync()
    finally:
        d.close()


def test_population_expected_counts():
    """two data sequences = the sequences run one at a time; the column sums are compute_rescaled_intervals' expected counts"""
    from tests.test_gpu_hvp import _std_population
    popn = _std_population(3, 1.003, 5)
    try:
        rng = np.random.default_rng(6)
        S2 = np.minimum(rng.poisson(0.03, size=(777, 3)), 10).astype(np.uint8)
        popn.add_data({'S': S2, 'N': 3, 'dt': 0.001, 'T': 0.777, 'stim': None, 'dt_stim': 0.1})
        x = popn.sample(np.random.RandomState(3))
        seqs = list(popn.data_sequences)
        for win in (50, 300):
            Lam, obs = popn.compute_expected_counts(x, win)
            nw = [R.n_windows(1003, win), R.n_windows(777, win)]
            assert Lam.shape == obs.shape == (sum(nw), 3)
            theta, Weff = popn.theta_matrix(x), popn.W_eff(x)
            one = [popn._handle(s).rate_windows(theta, Weff, win) for s in seqs]
            assert np.array_equal(Lam, np.concatenate([o[0] for o in one])) and np.array_equal(obs, np.concatenate([o[1] for o in one]))
            assert np.array_equal(obs[:nw[0]].sum(axis=0), np.asarray(seqs[0]['S']).sum(axis=0))
            assert np.array_equal(obs[nw[0]:].sum(axis=0), S2.sum(axis=0))
            want = popn.compute_rescaled_intervals(x)[1][:, 0]
            assert np.all(np.abs(Lam.sum(axis=0) - want) <= 1e-12 * want), (win, Lam.sum(axis=0), want)
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                popn.compute_expected_counts(x, 50)
        finally:
            popn.set_time_shard(None)
    finally:
        popn.release_data()


def test_rate_bands_against_eval_state():
    """C1-sized (N = 4, nT = 60 000), draws theta + 0.01 z: mean and sd of the expected counts of 50-bin windows against the
    loop over eval_state reduced in numpy.  Both routes evaluate the rate in f64 from currents that differ by the order of
    their sums (~1e-13 of the current), so a window's count agrees to 1e-10 relative; an error eps in every draw's value
    moves the sd by at most 2 eps."""
    from tests.test_gpu_hvp import _std_population
    from theano_pyglm_amd.inference import batched_hmc as B
    from theano_pyglm_amd.inference import predictive as PP
    popn = _std_population(4, 60.0, 17)
    try:
        x = popn.sample(np.random.RandomState(11))
        S, win, dt = 5, 50, 0.001
        theta = popn.theta_matrix(x)
        smp = theta[None] + 0.01 * np.random.default_rng(2).standard_normal((S,) + theta.shape)
        res = PP.rate_bands(popn, x, smp, win=win, keep=True)
        nw = 1200
        assert res['mean'].shape == res['obs'].shape == res['pit'].shape == (nw, 4) and res['draws'].shape == (S, nw, 4)
        assert np.allclose(res['t0'], np.arange(nw) * 0.05) and np.allclose(res['width'], 0.05) and res['n_draws'] == S
        host = []
        for i in range(S):
            st = popn.eval_state(dict(x, glms=B.samples_to_states(popn, x, smp, i)))
            lam = np.stack([st['glms'][n]['lam'] for n in range(4)], axis=1)
            host.append(dt * np.add.reduceat(lam, np.arange(0, lam.shape[0], win), axis=0))
        host = np.array(host)
        mean, sd = host.mean(axis=0), host.std(axis=0, ddof=1)
        r_mean = float(np.max(np.abs(res['mean'] - mean) / mean))
        r_sd = float(np.max(np.abs(res['sd'] - sd) / mean))
        print("rate_bands against eval_state: mean %.2e relative, sd %.2e of the mean" % (r_mean, r_sd))
        assert r_mean <= 1e-10 and r_sd <= 2e-10
        Sd = np.asarray(popn.data_sequences[0]['S'])
        assert np.array_equal(res['obs'], np.add.reduceat(Sd.astype(np.int64), np.arange(0, 60000, win), axis=0))
        # keep=True is consistent with the planes
        dr = res['draws']
        assert np.array_equal(dr.min(axis=0), res['min']) and np.array_equal(dr.max(axis=0), res['max'])
        assert np.all(np.abs(dr.mean(axis=0) - res['mean']) <= 1e-14 * res['mean'])
        assert np.all(np.abs(dr.std(axis=0, ddof=1) - res['sd']) <= 1e-9 * res['mean'])
        host_acc = R.host_fold(dr, res['obs'])
        assert np.array_equal(host_acc[0], res['mean']) and np.all(np.abs(host_acc[4] - res['pit']) <= PIT_REL * host_acc[4])
        var = res['sd'] ** 2
        assert np.allclose(res['pearson'], (res['obs'] - res['mean']) / np.sqrt(res['mean'] + var), rtol=1e-12, atol=0)
        assert res['pit_ks'].shape == (4,) and np.all(res['n_pit_nan'] == 0)
        assert all(res['pit_ks'][m] == PP.ks_uniform(res['pit'][:, m]) for m in range(4))
        # a range of neurons from a device tensor with a chain axis: the same numbers
        import torch
        sub = PP.rate_bands(popn, x, torch.tensor(smp[:4, 1:3], device='cuda').reshape(2, 2, 2, -1), win=win, n_lo=1)
        full4 = PP.rate_bands(popn, x, smp[:4], win=win)
        assert np.array_equal(sub['mean'], full4['mean'][:, 1:3]) and np.array_equal(sub['pit'], full4['pit'][:, 1:3])
        print(PP.format_rate_table(res))
    finally:
        popn.release_data()
