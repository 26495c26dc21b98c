"""GPU tests of the warm-up mass adaptation (mass='adapt': pgl_mass_adapt_dev, pgl_nuts_adapt_step_dev) and of several
chains per neuron (n_chains) in the lock-step samplers.

Against the mirror (tests/adapt_mirror.py: csrc/pglm_adapt.h on top of the HMC / NUTS mirrors), both fed by the DEVICE's
evaluations, so the two differ by rounding only (the order of the row sums, fused multiply-adds) and no decision can flip
unless its margin is of that size.  HMC: the device chain records every (ll, grad) it consumed and the mirror replays
them in order.  NUTS: launch by launch from the device's own state (see test_nuts_adapt_equals_mirror for why).  Tolerances: test_gpu_hmc's and test_gpu_nuts's for the unadapted chains -- kept draws
1e-9 of the row's largest entry, HMC steps rtol 1e-15 (a bang-bang rule), NUTS steps and statistics 1e-9 -- and minv, a
smooth function of the draws, the draws' 1e-9.  n_warmup = 201 is the shortest warm-up with two windows: (75, 100),
(100, 151)."""
import numpy as np
import pytest

from tests import adapt_mirror as AM
from tests import helpers as H
from tests import hmc_mirror as HM
from tests import nuts_mirror as NM
from tests.test_gpu_hmc import GAUSS
from theano_pyglm_amd.inference import mass_adapt as MA

N_WARM = 201
PRM = GAUSS


class Replay(object):
    """target(X) for a mirror: the recorded evaluations in order; X must be the recorded point to 1e-9."""

    def __init__(self, rec):
        self.rec, self.k, self.err = rec, 0, 0.0

    def __call__(self, X):
        assert self.k < len(self.rec), "the mirror asks for more evaluations than the device made (%d)" % len(self.rec)
        Xr, ll, g = self.rec[self.k]
        e = np.max(np.abs(X - Xr) / np.max(np.abs(Xr), axis=1, keepdims=True), axis=1)
        assert np.all(e <= 1e-6), "evaluation %d: the mirror's points left the device's, per row %s" % (self.k, e)
        self.k += 1
        self.err = max(self.err, float(e.max()))
        return ll.copy(), g.copy()


def _setup(p, M, P):
    import torch
    dev = torch.device('cuda', 0)
    h = p.device(0)
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    Weff = torch.tensor(p.Weff, dtype=torch.float64, device=dev)
    buf = torch.empty(M * (1 + P), dtype=torch.float64, device=dev)
    return torch, dev, h, stream, Weff, buf


def hmc_device(p, X0, n_lo, n_hi, n_trans, L, step, seed, n_warmup):
    M, P = X0.shape
    torch, dev, h, stream, Weff, buf = _setup(p, M, P)
    f64 = torch.float64
    try:
        with torch.cuda.stream(stream):
            st = torch.zeros(h.hmc_state_doubles(M, P), dtype=f64, device=dev)
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            sc = st[4 * M * P:].view(10, M)
            windows = MA.adapt_windows(n_warmup)
            ad = torch.zeros(h.adapt_state_doubles(M, P), dtype=f64, device=dev)
            assert ad.numel() == 2 * M * P + 2 * M
            sched = torch.tensor(MA.schedule_ints(windows), dtype=torch.int32, device=dev)
            minv = torch.ones((M, P), dtype=f64, device=dev)
            Xt = torch.empty((M, P), dtype=f64, device=dev)
            samples = torch.zeros((n_trans, M, P), dtype=f64, device=dev)
            rec, steps, minvs = [], [], []

            def evaluate(Xe):
                h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), n_lo, n_hi)
                stream.synchronize()
                rec.append((Xe.cpu().numpy().copy(), buf[:M].cpu().numpy().copy(), buf[M:].view(M, P).cpu().numpy().copy()))
                return buf[:M], buf[M:]

            ll, g = evaluate(st[:M * P].view(M, P))
            h.hmc_init_dev(st.data_ptr(), M, P, n_lo, ll.data_ptr(), g.data_ptr(), PRM, step, seed)
            for t in range(n_trans):
                h.hmc_begin_dev(st.data_ptr(), M, P, minv.data_ptr(), Xt.data_ptr())
                for i in range(L):
                    ll, g = evaluate(Xt)
                    h.hmc_leap_dev(st.data_ptr(), M, P, minv.data_ptr(), ll.data_ptr(), g.data_ptr(), PRM, i == L - 1, n_warmup,
                                   Xt.data_ptr(), samples[t].data_ptr() if i == L - 1 else 0)
                h.mass_adapt_dev(st.data_ptr(), M, P, ad.data_ptr(), sched.data_ptr(), minv.data_ptr())
                stream.synchronize()
                steps.append(sc[HM.SC['step']].cpu().numpy())
                minvs.append(minv.cpu().numpy())
            return {'samples': samples.cpu().numpy(), 'sc': sc.cpu().numpy(), 'steps': np.array(steps), 'minv': np.array(minvs),
                    'ad': ad.cpu().numpy(), 'rec': rec}
    finally:
        h.close()


def nuts_device(p, X0, n_lo, n_hi, n_keep, D, step, seed, n_warmup):
    M, P = X0.shape
    torch, dev, h, stream, Weff, buf = _setup(p, M, P)
    f64 = torch.float64
    try:
        with torch.cuda.stream(stream):
            st = torch.zeros(h.nuts_state_doubles(M, P, D), dtype=f64, device=dev)
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            sc = st[(NM.NVEC + 2 * D) * M * P:].view(len(NM.FIELDS), M)
            ad = torch.zeros(h.adapt_state_doubles(M, P), dtype=f64, device=dev)
            sched = torch.tensor(MA.schedule_ints(MA.adapt_windows(n_warmup)), dtype=torch.int32, device=dev)
            minv = torch.ones((M, P), dtype=f64, device=dev)
            step0 = torch.full((M,), step, dtype=f64, device=dev)
            Xt = torch.empty((M, P), dtype=f64, device=dev)
            samples = torch.zeros((n_keep, M, P), dtype=f64, device=dev)
            stats = torch.zeros((n_keep, 2, M), dtype=f64, device=dev)
            rec, log, t_prev, snaps = [], [[] for _ in range(M)], np.zeros(M), []

            def snap():
                snaps.append(torch.cat([st, ad, minv.flatten(), Xt.flatten()]).cpu().numpy())

            def evaluate(Xe):
                h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), n_lo, n_hi)
                stream.synchronize()
                rec.append((Xe.cpu().numpy().copy(), buf[:M].cpu().numpy().copy(), buf[M:].view(M, P).cpu().numpy().copy()))
                return buf[:M], buf[M:]

            ll, g = evaluate(st[:M * P].view(M, P))
            h.nuts_init_dev(st.data_ptr(), M, P, D, n_lo, ll.data_ptr(), g.data_ptr(), PRM, minv.data_ptr(), 0, step0.data_ptr(),
                            seed, n_warmup, 1, n_keep, Xt.data_ptr())
            stream.synchronize()
            snap()
            for launch in range(20000):
                ll, g = evaluate(Xt)
                h.nuts_adapt_step_dev(st.data_ptr(), M, P, D, ll.data_ptr(), g.data_ptr(), PRM, minv.data_ptr(), ad.data_ptr(),
                                      sched.data_ptr(), 0.8, n_warmup, 1, n_keep, Xt.data_ptr(), samples.data_ptr(),
                                      stats.data_ptr())
                stream.synchronize()
                snap()
                s = sc.cpu().numpy()
                ended = np.flatnonzero(s[NM.SC['t']] != t_prev)
                if ended.size:
                    mv = minv.cpu().numpy()
                    for r in ended:
                        log[r].append((tuple(int(s[NM.SC[k], r]) for k in ('last_depth', 'last_nleaf', 'last_stop', 'last_sel')),
                                       s[NM.SC['step'], r], s[NM.SC['last_acc'], r], mv[r].copy()))
                t_prev = s[NM.SC['t']].copy()
                if np.all(s[NM.SC['done']] != 0.0):
                    break
            assert np.all(s[NM.SC['done']] != 0.0)
            return {'samples': samples.cpu().numpy(), 'stats': stats.cpu().numpy(), 'sc': s, 'log': log, 'rec': rec,
                    'minv': minv.cpu().numpy(), 'ad': ad.cpu().numpy(), 'snaps': snaps}
    finally:
        h.close()


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=-1, keepdims=True)))


def _prior(p):
    return (PRM[0], p.N, p.B, p.Dstim, PRM[1:])


# (N, n_lo, n_hi): P = 11 < 64;  P = 26, no multiple of 64, M = 3;  one row
SHAPES = [(2, 0, 2), (5, 1, 4), (5, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('N,n_lo,n_hi', SHAPES)
def test_hmc_adapt_equals_mirror(N, n_lo, n_hi):
    """Through both window ends (t = 99, 150) and five kept draws: minv after every transition, the steps, the draws."""
    p = H.Problem(N, 2000, H.std_ibasis(), kind='explinear', seed=31)
    X0 = p.theta[n_lo:n_hi].copy()
    n_trans, L = N_WARM + 5, 3
    d = hmc_device(p, X0, n_lo, n_hi, n_trans, L, 0.5, 3, N_WARM)
    rp = Replay(d['rec'])
    mir = AM.HmcMirror(rp, X0, N_WARM, n_lo=n_lo, prior=_prior(p), step0=0.5, seed=3)
    steps, minvs, samples, accs = [], [], [], []
    for t in range(n_trans):
        s, a, _ = mir.transition(L)
        samples.append(s), accs.append(a), steps.append(mir.sc[HM.SC['step']].copy()), minvs.append(mir.minv.copy())
    assert rp.k == len(d['rec']) and rp.err <= 1e-9
    accs = np.array(accs)
    print("accepted %d of %d; replayed points agree to %.2e; minv range %.2e .. %.2e" % (accs.sum(), accs.size, rp.err,
                                                                                          d['minv'][-1].min(), d['minv'][-1].max()))
    assert accs.any() and not accs.all()
    assert np.array_equal(d['sc'][HM.SC['n_accept']], mir.sc[HM.SC['n_accept']])
    assert np.allclose(d['steps'], np.array(steps), rtol=1e-15, atol=0.0)
    err_m, err_s = _rel(d['minv'], np.array(minvs)), _rel(d['samples'], np.array(samples))
    print("device against mirror: minv %.2e, samples %.2e" % (err_m, err_s))
    assert err_m <= 1e-9 and err_s <= 1e-9
    # minv changes exactly at the two window ends and is frozen afterwards
    changed = [t for t in range(1, n_trans) if not np.array_equal(d['minv'][t], d['minv'][t - 1])]
    assert changed == [99, 150] and np.all(d['minv'][98] == 1.0)
    M, P = X0.shape
    assert np.all(d['ad'][:2 * M * P] == 0.0) and np.all(d['ad'][2 * M * P:2 * M * P + M] == 0.0) and np.all(d['ad'][2 * M * P + M:] == 2.0)
    assert np.allclose(d['sc'][HM.SC['avg_accept']], mir.sc[HM.SC['avg_accept']], rtol=1e-15, atol=0.0)


def _close(a, b, shape):
    """|a - b| <= 1e-9 of the largest entry of b's row (rows: the last axis of `shape`); infinities must be equal."""
    a, b = a.reshape(shape), b.reshape(shape)
    fin = np.isfinite(b)
    if not np.array_equal(fin, np.isfinite(a)) or not np.array_equal(a[~fin], b[~fin]):
        return np.inf
    scale = np.max(np.where(fin, np.abs(b), 0.0), axis=-1, keepdims=True)
    d = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)), 0.0)
    bad = d > 1e-9 * scale
    return float(np.max(d / np.where(scale > 0.0, scale, 1.0))) if not bad.any() else float(np.max(np.where(bad, np.inf, 0.0)))


@pytest.mark.gpu
@pytest.mark.parametrize('N,n_lo,n_hi', SHAPES)
def test_nuts_adapt_equals_mirror(N, n_lo, n_hi):
    """max_depth = 4, through both window ends and five kept draws, EVERY launch against the mirror: the mirror takes the
    device's state before the launch and the evaluation the device consumed, makes the same step, and the whole state after
    it -- every vector, every scalar (the decisions, the step, the statistic of a transition that ended: computed under
    ONE mass, the mirror switches only at the boundary), the adaptation state, minv and the next points -- agrees to 1e-9 of
    the row's largest entry; then the kept draws and their statistics.

    Why per launch: run freely from the same start, the two chains drift apart although nothing is wrong -- measured here
    (N = 2, step 0.3, seed 2, the mirror evaluating its own points on the device): relative step error 3e-15 after
    transition 0, 2.5e-12 after 20, 1.3e-8 after 40, 4.5e-7 after 70, all BEFORE the first window's end, the first differing
    tree at transition 174 (row 0) and 88 (row 1).  The dual averaging feeds every rounding difference of exp(H0 - H) back
    into the step of the next tree.  The free-running comparison over 8 transitions is tests/test_gpu_nuts.py's."""
    p = H.Problem(N, 2000, H.std_ibasis(), kind='explinear', seed=31)
    X0 = p.theta[n_lo:n_hi].copy()
    M, P = X0.shape
    D, n_keep = 4, 5
    d = nuts_device(p, X0, n_lo, n_hi, n_keep, D, 0.3, 2, N_WARM)
    rp = Replay(d['rec'])
    mir = AM.NutsMirror(rp, X0, n_keep, N_WARM, max_depth=D, n_lo=n_lo, prior=_prior(p), step0=0.3, seed=2)
    n_st, n_ad, MP = mir.st.size, mir.ad.st.size, M * P
    n_vec = (NM.NVEC + 2 * D)

    def parts(z):
        return z[:n_st], z[n_st:n_st + n_ad], z[n_st + n_ad:n_st + n_ad + MP], z[n_st + n_ad + MP:]

    def compare(k):
        st, ad, mv, xt = parts(d['snaps'][k])
        errs = (_close(mir.st[:n_vec * MP], st[:n_vec * MP], (n_vec * M, P)), _close(mir.st[n_vec * MP:], st[n_vec * MP:], (-1, 1)),
                _close(mir.ad.st[:2 * MP], ad[:2 * MP], (2 * M, P)), _close(mir.ad.st[2 * MP:], ad[2 * MP:], (-1, 1)),
                _close(mir.minv.ravel(), mv, (M, P)), _close(mir.Xt.ravel(), xt, (M, P)))
        assert max(errs) <= 1e-9, "launch %d: vectors, scalars, Welford, counts, minv, Xt: %s" % (k, errs)
        return max(errs)

    worst = compare(0)                                          # (after init)
    ends = 0
    for k in range(1, len(d['snaps'])):
        st, ad, mv, xt = parts(d['snaps'][k - 1])
        mir.st[:], mir.ad.st[:], mir.minv[:], mir.Xt[:] = st, ad, mv.reshape(M, P), xt.reshape(M, P)
        acts = mir.step()
        ends += int(np.sum((acts & NM.END) != 0))
        worst = max(worst, compare(k))
    assert rp.k == len(d['rec']) == len(d['snaps']) and rp.err == 0.0
    print("%d launches, %d transitions; device against mirror, launch by launch: largest error %.2e" % (rp.k - 1, ends, worst))
    assert ends == M * (N_WARM + n_keep)
    assert _close(mir.samples.ravel(), d['samples'], (n_keep * M, P)) <= 1e-9 and np.array_equal(mir.stats, d['stats'])
    for r in range(M):
        dl = d['log'][r]
        assert len(dl) == N_WARM + n_keep
        changed = [t for t in range(1, len(dl)) if not np.array_equal(dl[t][3], dl[t - 1][3])]
        assert changed == [99, 150] and np.all(dl[98][3] == 1.0), (r, changed)
        assert len(set(e[0][0] for e in dl)) > 1                                # trees of several depths
    assert np.array_equal(d['ad'][-M:], np.full(M, 2.0)) and np.all(d['sc'][NM.SC['done']] != 0.0)


# ---- the drivers -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def popn():
    from tests.test_gpu_hvp import _std_population
    p = _std_population(4, 3.0, 89, nlin='exp', bias_mu=3.0)
    yield p, p.sample(np.random.RandomState(97))
    p.release_data()


def _hmc(popn, x, **kw):
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc
    a = dict(n_warmup=40, n_leapfrog=3, step_sz=0.05, seed=5)
    a.update(kw)
    return sample_glms_hmc(popn, x, 4, **a)


def _nuts(popn, x, **kw):
    from theano_pyglm_amd.inference.batched_nuts import sample_glms_nuts
    a = dict(n_warmup=40, max_depth=3, step_sz=0.05, seed=5)
    a.update(kw)
    return sample_glms_nuts(popn, x, 4, **a)


KEYS = ('samples', 'step_sz', 'accept_rate', 'minv')


@pytest.mark.gpu
@pytest.mark.parametrize('run', [_hmc, _nuts])
def test_determinism_slicing_and_stats(popn, run):
    """n_warmup = 40: one window (6, 36)."""
    p, x = popn
    a = run(p, x, mass='adapt')
    st = dict(p.last_fit_stats)
    b = run(p, x, mass='adapt')
    sub = run(p, x, mass='adapt', n_lo=1, n_hi=3)
    P = p.glm.P
    assert a['minv'].shape == (4, P) and a['adapt_windows'] == [(6, 36)] and np.all(a['minv'] > 0.0) and np.any(a['minv'] != 1.0)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(sub[k], a[k][..., 1:3, :] if a[k].ndim > 1 else a[k][1:3]), k
    assert st['mass'] == 'adapted diagonal' and st['mass_setup_s'] == 0
    if run is _hmc:
        run(p, x)
        assert st['host_syncs_in_chain'] == p.last_fit_stats['host_syncs_in_chain'] == 0
        assert st['adapt_launches'] == 30 and st['row_launches_per_transition'] == 4


@pytest.mark.gpu
@pytest.mark.parametrize('run', [_hmc, _nuts])
def test_freezing(popn, run):
    p, x = popn
    # one kept draw against four: minv is what it was right after the last window
    one = run(p, x, mass='adapt')
    from theano_pyglm_amd.inference import batched_hmc, batched_nuts
    fn = batched_hmc.sample_glms_hmc if run is _hmc else batched_nuts.sample_glms_nuts
    kw = dict(n_warmup=40, step_sz=0.05, seed=5, mass='adapt')
    kw.update(dict(n_leapfrog=3) if run is _hmc else dict(max_depth=3))
    long = fn(p, x, 12, **kw)
    assert np.array_equal(one['minv'], long['minv']) and np.array_equal(one['samples'], long['samples'][:4])
    # no window: the bits of mass=None
    a, b = run(p, x, mass='adapt', n_warmup=10), run(p, x, n_warmup=10)
    assert a['adapt_windows'] == [] and np.all(a['minv'] == 1.0)
    for k in KEYS[:3]:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('run', [_hmc, _nuts])
@pytest.mark.parametrize('mass', [None, 'array', 'adapt'])
def test_chains_equal_single_chain_runs(popn, run, mass):
    """n_chains = 3 over the neurons [1, 4) (M = 3, R = 9): chain c is the single-chain run with chain_seed(seed, c)."""
    p, x = popn
    P = p.glm.P
    m = 0.5 + np.random.default_rng(7).random((3, P)) if mass == 'array' else mass
    out = run(p, x, mass=m, n_chains=3, n_lo=1, n_hi=4)
    assert p.last_fit_stats['n_chains'] == 3
    assert out['samples'].shape == (3, 4, 3, P) and out['step_sz'].shape == (3, 3) and out['accept_rate'].shape == (3, 3)
    if mass == 'adapt':
        assert out['minv'].shape == (3, 3, P)
        assert not np.array_equal(out['minv'][0], out['minv'][1])               # every chain learns its own
    for c in range(3):
        one = run(p, x, mass=m, n_lo=1, n_hi=4, seed=MA.chain_seed(5, c))
        for k in KEYS:
            if k in out:
                assert np.array_equal(out[k][c], one[k]), (c, k)
    assert not np.array_equal(out['samples'][0], out['samples'][1])
    from theano_pyglm_amd.inference.batched_hmc import summarize
    s = summarize(out['samples'], chains=True)
    assert s['rhat'].shape == (3, P) and np.all(np.isfinite(s['rhat'])) and s['ess'].shape == (3, P)


@pytest.mark.gpu
def test_jitter_and_dense_mass_with_chains(popn):
    p, x = popn
    P = p.glm.P
    a = _hmc(p, x, n_chains=2, init_jitter=0.01, n_warmup=0, n_lo=0, n_hi=2)
    b = _hmc(p, x, n_chains=2, n_warmup=0, n_lo=0, n_hi=2)
    assert not np.array_equal(a['samples'], b['samples']) and np.all(np.isfinite(a['samples']))
    S = np.tile(0.5 * np.eye(P), (2, 1, 1))
    for run in (_hmc, _nuts):
        out = run(p, x, mass=S, n_chains=2, n_lo=0, n_hi=2, n_warmup=4)
        for c in range(2):
            one = run(p, x, mass=S, n_lo=0, n_hi=2, n_warmup=4, seed=MA.chain_seed(5, c))
            assert np.array_equal(out['samples'][c], one['samples'])


@pytest.mark.gpu
def test_errors(popn):
    from theano_pyglm_amd.inference.batched_ais import ais_glms
    p, x = popn
    for run in (_hmc, _nuts):
        with pytest.raises(ValueError, match="factor_on_device"):
            run(p, x, mass='adapt', factor_on_device=True)
        with pytest.raises(ValueError, match="n_chains"):
            run(p, x, n_chains=0)
    with pytest.raises(ValueError, match="adapt"):
        ais_glms(p, x, n_particles=2, n_temps=6, mass='adapt')
