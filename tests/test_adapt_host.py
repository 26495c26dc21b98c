"""CPU tests of the warm-up mass adaptation and the chain helpers: the schedule, csrc/pglm_adapt.h through
tests/csrc/adapt_host.c (tests/adapt_mirror.py), split-R-hat and the chains' seeds.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import adapt_mirror as AM
from tests import hmc_mirror as HM
from tests import nuts_mirror as NM
from theano_pyglm_amd.inference import mass_adapt as MA


# ---- schedule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 19, 20, 100, 149, 150, 151, 300, 1000])
def test_schedule_tiles_and_doubles(n):
    w = MA.adapt_windows(n)
    if n < 20:
        assert w == []
        return
    init, term = (75, 50) if n >= 150 else (int(0.15 * n), int(0.10 * n))
    base = 25 if n >= 150 else n - init - term
    assert w[0][0] == init and w[-1][1] == n - term
    assert all(a[1] == b[0] for a, b in zip(w[:-1], w[1:]))                    # no gap, no overlap
    sizes = [e - s for s, e in w]
    assert all(s > 0 for s in sizes)
    assert sizes[:-1] == [base * 2 ** k for k in range(len(w) - 1)]            # doubling until the stretch
    assert sizes[-1] >= base * 2 ** (len(w) - 1)                               # the last one is stretched, never cut
    assert sizes[-1] < base * 2 ** (len(w) - 1) + 2 * base * 2 ** (len(w) - 1) + 1   # ... by less than its successor's size
    ints = MA.schedule_ints(w)
    assert ints.dtype == np.int32 and list(ints) == [len(w), init] + [e for _, e in w]


def test_schedule_examples():
    assert MA.adapt_windows(300) == [(75, 100), (100, 250)]                    # (the last window has 150 draws)
    assert MA.adapt_windows(1000) == [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]
    assert MA.adapt_windows(20) == [(3, 18)]
    assert list(MA.schedule_ints([])) == [0, 0]


# ---- Welford, shrinkage ------------------------------------------------------------------------------------------
def _window(L, col):
    mean, m2 = C.c_double(0.0), C.c_double(0.0)
    for k, v in enumerate(col):
        L.adapt_welford(float(v), float(k + 1), C.byref(mean), C.byref(m2))
    return mean.value, m2.value


def test_welford_against_numpy():
    L = AM.lib()
    rng = np.random.default_rng(3)
    n = 40
    for scale in 10.0 ** np.arange(-6, 7):
        col = scale * (3.0 + rng.standard_normal(n))
        mean, m2 = _window(L, col)
        assert abs(mean - col.mean()) <= 1e-13 * abs(col.mean())
        var = np.var(col, ddof=1)
        assert abs(m2 / (n - 1) - var) <= 1e-13 * var
        assert L.adapt_minv(m2, float(n)) == (n / (n + 5.0)) * (m2 / (n - 1.0)) + 1e-3 * (5.0 / (n + 5.0))
    mean, m2 = _window(L, np.full(n, 0.7))
    assert m2 == 0.0 and L.adapt_minv(m2, float(n)) == 1e-3 * (5.0 / (n + 5.0))
    col = rng.standard_normal(n)
    col[7] = np.nan
    assert L.adapt_minv(_window(L, col)[1], float(n)) == 1.0
    assert L.adapt_minv(np.inf, float(n)) == 1.0


def test_row_machine_through_two_windows():
    """adapt_hmc_step on a state whose q the test writes: counts, the window index, minv at the ends, zeroed accumulators."""
    L = AM.lib()
    R, P, n_warm = 2, 3, 300
    rng = np.random.default_rng(5)
    st = np.zeros(4 * R * P + 10 * R)
    q, sc = st[:R * P].reshape(R, P), st[4 * R * P:].reshape(10, R)
    ad = AM.Adapt(R, P, n_warm)
    pts = rng.standard_normal((n_warm + 5, R, P)) * np.array([1e-3, 1.0, 1e3])
    pts[120:130, 1] = pts[119, 1]                                               # (a run of rejections repeats the point)
    for t in range(n_warm + 5):
        q[:] = pts[t]
        sc[HM.SC['t']] = t + 1
        sc[HM.SC['avg_accept']] = 0.5
        before = ad.minv.copy()
        L.adapt_hmc_step(AM._p(st), R, P, AM._p(ad.st), AM._p(ad.sched), AM._p(ad.minv))
        ends = [e for _, e in ad.windows]
        if t + 1 in ends:
            s, e = ad.windows[ends.index(t + 1)]
            n = e - s
            want = (n / (n + 5.0)) * pts[s:e].var(axis=0, ddof=1) + 1e-3 * 5.0 / (n + 5.0)
            assert np.allclose(ad.minv, want, rtol=1e-12, atol=0.0)
            assert np.all(ad.mean == 0.0) and np.all(ad.m2 == 0.0) and np.all(ad.count == 0.0)
            assert np.all(ad.widx == ends.index(t + 1) + 1)
            assert np.all(sc[HM.SC['avg_accept']] == 0.9)                       # the restart
        else:
            assert np.array_equal(ad.minv, before)
            assert np.all(sc[HM.SC['avg_accept']] == 0.5)
            inside = 75 <= t < 250
            assert np.all(ad.count == ((t - (75 if t < 100 else 100) + 1) if inside else 0.0))
    assert np.all(ad.widx == 2)


# ---- restart rules -----------------------------------------------------------------------------------------------
def test_restart_equals_fresh_state():
    L = AM.lib()
    f, g = np.zeros(10), np.zeros(10)
    L.adapt_fresh_hmc(AM._p(f), 0.37)
    g[:] = f
    g[HM.SC['avg_accept']] = 0.123
    L.adapt_restart_hmc(AM._p(g))
    assert np.array_equal(f, g) and g[HM.SC['step']] == 0.37
    f, g = np.zeros(30), np.zeros(30)
    L.adapt_fresh_nuts(AM._p(f), 0.37)                                          # mu = log(10 * 0.37), hbar = log eps bar = 0
    g[:] = f
    for name in ('hbar', 'logeps_bar', 'mu'):
        g[NM.SC[name]] = 7.0
    L.adapt_restart_nuts(AM._p(g))
    assert np.array_equal(f, g) and g[NM.SC['mu']] == np.log(10.0 * 0.37)


# ---- recovery of a Gaussian's scales -----------------------------------------------------------------------------
SIGMA = 10.0 ** np.linspace(-2.0, 2.0, 24)


def _gauss(X):
    return -0.5 * np.sum((X / SIGMA) ** 2, axis=1), -X / SIGMA ** 2


def test_nuts_recovers_the_scales():
    """NUTS on an independent Gaussian with sd 1e-2 .. 1e2, n_warmup = 300 (windows (75, 100), (100, 250): the last has 150
    draws).  Every final minv_j / sigma_j^2 within [1/2, 2]; the frozen step within a factor 3 of the exact-mass chain's."""
    X0 = SIGMA[None, :] * np.array([NM.lib().nuts_normal(99, 0, 0, j) for j in range(24)])[None, :]
    kw = dict(max_depth=8, step0=0.01, seed=1, delta=0.8)
    m = AM.NutsMirror(_gauss, X0, 10, 300, **kw)
    m.run()
    ratio = m.minv[0] / SIGMA ** 2
    exact = NM.Mirror(_gauss, X0, 10, n_warmup=300, minv=(SIGMA ** 2)[None, :], **kw)
    exact.run()
    step, step_exact = m.sc[NM.SC['step'], 0], exact.sc[NM.SC['step'], 0]
    print("minv / sigma^2: min %.3f max %.3f; step %.4f against %.4f under the exact mass" % (ratio.min(), ratio.max(), step,
                                                                                               step_exact))
    assert np.all(ratio > 0.5) and np.all(ratio < 2.0)
    assert step_exact / 3.0 < step < step_exact * 3.0
    assert np.all(m.ad.widx == 2) and np.all(m.ad.count == 0.0)
    # the kept draws were made under the final mass only: minv at the ends of the kept transitions never changes
    kept = m.log[0][300:]
    assert len(kept) == 10 and all(np.array_equal(k['minv'], m.minv[0]) for k in kept)


def test_short_warmup_is_the_unadapted_chain():
    X0 = np.array([[0.3, -0.2, 0.1], [0.1, 0.0, -0.4]])
    sig = np.array([0.5, 1.0, 2.0])

    def tgt(X):
        return -0.5 * np.sum((X / sig) ** 2, axis=1), -X / sig ** 2
    a = AM.NutsMirror(tgt, X0, 6, 19, max_depth=5, step0=0.3, seed=4)
    b = NM.Mirror(tgt, X0, 6, n_warmup=19, max_depth=5, step0=0.3, seed=4)
    a.run(), b.run()
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.sc, b.sc) and np.all(a.minv == 1.0)
    h = AM.HmcMirror(tgt, X0, 19, step0=0.3, seed=4)
    g = HM.Mirror(tgt, X0, step0=0.3, seed=4)
    sh, sg = h.run(30, 4), g.run(30, 4, 19)
    assert np.array_equal(sh[0], sg[0]) and np.array_equal(h.sc, g.sc)


def test_hmc_mirror_adapts():
    """The HMC chain under mass='adapt' on a Gaussian with sd 0.1, 1, 10: the scales' order is recovered and the decisions
    after a window's end run under the new mass (H0 of the next transition uses it)."""
    sig = np.array([0.1, 1.0, 10.0])

    def tgt(X):
        return -0.5 * np.sum((X / sig) ** 2, axis=1), -X / sig ** 2
    h = AM.HmcMirror(tgt, np.zeros((1, 3)), 300, step0=0.05, seed=2)
    h.run(310, 10)
    ratio = h.minv[0] / sig ** 2
    print("HMC minv / sigma^2", ratio)
    assert h.minv[0, 0] < h.minv[0, 1] < h.minv[0, 2]
    assert np.all(h.ad.widx == 2)


# ---- R-hat -------------------------------------------------------------------------------------------------------
def test_rhat():
    rng = np.random.default_rng(11)
    s = rng.standard_normal((4, 500, 3))
    r = MA.rhat(s)
    assert r.shape == (3,) and np.all(np.abs(r - 1.0) < 0.02)
    s2 = s.copy()
    s2[2] += 2.0
    assert np.all(MA.rhat(s2) > 1.3)
    s3 = s.copy()
    s3[1] += np.linspace(-2.0, 2.0, 500)[:, None]                               # a trend: only the split sees it
    assert np.all(MA.rhat(s3) > 1.1)
    one = MA.rhat(s3[1:2])
    assert np.all(one > 1.1)                                                    # (a single chain: its two halves)
    with pytest.raises(ValueError):
        MA.rhat(np.zeros((2, 3)))


def test_summarize_with_chains():
    from theano_pyglm_amd.inference.batched_hmc import summarize
    rng = np.random.default_rng(13)
    s = rng.standard_normal((3, 200, 2, 4))
    out = summarize(s, chains=True)
    assert out['rhat'].shape == (2, 4) and out['mean'].shape == (2, 4) and out['ess'].shape == (2, 4)
    assert np.all(np.abs(out['rhat'] - 1.0) < 0.05)
    assert np.all(out['ess'] > 300.0)                                           # pooled over the chains: about 3 x 200
    assert np.allclose(out['mean'], s.reshape(600, 2, 4).mean(axis=0))
    single = summarize(s[0])
    assert 'rhat' not in single and single['ess'].shape == (2, 4)


# ---- seeds -------------------------------------------------------------------------------------------------------
def test_chain_seed():
    L = AM.lib()
    seen = set()
    for s in list(range(10)) + [2 ** 63 + 5, 2 ** 64 - 1]:
        assert MA.chain_seed(s, 0) == s
        for c in range(100):
            v = MA.chain_seed(s, c)
            assert v == L.adapt_chain_seed(s, c)
            seen.add(v)
    assert len(set(MA.chain_seed(s, c) for s in range(40) for c in range(25))) == 1000
    z = MA.start_jitter(7, 3, 50)
    assert z.shape == (50,) and np.all(np.isfinite(z)) and abs(z.mean()) < 0.5 and 0.6 < z.std() < 1.4
    zc = np.array([NM.lib().nuts_normal(7, 3, 2 ** 64 - 1, j) for j in range(50)])
    assert np.allclose(z, zc, rtol=1e-12, atol=1e-15)                           # (the chains' generator under the key of t = 2^64 - 1)
