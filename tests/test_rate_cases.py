"""The rate-window reference without a GPU (tests/rate_reference.py, tests/rate_cases.json): the windows partition the range,
the expected counts add up to the rescaling reference's expected count and the observed ones to the spike count, the case
table holds the data it names, the numpy statement of the fold equals numpy's moments, the pit at win = 1 is the mid-p value
written out by hand, the Poisson terms agree with an independent statement of the law, and the pit of counts drawn from the
model's own Poisson law is uniform."""
import numpy as np
import pytest

from tests import rate_reference as R
from tests import rescale_reference as RR

CASES = R.load_cases()
longdouble = pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps,
                                reason="numpy.longdouble is float64 here")


def test_windows_partition_the_range():
    for n in (1, 7, 255, 256, 257, 933, 1003):
        for win in (1, 7, 10, 50, 256, 300, 933, 10000):
            st = R.window_starts(n, win)
            ends = np.minimum(st + win, n)
            assert st[0] == 0 and ends[-1] == n and np.array_equal(st[1:], ends[:-1])
            assert len(st) == R.n_windows(n, win) == R.lib().rw_windows(n, win)
            assert np.all(ends - st >= 1) and np.all((ends - st)[:-1] == win)


def test_case_table_is_well_formed_and_holds_what_it_names():
    assert len(set(c['name'] for c in CASES)) == len(CASES)
    assert set(c['kind'] for c in CASES) == {'explinear', 'exp'} and any(c['Dstim'] > 0 for c in CASES)
    assert set(c['N'] for c in CASES) >= {3, 17}
    wins = set(w for c in CASES for w in c['wins'])
    assert wins >= {1, 7, 256, 300, 10000}
    off16 = short_piece = False
    for c in CASES:
        p = R.problem(c)
        assert p.S[:, c['silent']].sum() == 0 and p.S.max() >= 2, c['name']
        assert c['nT'] * c['N'] <= 1100 * 17                                    # (quick on the device)
        for t_lo, t_hi in R.ranges(c):
            assert 0 <= t_lo < t_hi <= c['nT'] and t_lo % 16 == 0              # (pgl_set_time_range takes no other t_lo)
            n = t_hi - t_lo
            off16 |= t_lo % 256 != 0 and any((t_lo + w) % 16 != 0 for w in c['wins'])   # windows start off the 16-bin grid
            short_piece |= any(w > 256 and 0 < (n % w) % 256 for w in c['wins'])
            assert any(n % w != 0 for w in c['wins']) and any(w >= n for w in c['wins']) or len(c['wins']) < 5
    assert off16 and short_piece
    # an event in the first and in the last bin of a window, a bin holding two spikes, an event right behind t_hi
    c = CASES[0]
    S = R.problem(c).S
    assert S[83, 2] and S[89, 2] and (83 - 48) % 7 == 0 and S[347, 2] and S[348, 2] and (348 - 48) % 300 == 0
    assert S[0, 2] and S[1002, 2] and S[299, 1] == 2 and S[980, 1] and S[981, 1]


@longdouble
def test_counts_add_up_to_the_rescaling_reference_and_the_spike_count():
    """sum_w Lam = the expected count of tests/rescale_reference.reference (the same longdouble rates, one sum over the
    range), sum_w obs = the spikes of the range, for every window length"""
    for c in RR.load_cases()[:4]:
        p = RR.problem(c)
        for t_lo, t_hi, _ in RR.ranges(c):
            want = RR.reference(c, t_lo, t_hi)[1][:, 0]
            for win in (1, 7, 50, 256, 300, 10 ** 6):
                Lam, obs = R.counts(RR.currents(c, t_lo, t_hi), p.S[t_lo:t_hi], p.kind, p.dt, win)
                assert Lam.shape == obs.shape == (R.n_windows(t_hi - t_lo, win), p.N)
                assert np.all(np.abs(Lam.sum(axis=0) - want) <= 1e-13 * want), (c['name'], win)
                assert np.array_equal(obs.sum(axis=0), p.S[t_lo:t_hi].sum(axis=0))


@longdouble
def test_pieced_order_meets_the_bound():
    """the header's order (tests/csrc/ratewin_host.c: pieces of 256 bins from the window's own start) on float64 rates stays
    inside the GPU test's bound of the plain longdouble sums"""
    for c in CASES:
        p = R.problem(c)
        x = R.currents_of(p, p.theta)
        lam64 = np.asarray(RR.rate_longdouble(x, p.kind), dtype=np.float64)
        for t_lo, t_hi in R.ranges(c):
            for win in c['wins']:
                ref_Lam, ref_obs = R.reference(c, t_lo, t_hi, win)
                got = [R.host_counts(lam64[t_lo:t_hi, n], p.S[t_lo:t_hi, n], win, p.dt) for n in range(p.N)]
                Lam = np.array([g[0] for g in got]).T
                assert np.array_equal(np.array([g[1] for g in got]).T, ref_obs)
                r = R.ratio(Lam, ref_Lam)
                print("%-14s [%4d, %4d) win %5d: pieced float64 sums %.2e of the bound" % (c['name'], t_lo, t_hi, win, r))
                assert r <= 1.0


def test_fold_is_numpys_moments():
    rng = np.random.default_rng(3)
    S = 40
    mu = np.exp(rng.uniform(-3.0, 5.0, size=(4, 3)))
    lam = mu[None] * np.exp(0.2 * rng.standard_normal((S, 4, 3)))
    y = rng.poisson(mu).astype(float)
    acc = R.fold_numpy(lam, y)
    assert np.all(np.abs(acc[0] - lam.mean(axis=0)) <= 1e-14 * lam.mean(axis=0))
    var = lam.var(axis=0, ddof=1)
    assert np.all(np.abs(acc[1] / (S - 1.0) - var) <= 1e-12 * var)
    assert np.array_equal(acc[2], lam.min(axis=0)) and np.array_equal(acc[3], lam.max(axis=0))
    u = np.array([R.midp(lam[s], y) for s in range(S)])
    assert np.all(np.abs(acc[4] - u.mean(axis=0)) <= 1e-14)


def test_pit_of_one_bin_is_the_midp_value_by_hand():
    """win = 1: y is 0, 1 or 2 and u = 0.5 e^-L,  e^-L (1 + L / 2),  e^-L (1 + L + L^2 / 4)"""
    rng = np.random.default_rng(8)
    L = np.exp(rng.uniform(-7.0, 0.5, size=(6, 30)))
    y = np.resize(np.array([0.0, 1.0, 0.0, 2.0, 0.0]), 30)
    e = np.exp(-L)
    hand = np.where(y == 0, 0.5 * e, np.where(y == 1, e * (1.0 + 0.5 * L), e * (1.0 + L + 0.25 * L * L)))
    acc = R.fold_numpy(L, y)
    assert np.all(np.abs(acc[4] - hand.mean(axis=0)) <= 1e-15)
    assert R.midp(0.0, 0.0) == 0.5 and R.midp(0.0, 3.0) == 1.0


def test_poisson_terms_against_an_independent_statement():
    for lam in (1e-3, 0.5, 3.0, 40.0, 250.0, 699.0):
        term, ref = R.poisson_pmf_check(lam, 1024)
        ok = ref > 1e-290
        assert np.all(np.abs(term[ok] - ref[ok]) <= 1e-11 * ref[ok]), lam
        assert abs(term.sum() - 1.0) <= 1e-12


def test_pit_of_the_models_own_counts_is_uniform():
    """counts drawn from Poisson(Lam) with Lam spread over [50, 400]: the atoms of the mid-p values (~ 1 / sqrt(2 pi Lam) <
    0.06 each, at different places for different Lam) smear out, and the KS distance of n = 1000 values stays under the 1 %
    band 1.628 / sqrt(n); the same counts against means 10 % too high leave it"""
    rng = np.random.default_rng(2025)
    n = 1000
    Lam = rng.uniform(50.0, 400.0, size=n)
    y = rng.poisson(Lam).astype(float)
    band = 1.628 / np.sqrt(n)
    d = R.ks_uniform(R.midp(Lam, y))
    d_bad = R.ks_uniform(R.midp(1.1 * Lam, y))
    print("KS distance %.4f (band %.4f); with means 10 %% too high %.4f" % (d, band, d_bad))
    assert d <= band < d_bad
    from theano_pyglm_amd.inference import predictive as PP
    assert PP.ks_uniform(R.midp(Lam, y)) == pytest.approx(d, abs=1e-15)
