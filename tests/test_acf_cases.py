"""The case table of the independence rule (tests/acf_cases.json) and the longdouble reference (tests/acf_reference.py) judged
on their own, without a GPU: the reference's normal quantile against mpmath, every case reaches the branch it names, the checks
of the other ACF tests reject emulated defects, and the statistical claims of the test on the reference alone."""
import numpy as np
import pytest

from tests import acf_reference as AR

LD = AR.LD
needs_ld = pytest.mark.skipif(not AR.LD_IS_WIDER, reason="numpy.longdouble is float64 here")


@needs_ld
def test_reference_quantile_against_mpmath():
    import mpmath as mp
    mp.mp.dps = 360                                                  # 2 p - 1 at p = DBL_MIN keeps 50 digits of p
    ps = [AR.DBL_MIN, 1e-300, 1e-200, 1e-100, 1e-50, 1e-30, 1e-20, 1e-16, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3,
          0.01, 0.02, 0.05, 0.074, 0.075, 0.076, 0.1, 0.2, 0.3, 0.4, 0.45, 0.49, 0.499, 0.4999999, 0.5000001, 0.501, 0.51, 0.55,
          0.6, 0.7, 0.8, 0.9, 0.924, 0.925, 0.926, 0.95, 0.99, 0.999, 1 - 1e-6, 1 - 1e-9, 1 - 1e-12, 1 - 2.0 ** -40, 1 - 2.0 ** -53]
    assert len(ps) == 50
    worst = 0.0
    for p in ps:
        exact = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1)
        got = mp.mpf(float(AR.quantile(p))) + mp.mpf(float(AR.quantile(p) - LD(float(AR.quantile(p)))))
        worst = max(worst, float(abs(got - exact) / abs(exact)))
        # the upper tail entered with its own probability mirrors the lower one
        assert AR.quantile(upper=p) == -AR.quantile(p)
    print("reference quantile: worst relative error %.2e" % worst)
    assert worst <= 1e-15


def test_every_case_reaches_its_branch():
    names = set()
    for c in AR.load():
        tau, runs, L, want = AR.case_tau(c), c['runs'], c['L'], set(c['expect'])
        n = tau.size
        names |= want
        assert n == sum(runs)
        br = set(AR.branch(tau[~np.isnan(tau)]))
        if 'tail' in want:
            assert {'tail', 'central'} <= br
        if 'clamp' in want:
            assert 'clamp' in br and np.any(tau == 0.0) and np.any(np.isinf(tau)) and np.any((tau > 0) & (tau < AR.DBL_MIN))
        if 'piece_edge' in want:
            assert n >= AR.PIECE                                     # pairs that straddle a piece edge exist
        if 'many_tiles' in want:
            assert n > 8 * AR.PIECE * 32
        if 'cross_run' in want:
            assert sum(1 for l in runs if l > 0) >= 2
            assert np.any(AR.pair_counts(runs, L) < np.maximum(n - np.arange(1, L + 1), 0))
        if 'empty_run' in want:
            assert 0 in runs and 1 in runs and any(1 < l < L for l in runs)
        if 'lag_ge_n' in want:
            assert np.any(AR.pair_counts(runs, L) == 0) and n >= 3
        if 'void_n' in want:
            assert n < 3
        if 'void_tau' in want:
            assert np.any(~(tau >= 0.0))
        if 'void_c0' in want:
            assert n >= 3 and n & (n - 1) == 0 and np.all(tau == tau[0])
    assert names == {'tail', 'clamp', 'piece_edge', 'many_tiles', 'cross_run', 'empty_run', 'lag_ge_n', 'void_n', 'void_tau', 'void_c0'}
    lens = sorted(sum(c['runs']) for c in AR.load())
    assert set([0, 1, 2, 3, 255, 256, 257, 513, 70000]) <= set(lens)
    assert set(c['L'] for c in AR.load()) >= {1, 20, 64}
    # a run boundary exactly on a multiple of the piece, and one element to either side
    assert {c['runs'][0] for c in AR.load() if c['name'].startswith('edge')} == {255, 256, 257}


# ---- emulated defects -------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c in one rounding: math.fma where Python has it, else exact rational arithmetic rounded once"""
    import math
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _variant(g, runs, L, cross=False, piece_from_run=False, nk_simple=False, fma=False):
    """the rule in plain Python doubles with one defect switched on -> (NHEAD + L)"""
    n = g.size
    end = AR.run_ends(runs)
    start = np.concatenate([np.full(int(l), int(e - l)) for l, e in zip(runs, np.cumsum(runs))])
    out = np.full(AR.NHEAD + L, np.nan)

    def piece_sum(pairs):                                            # pairs: (i, a, b) terms a * b of index i, ascending
        tot, s, cur = 0.0, 0.0, None
        for i, a, b in pairs:
            p = ((i - start[i]) // AR.PIECE, start[i]) if piece_from_run else i // AR.PIECE
            if p != cur:
                if cur is not None:
                    tot += s
                s, cur = 0.0, p
            s = _fma(a, b, s) if fma else s + a * b
        return tot + s if cur is not None else 0.0
    mean = piece_sum((i, g[i], 1.0) for i in range(n)) / n
    d = g - mean
    c0 = piece_sum((i, d[i], d[i]) for i in range(n))
    out[:3] = n, mean, c0
    Q, dof = 0.0, 0
    for k in range(1, L + 1):
        idx = [i for i in range(n - k) if cross or i + k < end[i]]
        nk = (n - k) if nk_simple else len(idx)
        if nk < 1:
            continue
        r = piece_sum((i, d[i], d[i + k]) for i in idx) / c0
        Q += r * r / (nk / (float(n) * (n + 2.0)))
        dof += 1
        out[AR.NHEAD + k - 1] = r
    out[3], out[4], out[5] = Q, dof, 0.0
    return out


def _case(name):
    c = [c for c in AR.load() if c['name'] == name][0]
    return c, AR.case_tau(c)


@needs_ld
def test_the_checks_reject_emulated_defects():
    from theano_pyglm_amd.inference import gof
    # the plain variant is the rule: the bits of gof.acf_from_scores
    for name in ('runs3_short', 'edge255', 'ar1'):
        c, tau = _case(name)
        g = gof.normal_scores(tau)
        good = gof.acf_from_scores([AR.split_runs(g, c['runs'])], c['L'])[0]
        assert _variant(g, c['runs'], c['L']).tobytes() == good.tobytes(), name
        # bit checks: an FMA-contracted sum, a piece grid that starts at the run
        assert _variant(g, c['runs'], c['L'], fma=True).tobytes() != good.tobytes(), name
        if name != 'ar1':
            assert _variant(g, c['runs'], c['L'], piece_from_run=True).tobytes() != good.tobytes(), name
        # tolerance checks: pairs across a run boundary, n - k for n_k
        if name != 'ar1':
            ref = AR.reference(tau, c['runs'], c['L']).astype(float)
            bad = _variant(g, c['runs'], c['L'], cross=True)
            assert np.nanmax(np.abs(bad[AR.NHEAD:] - ref[AR.NHEAD:])) > 1e3 * AR.R_TOL, name
            bad = _variant(g, c['runs'], c['L'], nk_simple=True)
            assert abs(bad[3] - ref[3]) > 1e3 * AR.Q_RTOL * ref[3], name
    # 1 - z for the upper tail: tau = 40 loses its score (1 - z = 0 exactly), tau = 30 most of its digits
    for tau in (30.0, 40.0):
        z = -np.expm1(-tau)
        with np.errstate(all='ignore'):
            wrong = float(AR.ppnd_tail(np.array([max(1.0 - z, AR.DBL_MIN)], dtype=LD))[0])
        right = float(AR.scores(np.array([tau]))[0])
        assert abs(wrong - right) > 1e3 * AR.SCORE_RTOL * abs(right), tau


# ---- statistics of the reference alone --------------------------------------------------------------------------------------
def _pvalue(out):
    from scipy import special
    return special.gammaincc(float(out[4]) / 2.0, float(out[3]) / 2.0)


IID_SEED = 1000


@needs_ld
def test_iid_intervals_are_rejected_at_the_nominal_rate():
    """200 iid Exp(1) samples of n = 2000 at L = 20: the share of p < 0.05 within binomial 3 sigma of 0.05"""
    rej = 0
    for s in range(200):
        tau = np.random.default_rng(IID_SEED + s).exponential(size=2000)
        rej += _pvalue(AR.reference(tau, [2000], 20)) < 0.05
    print("rejection share %.3f" % (rej / 200.0))
    assert 0.005 <= rej / 200.0 <= 0.10


@needs_ld
def test_copula_ar1_is_found_in_every_seed():
    for s in range(20):
        tau = AR.copula_ar1(np.random.default_rng(2000 + s), 2000, 0.3)
        out = AR.reference(tau, [2000], 20)
        assert abs(float(out[AR.NHEAD]) - 0.3) <= 0.085, (s, float(out[AR.NHEAD]))
        assert _pvalue(out) < 0.05, s


@pytest.mark.parametrize('n', [2, 3, 7, 100, 1001, 20000])
def test_ks_pvalue_equals_scipy(n):
    from scipy import stats
    from theano_pyglm_amd.inference import gof
    assert hasattr(stats, 'kstwo')                                   # the exact law: what the README says this build has
    rng = np.random.default_rng(1000 + n)
    for z in (rng.random(n), -np.expm1(-rng.exponential(size=n)), -np.expm1(-1.7 * rng.exponential(size=n)),
              np.full(n, 0.25)):
        res = stats.kstest(z, 'uniform', method='exact')
        p = float(gof.ks_pvalue(gof.ks_uniform(z), n))
        assert abs(p - res.pvalue) <= 1e-12, (n, p, res.pvalue)
    assert np.isnan(gof.ks_pvalue(np.nan, 5)) and np.isnan(gof.ks_pvalue(0.3, 0))
