"""Convergence diagnostics without a GPU: the longdouble reference of tests/diag_reference.py keeps every case of its table
(no discontinuous decision closer to its threshold than the floor) and the cases reach what they name; the float64 numpy
statement of inference/diagnostics.py against the reference gives the error scale e0 recorded there; the host build of
csrc/pglm_diag.h meets the bounds; Phi^-1 against mpmath; rhat_plain against mass_adapt.rhat; the AR(1) law of the ESS; the
bounds reject five emulated defects."""
import os
import re

import numpy as np
import pytest

from tests import diag_reference as R
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import diagnostics as D
from theano_pyglm_amd.inference.mass_adapt import rhat as plain_rhat

IDS = [c['name'] for c in R.CASES]


def _case(name):
    return [c for c in R.CASES if c['name'] == name][0]


def _rows(d):
    return np.stack([np.asarray(d[k], dtype=float).reshape(-1) for k in R.ROWS])


def _row(ref, name):
    return np.asarray(ref[R.ROWS.index(name)], dtype=float)


@pytest.mark.parametrize('c', R.CASES, ids=IDS)
def test_reference_keeps_the_case(c):
    x, ref, margin = R.case_reference(c)
    print(c['name'], "smallest margin", margin)
    assert x.shape == (c['C'], c['n'], c['K']) and margin > R.MARGIN_FLOOR


def test_cases_reach_what_they_name():
    S = sorted(set(c['C'] * c['n'] for c in R.CASES))
    for want in (255, 256, 257, 1023, 1024, 1025, R.MAX_DRAWS):
        assert want in S
    assert set((8, 9, 15, 16, 511, 512, 513, 1000)) <= set(c['n'] for c in R.CASES)
    assert set((1, 2, 3, 4, 8)) <= set(c['C'] for c in R.CASES) and set((1, 3, 161)) <= set(c['K'] for c in R.CASES)
    assert set((255, 256, 257)) <= set(c['n'] // 2 for c in R.CASES)
    ref = dict((c['name'], R.case_reference(c)[1]) for c in R.CASES)
    assert np.all(_row(ref['ar99'], 'lag_mean') >= 100)                                       # truncates late
    n_s = 4 * 200
    assert np.all(_row(ref['arm90'], 'ess_mean') > n_s)                                       # antithetic: above S
    assert np.any(np.isclose(_row(ref['arm90'], 'ess_mean'), n_s * np.log10(n_s), rtol=1e-12))   # and at the cap
    assert np.all(_row(ref['shifted'], 'rhat') > 1.5)
    assert np.all(_row(ref['wide_chain'], 'rhat') > 1.1) and np.all(_row(ref['wide_chain'], 'rhat_plain') < 1.05)
    x = R.case_reference(_case('integers'))[0]
    assert len(np.unique(x)) < 30                                                             # heavy ties
    assert np.all(_row(ref['two_valued'], 'ess_tail') == 0)              # I(x <= q95) is 1 everywhere: a constant series
    k = ref['constant'].astype(float)
    assert np.all(k[[0, 2, 3, 4]] == 2.75) and np.all(k[[1, 7, 8, 9, 11, 12, 13, 14]] == 0) and np.all(np.isnan(k[[5, 6, 10]]))
    w = ref['const_in_halves'].astype(float)
    assert np.all(np.isinf(w[5])) and np.all(np.isinf(w[6])) and np.all(w[14] == 6) and np.allclose(w[9], 40.0 / 12.0)   # N / (2 T)
    nf = ref['nonfinite'].astype(float)
    assert np.isnan(nf).all(axis=0).sum() == 9 and np.isfinite(nf).all(axis=0).sum() == 3


def test_constants_agree():
    src = open(os.path.join(R.ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_diag.h')).read()
    pub = open(os.path.join(R.ROOT, 'include', 'pyglm_hip.h')).read()
    for text in (src, pub):
        assert int(re.search(r'#define PGL_DIAG_MAX_DRAWS (\d+)', text).group(1)) == R.MAX_DRAWS == _lib.DIAG_MAX_DRAWS >= 4096
        assert int(re.search(r'#define PGL_DIAG_NOUT (\d+)', text).group(1)) == len(R.ROWS) == _lib.DIAG_NOUT
    assert R.lib().diag_max_draws() == R.MAX_DRAWS and R.lib().diag_rows() == _lib.DIAG_NOUT
    assert _lib.DIAG_ROWS == R.ROWS
    for i, name in enumerate(R.ROWS):
        assert re.search(r'#define PGL_DIAG_%s %d\b' % (name.upper(), i), src), name
    for s in ('pgl_chain_diag_dev', 'pgl_chain_diag'):
        assert s in _lib.SYMBOLS
    assert _lib.ABI_VERSION >= 112


def _worst(fn):
    worst = dict((q, 0.0) for q in R.SUMS + R.COMPOSED)
    ratio = dict(worst)
    for c in R.CASES:
        x, ref, _ = R.case_reference(c)
        got = fn(x)
        e = R.errors(got, ref)
        r = R.ratios(got, ref, x)
        for q in worst:
            worst[q] = max(worst[q], e[q])
            ratio[q] = max(ratio[q], r[q])
    return worst, ratio


def test_error_scale():
    """e0: the float64 statement against the longdouble reference over the whole table, within the recorded constants"""
    worst, ratio = _worst(lambda x: _rows(D.chain_diagnostics(x)))
    print("e0 measured %s, recorded %s" % (worst, R.E0))
    for q in R.COMPOSED:
        assert worst[q] <= R.E0[q] * 1.05, (q, worst[q])
        assert R.BOUND[q] == 100.0 * R.E0[q]
    for q in R.SUMS:
        assert ratio[q] <= 1.0, (q, ratio[q])


def test_host_mirror_meets_the_bounds():
    worst, ratio = _worst(R.host_mirror)
    print("host mirror: worst %s, ratio to the bounds %s" % (worst, ratio))
    assert all(r <= 1.0 for r in ratio.values()), ratio
    for c in (_case('ar50'), _case('nonfinite')):
        x = R.case_reference(c)[0]
        assert np.array_equal(R.host_mirror(x, pad=3), R.host_mirror(x), equal_nan=True)       # NaN padding is never read


def test_normal_score_against_mpmath():
    import mpmath
    mpmath.mp.dps = 40
    worst = 0.0
    for S in (8, R.MAX_DRAWS):
        rs = np.arange(1, S + 1, dtype=float) if S == 8 else np.concatenate([np.arange(1, 40), np.arange(1.5, 40), np.linspace(41, S - 41, 97).round(),
                                                                            S + 1 - np.arange(1, 40), [(S + 1) / 2.0]])
        for r in rs:
            p = (mpmath.mpf(r) - mpmath.mpf(3) / 8) / (mpmath.mpf(S) + mpmath.mpf(1) / 4)
            want = mpmath.sqrt(2) * mpmath.erfinv(2 * p - 1)
            for got in (R.lib().diag_score(float(r), float(S)), float(D.normal_score(np.array([r]), S)[0])):
                err = abs(mpmath.mpf(got) - want) / max(abs(want), mpmath.mpf(1e-300)) if want != 0 else abs(got)
                worst = max(worst, float(err))
    # both tails, far out: the lowest and highest rank among 10^12 (outside any S the kernel takes; the routine's third branch)
    for r, S in ((1.0, 1e12), (1e12, 1e12)):
        p = (mpmath.mpf(r) - mpmath.mpf(3) / 8) / (mpmath.mpf(S) + mpmath.mpf(1) / 4)
        want = mpmath.sqrt(2) * mpmath.erfinv(2 * p - 1)
        worst = max(worst, float(abs(mpmath.mpf(R.lib().diag_score(r, S)) - want) / abs(want)))
    print("Phi^-1: worst relative error", worst)
    # the bound, from the routine's own arithmetic: AS 241's approximation error 1e-16, one rounding in the argument, at most 14 in
    # each of the two seven-step Horner sums (all terms positive), one each in the product and the quotient: 31 roundings
    assert worst < 1e-16 + 31 * 2.0 ** -53
    assert R.lib().diag_score(3.0, 8.0) == -R.lib().diag_score(6.0, 8.0) and R.lib().diag_score(4.5, 8.0) == 0.0


def test_rhat_plain_is_mass_adapt_rhat():
    for name in ('n9', 'n513', 'C8', 'shifted', 'const_in_halves'):
        x = R.case_reference(_case(name))[0]
        with np.errstate(all='ignore'):
            want = plain_rhat(x)
        for got in (D.chain_diagnostics(x)['rhat_plain'], R.host_mirror(x)[5]):
            assert np.allclose(got, want, rtol=1e-13, atol=0, equal_nan=True), name


def test_quantiles_are_numpy_percentile():
    for name in ('S255', 'S256', 'n1000', 'integers'):
        x = R.case_reference(_case(name))[0]
        d = D.chain_diagnostics(x)
        lo, med, hi = np.percentile(x.reshape(-1, x.shape[2]), [2.5, 50.0, 97.5], axis=0)
        for got, want in ((d['q025'], lo), (d['median'], med), (d['q975'], hi)):
            assert np.allclose(got, want, rtol=1e-14, atol=1e-15)


def test_ess_follows_the_ar1_law():
    """ESS / S of an AR(1) chain tends to (1 - rho) / (1 + rho) = 1 / tau.  K = 40 independent columns of 4 x 5000 draws; the
    mean of ess_mean / S over the columns, with its standard error se = sd / sqrt(K) measured from the columns themselves,
    must lie within k = 4 standard errors of the law.
    Why k = 4, reasoned before any run.  The relative sd of the estimate is about sqrt(2 (2 M + 1) / S) with M the truncation
    lag, about 10 here: 0.046, so se is about 0.7 % of the law.  The estimator's known biases at these sizes are together
    below that: (a) truncation -- Geyer stops where a pair sum falls to the noise level 1 / sqrt(S) = 0.007, near lag 8 at
    rho = 0.5, and the tail it drops, 2 rho^8 / (1 - rho) = 0.016 of tau = 3, raises ESS by 0.5 % (rho = 0.3: 0.1 %);
    (b) Jensen, E[1 / tau^] - 1 / E[tau^], the squared relative sd: 0.2 %; (c) the O(1 / n) bias of autocovariances about an
    estimated mean, tau / n = 0.06 %.  One standard error is left to these, three to chance.
    Only positive rho: for an antithetic chain tau is small (1 / 3 at rho = -0.5) while the dropped tail is not smaller, so
    the same truncation is several per cent of tau and the law does not hold at a useful k."""
    rng = np.random.default_rng(12)
    for rho in (0.3, 0.5):
        x = R._ar1(rng, rho, 4, 5000, 40)
        r = D.chain_diagnostics(x)['ess_mean'] / 20000.0
        law = (1.0 - rho) / (1.0 + rho)
        se = r.std(ddof=1) / np.sqrt(r.size)
        print(rho, r.mean(), law, se, abs(r.mean() - law) / se)
        assert abs(r.mean() - law) <= 4.0 * se


def zero_sign_draws():
    """(2, 16, 2): zeros of both signs in the middle of the order, -1 and +1 around them; column 1 is all zeros of both signs"""
    x = np.zeros((2, 16, 2))
    x[:, ::2] = -0.0
    x[0, :3, 0], x[1, -3:, 0] = -1.0, 1.0
    return x


def test_a_zero_order_statistic_is_plus_zero():
    x = zero_sign_draws()
    for out in (_rows(D.chain_diagnostics(x)), R.host_mirror(x)):
        assert np.all(out[[2, 3, 4], 1] == 0) and not np.any(np.signbit(out[[0, 2, 3, 4], 1]))      # the constant column
        assert out[2, 0] == 0 and not np.signbit(out[2, 0]) and out[3, 0] == -1.0 and out[4, 0] == 1.0


@pytest.mark.parametrize('defect', ['no_tie_average', 'keep_middle', 'no_monotone', 'lag_short', 'swap_strides'])
def test_bounds_reject_defect(defect):
    """the reference with one defect built in, held to the bounds against the sound reference: some case must fail"""
    names = {'no_tie_average': ('integers', 'two_valued'), 'keep_middle': ('n9', 'n15', 'n513'), 'no_monotone': ('ar99', 'shifted', 'K161'),
             'lag_short': ('ar50', 'n16', 'ar99'), 'swap_strides': ('shifted', 'C3', 'wide_chain')}[defect]
    caught = []
    for name in names:
        x, ref, _ = R.case_reference(_case(name))
        bad, _ = R.reference(x, defect=defect)
        if not R.within(bad, ref, x):
            caught.append(name)
    print(defect, caught)
    assert caught, defect


def test_argument_checks_and_shapes():
    with pytest.raises(ValueError):
        D.chain_diagnostics(np.zeros((2, 7, 3)))
    x = R.case_reference(_case('C3'))[0]
    d = D.chain_diagnostics(x.reshape(3, 64, 3, 1))
    assert d['rhat'].shape == (3, 1) and set(d) == set(R.ROWS)
    one = D.chain_diagnostics(x[0], chains=False)
    assert np.array_equal(one['ess_bulk'], D.chain_diagnostics(x[:1])['ess_bulk'])
    text = D.worst_table(dict((k, v.reshape(1, 3)) for k, v in D.chain_diagnostics(x).items()), 3)
    assert text.startswith("convergence (3 chains)") and text.split("\n")[-1].startswith("3 of 3 parameters flagged")
