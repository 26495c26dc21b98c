"""Host tests of the proximal-gradient state machine (theano_pyglm_amd/csrc/pglm_prox.h built by gcc: tests/prox_mirror.py)
driven by the oracle's ll and gradient: the prox against its closed form, a fit to gtol against a plain numpy ISTA, the
lam_max rule, the NaN rules, per-row lam, subset = batch, and the two failure statuses.  No GPU needed."""
import numpy as np
import pytest

from tests import helpers as H
from tests import prox_mirror as PM

N, B, NT = 4, 5, 3000
GTOL = 1e-5
_CACHE = {}


def _prior(kind):
    return (3.0 if kind == 'exp' else 20.0, 1.0, 1.0, 0.1, 2.0)   # (mu_b, sg_b, stim_sigma, mu, sigma): mu != 0, sigma != 1


def _setup(kind):
    """The problem, its target and lam_max (from the null fit), computed once per nonlinearity and left unchanged."""
    if kind not in _CACHE:
        kw = dict(bias_mu=3.0, w_scale=0.05) if kind == 'exp' else {}
        p = H.Problem(N, NT, H.std_ibasis(), kind=kind, seed=11, **kw)
        tg = PM.oracle_target([p], 0, N)
        prior = _prior(kind)
        null = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, np.inf, gtol=GTOL).run()
        assert np.all(null.field('status') == 0) and not null.support().any()
        gw = null.gx[:, 1:].reshape(N, N, B)
        lam_max = prior[4] * np.max(np.sqrt(np.sum(gw * gw, axis=2)), axis=1)
        _CACHE[kind] = (p, tg, prior, lam_max)
    return _CACHE[kind]


# ---- 1. the prox ---------------------------------------------------------------------------------------------------
def test_prox_equals_closed_form():
    rng = np.random.default_rng(5)
    n, b, ds, mu, sigma, lam, t = 6, 3, 2, 0.1, 2.0, 1.7, 0.3
    thr = t * lam / sigma
    v = np.concatenate([rng.standard_normal(1 + ds), mu + 0.4 * rng.standard_normal(n * b)])
    w = v[1 + ds:].reshape(n, b)
    w[1] = mu                                                   # a zero-norm group
    d = np.array([3.0, 4.0, 12.0]) / 13.0                       # |d| = 1 exactly in floating point
    assert np.sqrt(np.sum(d * d)) == 1.0
    w[2] = mu + 0.5 * thr * d                                   # inside the threshold
    w[4] = mu + 3.0 * thr * d                                   # outside
    z = PM.prox_apply(v, n, b, ds, mu, sigma, lam, t)
    ref = PM.prox_numpy(v[None], n, b, ds, (0, 1, 1, mu, sigma), lam, t)[0]
    assert np.array_equal(z[:1 + ds], v[:1 + ds])               # bias and stimulus untouched
    zw = z[1 + ds:].reshape(n, b)
    assert np.all(zw[1] == mu) and np.all(zw[2] == mu)
    assert np.max(np.abs(z - ref)) <= 4e-16 * np.max(np.abs(v))
    assert np.allclose(zw[4] - mu, 2.0 * thr * d, rtol=1e-14, atol=0.0)
    sup = np.any(zw != mu, axis=1)
    nrm = np.sqrt(np.sum((w - mu) ** 2, axis=1))
    assert np.array_equal(sup, nrm > thr)
    # a group EXACTLY at the threshold gives exactly mu: mu = 0, entries and threshold powers of two (no rounding anywhere)
    for g in ([0.5, 0.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25]):   # norms exactly 0.5 = thr
        zz = PM.prox_apply(np.array([0.7] + g), 1, 4, 0, 0.0, 2.0, 4.0, 0.25)
        assert zz[0] == 0.7 and np.all(zz[1:] == 0.0)
    zz = PM.prox_apply(np.array([0.7, 1.0, 0.0, 0.0, 0.0]), 1, 4, 0, 0.0, 2.0, 4.0, 0.25)
    assert np.array_equal(zz, [0.7, 0.5, 0.0, 0.0, 0.0])
    # lam = 0 leaves a group where it is, lam = +inf sends it to mu
    assert np.allclose(PM.prox_apply(v, n, b, ds, mu, sigma, 0.0, t), v, rtol=0, atol=1e-16)
    assert np.all(PM.prox_apply(v, n, b, ds, mu, sigma, np.inf, t)[1 + ds:] == mu)


# ---- 2. a fit to gtol against ISTA -------------------------------------------------------------------------------------
def _lipschitz(tg, X, prior, iters=30, eps=1e-6):
    """Largest eigenvalue of the Hessian of f at X, row by row: power iteration on finite differences of the gradient."""
    V = np.random.default_rng(0).standard_normal(X.shape)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    _, G0 = PM.smooth_f_grad(tg, X, 0, prior)
    for _ in range(iters):
        HV = (PM.smooth_f_grad(tg, X + eps * V, 0, prior)[1] - G0) / eps
        L = np.linalg.norm(HV, axis=1)
        V = HV / L[:, None]
    return L


def _fit_and_check(kind, gtol=GTOL, rise=0.0):
    """The fit to gtol and what holds of it on its own: the oracle-recomputed KKT residual, F, the monotone trace (rise: how
    much an accepted step may raise F, relative to max(1, |F|))."""
    p, tg, prior, lam_max = _setup(kind)
    lam = 0.5 * lam_max
    m = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, lam, gtol=gtol).run()
    assert np.all(m.field('status') == 0) and np.all(m.field('iters') < 500)
    X = m.x.copy()
    f, G = PM.smooth_f_grad(tg, X, 0, prior)
    r = PM.kkt_residual(X, G, N, B, 0, prior, lam)
    print(kind, "iters", m.field('iters'), "nfev", m.field('nfev'), "restarts", m.field('restarts'), "kkt", r, m.field('kkt'))
    assert np.all(r <= gtol)
    F = f + PM.h_value(X, N, B, 0, prior, lam)
    assert np.allclose(F, m.field('F_x'), rtol=1e-13, atol=0.0)
    for tr in m.F_trace:                                         # the accepted objective values never rise
        assert len(tr) >= 2 and np.all(np.diff(tr) <= rise * np.maximum(1.0, np.abs(tr[:-1])))
    sup = np.any(X[:, 1:].reshape(N, N, B) != prior[3], axis=2)
    assert np.array_equal(sup, m.support()) and sup.any() and not sup.all()      # exact zeros, and not only zeros
    return p, tg, prior, lam, X, F, sup


def _ista(p, tg, prior, lam, n_iter):
    """Plain ISTA in numpy: no momentum, the fixed step 1 / (1.5 L), L the Lipschitz estimate at the start (the factor
    covers the change of curvature along the way)."""
    t = 1.0 / (1.5 * _lipschitz(tg, p.theta.copy(), prior))[:, None]
    Xi = p.theta.copy()
    for _ in range(n_iter):
        _, Gi = PM.smooth_f_grad(tg, Xi, 0, prior)
        Xi = np.concatenate([PM.prox_numpy((Xi - t * Gi)[i:i + 1], N, B, 0, prior, lam[i], t[i, 0]) for i in range(N)])
    fi, Gi = PM.smooth_f_grad(tg, Xi, 0, prior)
    return Xi, fi + PM.h_value(Xi, N, B, 0, prior, lam), PM.kkt_residual(Xi, Gi, N, B, 0, prior, lam)


def test_fit_to_gtol_against_ista():
    """The issue's comparison on H.Problem's own nonlinearity (explinear).  The compared fit runs to gtol = 1e-7; the ISTA takes 3000
    steps of 1 / (1.5 L), which leave its own residual near 3e-4 (printed) -- three orders above the fit's -- and are enough
    for it to have found the support.  Then, plainly: F of the fit is no larger than the ISTA's F, and the supports are equal."""
    _fit_and_check('explinear')                                  # at gtol = 1e-5: the accepted F never rises
    # at 1e-7 the steps are below the rounding of f: a step from y = x may raise F by the allowance of test 1, no more (the
    # bound stated in csrc/pglm_prox.h; twice it here because it is relative to |f|, not |F|)
    p, tg, prior, lam, X, F, sup = _fit_and_check('explinear', 1e-7, rise=2.0 * PM.lib().prox_allowance())
    Xi, Fi, ri = _ista(p, tg, prior, lam, 3000)
    print("F - F_ista", F - Fi, "ISTA residual", ri)
    assert np.all(F <= Fi)
    assert np.array_equal(sup, np.any(Xi[:, 1:].reshape(N, N, B) != prior[3], axis=2))


def test_fit_to_gtol_exp_support_equals_ista():
    """The same fit on the exp nonlinearity.  This problem is so well conditioned that plain ISTA reaches a residual of
    1e-13 within 2000 steps: its F is the optimum to rounding, so 'no larger than the ISTA's F' would compare the fit's gtol
    with rounding noise and is not asserted here; the support is, and the properties the fit has on its own."""
    p, tg, prior, lam, X, F, sup = _fit_and_check('exp')
    Xi, Fi, ri = _ista(p, tg, prior, lam, 2000)
    print("F - F_ista", F - Fi, "ISTA residual", ri)
    assert np.array_equal(sup, np.any(Xi[:, 1:].reshape(N, N, B) != prior[3], axis=2))


# ---- 3. lam_max ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
def test_lam_max(kind):
    """lam >= lam_max: empty support; 0.9 lam_max: not.  At lam = lam_max itself the KKT condition of the last group holds
    with EQUALITY, F is flat to first order along it and a fit that stops at a residual <= gtol may stop a distance
    O(gtol / curvature) away from mu (measured: 9e-4), so 'above' starts a thousandth above."""
    p, tg, prior, lam_max = _setup(kind)
    for fac in (1.001, 2.0, np.inf):
        m = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, fac * lam_max, gtol=GTOL).run()
        assert np.all(m.field('status') == 0) and not m.support().any(), fac
    m = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, 0.9 * lam_max, gtol=GTOL).run()
    assert np.all(m.field('status') == 0) and np.all(m.support().any(axis=1))


# ---- 4. NaN rules ----------------------------------------------------------------------------------------------------------
def test_inf_beyond_a_radius_backtracks_and_nan_gradient_is_zeroed():
    """-ll = 1/2 a |x - c|^2 inside |x| <= 3, +inf outside, c just inside the ball.  The first step has length 1.01 and row 0
    starts 0.9 from c: it overshoots c and leaves the ball, the trial fails, the step halves, the fit converges inside.
    Row 1 (far from the wall) has a NaN in one gradient entry: the entry counts as 0, nothing becomes NaN, and only the
    prox moves that coordinate -- in steps of t lam / sigma, to mu."""
    n, b = 2, 2
    c = np.array([[2.9, 0.5, -0.5, 0.1, 0.1], [1.0, 0.5, -0.5, 0.1, 0.1]])
    a = 50.0
    calls = {'outside': 0}

    def target(X):
        bad = np.sqrt(np.sum(X * X, axis=1)) > 3.0
        calls['outside'] += int(bad[0])
        ll = np.where(bad, -np.inf, -0.5 * np.sum(a * (X - c) ** 2, axis=1))
        g = -a * (X - c)
        g[1, 4] = np.nan
        return ll, g
    X0 = np.array([[2.0, 0.5, -0.5, 0.1, 0.1], [0.0, 0.0, 0.0, 0.1, 0.7]])
    prior = (0.0, 1.0, 1.0, 0.1, 2.0)
    gtol = 1e-8
    m = PM.Mirror(target, X0, n, b, 0, prior, 1.0, gtol=gtol, smooth_prior=False).run()
    print(m.field('status'), m.field('iters'), m.field('nfev'), calls, m.x)
    assert np.all(m.field('status') == 0)
    assert calls['outside'] >= 1                                  # a trial of row 0 landed outside ...
    assert m.field('nfev')[0] > 1 + 2 * m.field('iters')[0] - m.field('restarts')[0]      # ... and was paid for
    assert np.all(np.sqrt(np.sum(m.x * m.x, axis=1)) <= 3.0)
    assert np.all(np.isfinite(m.x)) and m.x[1, 4] == 0.1          # the NaN entry's gradient is 0: shrunk to mu
    G = a * (m.x - c)
    G[1, 4] = 0.0
    assert np.all(PM.kkt_residual(m.x, G, n, b, 0, prior, 1.0) <= gtol)
    assert np.all(np.abs(m.x[:, 0] - c[:, 0]) <= gtol) and np.all(m.x[:, 3:] == 0.1) and np.all(m.x[:, 1:3] != 0.1)


# ---- 5. per-row lam, subset = batch -----------------------------------------------------------------------------------
def test_per_row_lam_and_subset_equals_batch():
    p, tg, prior, lam_max = _setup('explinear')
    lam = np.array([0.0, 0.3, 1.5, 0.7]) * lam_max
    full = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, lam, gtol=GTOL).run()
    assert np.all(full.field('status') == 0)
    sup = full.support()
    assert sup[0].all() and not sup[2].any() and sup[1].sum() >= sup[3].sum() >= 1
    for i in range(N):                                            # every row is the fit of its own lam
        one = PM.Mirror(PM.oracle_target([p], i, i + 1), p.theta[i:i + 1].copy(), N, B, 0, prior, lam[i], gtol=GTOL).run()
        assert np.array_equal(one.x[0], full.x[i]) and np.array_equal(one.sc[:, 0], full.sc[:, i])
    sub = PM.Mirror(PM.oracle_target([p], 1, 3), p.theta[1:3].copy(), N, B, 0, prior, lam[1:3], gtol=GTOL).run()
    assert np.array_equal(sub.x, full.x[1:3]) and np.array_equal(sub.sc, full.sc[:, 1:3])


# ---- 6. the failure statuses -------------------------------------------------------------------------------------------
def test_maxiter_and_max_backtrack_statuses():
    p, tg, prior, lam_max = _setup('exp')
    m = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, 0.5 * lam_max, gtol=GTOL, maxiter=3).run()
    assert np.all(m.field('status') == 1) and np.all(m.field('iters') == 3) and np.all(m.field('phase') == PM.PHASE_DONE)
    x_end = m.x.copy()
    m.step()                                                      # an ended row is never written again
    assert np.array_equal(m.x, x_end) and np.array_equal(m.Xt, x_end)
    m0 = PM.Mirror(tg, p.theta.copy(), N, B, 0, prior, 0.5 * lam_max, gtol=GTOL, maxiter=0).run()
    assert np.all(m0.field('status') == 1) and np.all(m0.field('iters') == 0) and m0.n_evals == 1

    def never(X):                                                 # finite at the start only: every trial fails
        ll, g = tg(X)
        return np.where(np.all(X == p.theta, axis=1), ll, -np.inf), g
    mb = PM.Mirror(never, p.theta.copy(), N, B, 0, prior, 0.5 * lam_max, gtol=GTOL, max_backtrack=5).run()
    assert np.all(mb.field('status') == 2) and np.all(mb.field('nbt') == 5) and np.all(mb.field('iters') == 0)
    assert np.array_equal(mb.x, p.theta) and np.array_equal(mb.Xt, p.theta) and mb.n_evals == 1 + 5


def test_allowance_is_the_documented_one():
    assert PM.lib().prox_allowance() == 1e-12
