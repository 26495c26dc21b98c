"""CPU tests of the lock-step Newton-CG optimiser's core (theano_pyglm_amd/csrc/pglm_ncg.h, compiled for the host with gcc
through tests/csrc/ncg_host.c and driven row by row with numpy supplying f, g and H v): it takes the iterates of
scipy.optimize.minimize(method='Newton-CG', jac=, hessp=) -- what fit_glm(use_rop=True) runs per neuron
(parallel_coord_descent.py:119-121 / map.py:38-45) -- and returns scipy's status codes on its exits; plus the host side of
the public interface (batched_newton_cg.supported, exported symbols).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.optimize as opt

from oracle import glm_oracle as O
from tests import helpers as H
from tests.test_hvp_host import curvature, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def ncg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('ncg') / 'ncg_host.so')
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'ncg_host.c')])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.ncg_start.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, vp]
    lib.ncg_feed_hv.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    lib.ncg_feed_fg.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


SC = dict(f=0, fprev=1, dri0=2, termcond=3, cgit=4, alphai=5, nit=6, nhev=7, nfev=8, status=9, phase=10)


def core_minimize(lib, f, g, hessp, x0, maxiter=225):
    """The core, one row: returns (x, fun, nit, nhev, status, allvecs)."""
    P = x0.size
    sc, ls = np.zeros(lib.ncg_nscal()), np.zeros(lib.ncg_nls())
    vec = np.zeros((8, P))
    vec[0] = x0
    allvecs = [x0.copy()]
    g0 = np.ascontiguousarray(g(x0), dtype=float)
    ph = lib.ncg_start(_p(sc), _p(ls), _p(vec), P, maxiter, float(f(x0)), _p(g0))
    nit = 0
    calls = 0
    while ph != 2:
        calls += 1
        assert calls < 10 ** 6
        if ph == 0:
            hv = np.ascontiguousarray(hessp(vec[0].copy(), vec[4].copy()), dtype=float)
            ph = lib.ncg_feed_hv(_p(sc), _p(ls), _p(vec), P, maxiter, _p(hv))
        else:
            xt = vec[7].copy()
            gt = np.ascontiguousarray(g(xt), dtype=float)
            ph = lib.ncg_feed_fg(_p(sc), _p(ls), _p(vec), P, maxiter, float(f(xt)), _p(gt))
        if sc[SC['nit']] > nit:
            nit = int(sc[SC['nit']])
            allvecs.append(vec[0].copy())
    return vec[0].copy(), sc[SC['f']], int(sc[SC['nit']]), int(sc[SC['nhev']]), int(sc[SC['status']]), allvecs


def scipy_minimize(f, g, hessp, x0, maxiter=225):
    """fit_glm's call (coord_descent.fit_glm: its NaN rules wrap f, g and hessp)."""
    def nll(v):
        y = f(v)
        return 1e16 if np.isnan(y) else y

    def gr(v):
        y = g(v)
        return np.zeros_like(y) if np.any(np.isnan(y)) else y

    def hp(v, p):
        y = hessp(v, p)
        return np.zeros_like(y) if np.any(np.isnan(y)) else y

    # (scipy's own return_all list aliases the array it updates in place: every entry is the final point; the callback
    #  sees each outer iterate)
    rec = [x0.copy()]
    res = opt.minimize(nll, x0.copy(), method='Newton-CG', jac=gr, hessp=hp, options={'maxiter': maxiter},
                       callback=lambda xk: rec.append(np.array(xk, dtype=float)))
    res['allvecs'] = rec
    return res


def scipy_margins(g, hessp, allvecs, nhev):
    """From scipy's side alone: replay the CG recursion of scipy's _minimize_newtoncg at scipy's own recorded outer
    iterates with numpy, and return the smallest relative distance of any decision from its threshold: |ri|_1 against
    termcond, curv against 0 (relative to |p| |H p|) and 3 eps, the update norm against P * 1e-5.  The replay must make
    exactly scipy's number of products (it is scipy's arithmetic on scipy's points)."""
    P = allvecs[0].size
    xtol = P * 1e-5
    worst = np.inf
    products = 0
    for k in range(len(allvecs) - 1):
        xk = allvecs[k]
        b = -g(xk)
        maggrad = np.linalg.norm(b, ord=1)
        termcond = min(0.5, np.sqrt(maggrad)) * maggrad
        xsupi = np.zeros(P)
        ri = -b
        psupi = -ri
        dri0 = ri.dot(ri)
        i = 0
        for _ in range(20 * P):
            r1 = np.add.reduce(np.abs(ri))
            worst = min(worst, abs(r1 - termcond) / termcond)
            if r1 <= termcond:
                break
            Ap = hessp(xk, psupi)
            products += 1
            curv = psupi.dot(Ap)
            worst = min(worst, abs(curv) / (np.linalg.norm(psupi) * np.linalg.norm(Ap)))
            if 0 <= curv <= 3 * EPS:
                break
            if curv < 0:
                break
            alphai = dri0 / curv
            xsupi = xsupi + alphai * psupi
            ri = ri + alphai * Ap
            dri1 = ri.dot(ri)
            psupi = -ri + (dri1 / dri0) * psupi
            i += 1
            dri0 = dri1
        upd = np.linalg.norm(allvecs[k + 1] - xk, ord=1)
        worst = min(worst, abs(upd - xtol) / xtol)
    assert products == nhev, (products, nhev)
    return worst


def check_against_scipy(lib, f, g, hessp, x0, label, maxiter=225, expect_status=0):
    ref = scipy_minimize(f, g, hessp, x0, maxiter)
    margin = scipy_margins(lambda v: np.where(np.any(np.isnan(g(v))), 0.0, g(v)), hessp, ref.allvecs, ref.nhev)
    x, fun, nit, nhev, status, allvecs = core_minimize(lib, f, g, hessp, x0, maxiter)
    scale = max(np.max(np.abs(v)) for v in ref.allvecs)
    n = min(len(allvecs), len(ref.allvecs))
    err = max(np.max(np.abs(a - b)) for a, b in zip(allvecs[:n], ref.allvecs[:n])) / scale
    print("%s: scipy nit %d nhev %d status %d | core nit %d nhev %d status %d | max iterate error %.2e | margin %.2e"
          % (label, ref.nit, ref.nhev, ref.status, nit, nhev, status, err, margin))
    assert ref.status == expect_status
    assert margin > 1e-6, "a decision of scipy's run is within 1e-6 of its threshold: pick another seed"
    assert (nit, nhev, status) == (ref.nit, ref.nhev, ref.status)
    assert len(allvecs) == len(ref.allvecs)
    assert err <= 1e-10
    assert abs(fun - ref.fun) <= 1e-10 * max(1.0, abs(ref.fun))


# ---- 1. the core takes scipy's iterates ---------------------------------------------------------------------------------
def quadratic(P, cond, seed, negative=0, spectrum='full', saddle_start=False):
    """f = 0.5 x^T A x - c^T x + 0.25 q sum x^4 (q > 0 only with negative eigenvalues, to bound f below).
    spectrum 'full': P log-spaced eigenvalues in a random orthogonal basis; 'scaled': badly scaled coordinates -- a
    diagonal A with three distinct values 1, sqrt(cond), cond (the shape of the GLM's own ill-conditioning: prior
    precisions beside O(1) directions)."""
    rng = np.random.default_rng(seed)
    if spectrum == 'full':
        Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
        ev = np.logspace(0.0, np.log10(cond), P)
        ev[:negative] *= -1.0
        A = (Q * ev).dot(Q.T)
        A = 0.5 * (A + A.T)
    else:
        Q = np.eye(P)
        A = np.diag(np.repeat(np.logspace(0.0, np.log10(cond), 3), P // 3))
    c = rng.standard_normal(P)
    x0 = rng.standard_normal(P)
    if saddle_start:                       # the first CG direction -g(x0) = c is (nearly) an eigenvector of negative curvature
        c = Q[:, 0] + 0.01 * c
        x0 = np.zeros(P)
    q = 1.0 if negative else 0.0
    return (lambda x: 0.5 * x.dot(A.dot(x)) - c.dot(x) + 0.25 * q * np.sum(x ** 4),
            lambda x: A.dot(x) - c + q * x ** 3,
            lambda x, p: A.dot(p) + 3.0 * q * x ** 2 * p,
            x0)


@pytest.mark.parametrize('cond,seed,spectrum', [(1.0, 1, 'full'), (1e2, 2, 'full'), (1e4, 3, 'scaled'), (1e6, 6, 'scaled'),
                                                (1e8, 3, 'scaled')])
def test_core_reproduces_scipy_on_convex_quadratics(ncg, cond, seed, spectrum):
    """Strictly convex quadratics, condition numbers 1 .. 1e8.  From 1e4 on the spectrum has three distinct values on
    the coordinate axes: CG then ends within three iterations per solve and stays out of the regime where the order of
    summation of a dot product alone (numpy's blocked sums against a sequential loop) moves the iterates of ANY two
    implementations apart by cond * eps and more (measured on log-spaced spectra in a random basis: 4e-6 at cond 1e4
    after 36 products, growing smoothly from 1e-16 -- CG's loss of orthogonality, not a branch).  The seeds are ones
    for which scipy's run keeps every decision 1e-6 away from its threshold (asserted) and whose last line search,
    where the decrease of f falls below the spacing of f, still succeeds in scipy."""
    f, g, hp, x0 = quadratic(12, cond, seed, spectrum=spectrum)
    check_against_scipy(ncg, f, g, hp, x0, "quadratic cond %.0e" % cond)


INDEFINITE = [(1, 11, False), (3, 12, True)]


def _negative_curvature_exits(f, g, hp, x0):
    """How often scipy's run meets curv < 0 on the first / on a later CG iteration of a solve."""
    seen = {'first': 0, 'later': 0}
    state = {'x': None, 'i': 0}

    def hp_spy(x, p):
        if state['x'] is None or not np.array_equal(state['x'], x):
            state['x'], state['i'] = x.copy(), 0
        Ap = hp(x, p)
        if p.dot(Ap) < 0:
            seen['first' if state['i'] == 0 else 'later'] += 1
        state['i'] += 1
        return Ap

    scipy_minimize(f, g, hp_spy, x0)
    return seen


@pytest.mark.parametrize('negative,seed,saddle', INDEFINITE)
def test_core_reproduces_scipy_with_negative_curvature(ncg, negative, seed, saddle):
    """Indefinite Hessians (a quartic term bounds f below): the steepest-descent exit (negative curvature on the first
    CG iteration) and the exit that keeps the CG iterate (on a later one)."""
    f, g, hp, x0 = quadratic(10, 50.0, seed, negative=negative, saddle_start=saddle)
    seen = _negative_curvature_exits(f, g, hp, x0)
    print("negative curvature in scipy's run:", seen)
    assert seen['first' if saddle else 'later'] > 0
    check_against_scipy(ncg, f, g, hp, x0, "indefinite (%d negative)" % negative)


def glm_objective(kind, prior, seed):
    """-(ll + log prior) of neuron 1 of a seeded N = 4 problem (6 s of spikes, complete graph) from oracle pieces: glm_ll_grad and the F^T (c o (F v))
    construction of tests/test_hvp_host.py; bias N(mu_b, 1), impulse weights Gaussian or group lasso."""
    from theano_pyglm_amd.components.priors import Gaussian, GroupLasso
    p = H.Problem(4, 6000, H.std_ibasis(200), kind=kind, seed=seed,
                  **({'bias_mu': 1.0, 'w_scale': 0.5} if kind == 'explinear' else {}))
    n = 1
    Sf = p.S.astype(float)
    F = features(p, n)
    mu_b, sg_b = p.theta[n, 0], 1.0
    pr = Gaussian({'mu': 0.0, 'sigma': 1.0}) if prior == 'gaussian' else GroupLasso({'mu': 0.0, 'sigma': 1.0, 'lam': 1.0})

    def ll_grad(x):
        ll, gb, _, gw = O.glm_ll_grad(n, Sf, p.fS, x[1:].reshape(p.N, p.B), p.Weff[:, n], x[0], p.dt, p.kind, None, None)
        return ll, np.concatenate([[gb], gw.reshape(-1)])

    def f(x):
        return -(ll_grad(x)[0] - 0.5 / sg_b ** 2 * (x[0] - mu_b) ** 2 + pr.log_p(x[1:].reshape(p.N, p.B)))

    def g(x):
        gp = np.concatenate([[-(x[0] - mu_b) / sg_b ** 2], np.asarray(pr.grad_log_p(x[1:].reshape(p.N, p.B))).reshape(-1)])
        return -(ll_grad(x)[1] + gp)

    def hp(x, v):
        c = curvature(F.dot(x), Sf[:, n], p.kind, p.dt)
        hv = F.T.dot(c * F.dot(v))
        hpv = np.concatenate([[-v[0] / sg_b ** 2],
                              np.asarray(pr.hess_log_p_vec(x[1:].reshape(p.N, p.B), v[1:].reshape(p.N, p.B))).reshape(-1)])
        return -(hv + hpv)

    return f, g, hp, p.theta[n].copy()


@pytest.mark.parametrize('kind', ['exp', 'explinear'])
@pytest.mark.parametrize('prior', ['gaussian', 'group_lasso'])
def test_core_reproduces_scipy_on_glm_objective(ncg, kind, prior):
    f, g, hp, x0 = glm_objective(kind, prior, seed=7)
    check_against_scipy(ncg, f, g, hp, x0, "glm %s %s" % (kind, prior))


# ---- 2. NaN rules and exits --------------------------------------------------------------------------------------------
def test_status_codes_of_the_exits(ncg):
    f, g, hp, x0 = quadratic(8, 1e3, 21)
    # maxiter
    for mi in (0, 1, 2):
        ref = scipy_minimize(f, g, hp, x0, maxiter=mi)
        x, fun, nit, nhev, status, _ = core_minimize(ncg, f, g, hp, x0, maxiter=mi)
        assert (status, nit, nhev) == (ref.status, ref.nit, ref.nhev) and status == 1
        assert np.max(np.abs(x - ref.x)) <= 1e-10 * np.max(np.abs(ref.x))
    # CG runs out of its 20 P iterations: scipy's status 3 (a skew-dominated "Hessian": the curvature p.Ap = |p|^2 stays
    # positive and the residual never falls below termcond)
    A = np.array([[1.0, 10.0], [-10.0, 1.0]])
    fl, gl, hl = (lambda x: np.sum(x)), (lambda x: np.ones(2)), (lambda x, p: A.dot(p))
    ref = scipy_minimize(fl, gl, hl, np.zeros(2))
    res = core_minimize(ncg, fl, gl, hl, np.zeros(2))
    assert (res[4], res[2], res[3]) == (ref.status, ref.nit, ref.nhev) == (3, 0, 40)
    # a gradient holding a NaN -> zero gradient: the zero update, scipy's status 0 after one iteration, x unchanged
    gn = lambda x: np.where(np.arange(x.size) == 2, np.nan, g(x))           # noqa: E731
    ref = scipy_minimize(f, gn, hp, x0)
    x, fun, nit, nhev, status, _ = core_minimize(ncg, f, gn, hp, x0)
    assert (status, nit, nhev) == (ref.status, ref.nit, ref.nhev) == (0, 1, 0)
    assert np.array_equal(x, x0) and np.array_equal(ref.x, x0)
    # a product holding a NaN -> zero product: curvature 0 on the first CG iteration, the zero update as well
    hn = lambda x, p: np.full(x.size, np.nan)                               # noqa: E731
    ref = scipy_minimize(f, g, hn, x0)
    x, fun, nit, nhev, status, _ = core_minimize(ncg, f, g, hn, x0)
    assert (status, nit, nhev) == (ref.status, ref.nit, ref.nhev) == (0, 1, 1)
    assert np.array_equal(x, x0)
    # NaN objective everywhere but the start: 1e16 at every trial, no sufficient decrease: precision loss (status 2)
    fbad = lambda x: f(x) if np.array_equal(x, x0) else np.nan              # noqa: E731
    ref = scipy_minimize(fbad, g, hp, x0)
    x, fun, nit, nhev, status, _ = core_minimize(ncg, fbad, g, hp, x0)
    print("NaN objective: scipy status %d nit %d | core status %d nit %d" % (ref.status, ref.nit, status, nit))
    assert status == ref.status == 2 and nit == ref.nit == 0 and np.array_equal(x, x0)


# ---- 3. host side of the public interface ------------------------------------------------------------------------------
def test_supported_models():
    from theano_pyglm_amd.inference import batched_newton_cg as B
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    m = make_model('standard_glm', N=3, dt=0.001)
    assert B.supported(Population(m))
    mb = make_model('standard_glm', N=3, dt=0.001)
    mb['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': mb['bkgd']['basis']}
    assert B.supported(Population(mb))
    for mm in (make_model('standard_glm', N=3, dt=0.001), mb):
        mm = dict(mm)
        mm['impulse'] = dict(mm['impulse'], prior={'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0})
        assert B.supported(Population(mm))
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):
        popn = Population(make_model(name, N=3, dt=0.001))
        assert not B.supported(popn)
        x = popn.sample(np.random.RandomState(1))
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            B.fit_glms_newton_cg_torch(popn, x)


def test_coord_descent_argument_errors():
    from theano_pyglm_amd.inference import coord_descent as cd
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model('standard_glm', N=2, dt=0.001))
    with pytest.raises(ValueError, match="use_rop"):
        cd.coord_descent(popn, popn.sample(np.random.RandomState(1)), use_rop=True, batched=True)
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):
        popn = Population(make_model(name, N=2, dt=0.001))
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            cd.coord_descent(popn, popn.sample(np.random.RandomState(1)), use_rop=True, batched='torch')


def test_ncg_symbols_version_and_kernels():
    import __graft_entry__ as ge
    ge.build_hip()
    import sys
    from theano_pyglm_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    names = ('pgl_ncg_state_doubles', 'pgl_ncg_init_dev', 'pgl_ncg_cg_step_dev', 'pgl_ncg_trial_dev',
             'pgl_ncg_search_step_dev')
    hdr = open(os.path.join(ROOT, 'include', 'pyglm_hip.h')).read()
    for n in names:
        assert hasattr(lib, n) and n in _lib.SYMBOLS and (n + '(') in hdr
    assert _lib.load().pgl_version() >= 102
    for m in ('ncg_state_doubles', 'ncg_init_dev', 'ncg_cg_step_dev', 'ncg_trial_dev', 'ncg_search_step_dev'):
        assert hasattr(_lib.DeviceGlm, m)
    assert _lib.load().pgl_ncg_state_doubles(3, 7) == 3 * 7 * 7 + 3 * (ncg_nscal_host() + 18)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import reachable_kernels as RK
    built = RK.built_fused()
    mine = dict((n, r) for n, r in built.items() if n.startswith('k_ncg_') or n == 'k_row_trial')  # (the trial kernel is shared)
    assert len(mine) >= 4, sorted(mine)
    for n, r in mine.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0, (n, r)
        assert not n.startswith(RK.FUSED)


def ncg_nscal_host():
    import re
    src = open(os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_ncg.h')).read()
    return int(re.search(r'#define PGL_NCG_NSCAL (\d+)', src).group(1))
