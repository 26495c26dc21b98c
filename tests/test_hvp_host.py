"""Host side of the Hessian-vector products (grads.py:68-95 hessian_rop_wrt_list): the priors' hess_log_p_vec against
central differences of their own gradients, the numpy reference product of the GPU tests against central differences of
the unmodified oracle's gradient, and the error paths of the public interface.  No GPU needed."""
import numpy as np
import pytest

from tests import helpers as H


# ---- the reference product of tests/test_gpu_hvp.py -------------------------------------------------------------------
def curvature(x, s, kind, dt):
    """c_t = -dt lam''(x_t) + S[t,n] (log lam)''(x_t)."""
    if kind == 'exp':
        return -dt * np.exp(x)
    sig = 1.0 / (1.0 + np.exp(-x))
    lam = np.logaddexp(0.0, x)
    return -dt * sig * (1.0 - sig) + s * (sig * (1.0 - sig) / lam - sig ** 2 / lam ** 2)


def features(p, n):
    """The materialised feature rows f_t = [1, fstim[t,:], Weff[n',n] fS[t,n',b]] of post-synaptic neuron n, (nT, P)."""
    cols = [np.ones((p.nT, 1))]
    if p.Dstim > 0:
        cols.append(p.fstim)
    cols.append((p.fS * p.Weff[:, n][None, :, None]).reshape(p.nT, p.N * p.B))
    return np.hstack(cols)


def ref_hvp(p, V, neurons=None, t_lo=0, t_hi=None, theta=None):
    """H_n . V[i] = F^T . (c o (F . V[i])) over the bins [t_lo, t_hi) for the listed neurons (default: all)."""
    neurons = range(p.N) if neurons is None else neurons
    t_hi = p.nT if t_hi is None else t_hi
    theta = p.theta if theta is None else theta
    out = np.zeros((len(neurons), p.P))
    for i, n in enumerate(neurons):
        F = features(p, n)[t_lo:t_hi]
        c = curvature(F.dot(theta[n]), p.S[t_lo:t_hi, n].astype(float), p.kind, p.dt)
        out[i] = F.T.dot(c * F.dot(V[i]))
    return out


# ---- 1. priors ---------------------------------------------------------------------------------------------------------
def _prior_cases():
    from theano_pyglm_amd.components.priors import Gaussian, GroupLasso
    return [Gaussian({'mu': 0.3, 'sigma': 2.0}), GroupLasso({'mu': 0.1, 'sigma': 10.0, 'lam': 1.5}),
            GroupLasso({'mu': 0.0, 'sigma': 0.7, 'lam': 0.4})]


@pytest.mark.parametrize('k', [0, 1, 2])
def test_prior_hess_vec_matches_central_difference_of_gradient(k):
    prior = _prior_cases()[k]
    rng = np.random.default_rng(11 + k)
    w = 0.5 + rng.standard_normal((6, 5))                      # seeded, away from a zero group
    v, u = rng.standard_normal((6, 5)), rng.standard_normal((6, 5))
    hv, hu = prior.hess_log_p_vec(w, v), prior.hess_log_p_vec(w, u)
    step = 1e-5 * (1.0 + np.max(np.abs(w)))
    fd = (np.asarray(prior.grad_log_p(w + step * v)) - np.asarray(prior.grad_log_p(w - step * v))) / (2 * step)
    print("prior %d: max|Hv - fd| / max|Hv| = %.3e" % (k, np.max(np.abs(hv - fd)) / np.max(np.abs(hv))))
    assert np.max(np.abs(hv - fd)) <= 1e-7 * np.max(np.abs(hv))
    a, b = np.sum(u * hv), np.sum(v * hu)
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def test_component_hess_vec_matches_central_difference_of_gradient():
    """Every served component's hess_log_p_vec next to its grad_log_p, through Glm.hess_log_prior_vec."""
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars
    mb = make_model('standard_glm', N=3, dt=0.001)
    mb['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': mb['bkgd']['basis']}
    for model in (make_model('standard_glm', N=3, dt=0.001), mb):
        popn = Population(model)
        glm, syms = popn.glm, popn.glm_syms()
        assert glm.hvp_packing() is None
        x = popn.sample(np.random.RandomState(4))
        xn = x['glms'][1]
        # (the sampled group norms are Laplace distributed: some groups sit next to w_g = 0, where a central difference of
        #  the group-lasso gradient is all truncation error -- a seeded point away from it, as for the priors above)
        xn['imp']['w_ir'] = 0.5 + np.random.default_rng(6).standard_normal(np.size(xn['imp']['w_ir']))
        w0, shapes = packdict(get_vars(syms, xn))
        rng = np.random.default_rng(5)
        v, u = rng.standard_normal(w0.size), rng.standard_normal(w0.size)

        def grad(w):
            d = unpackdict(w, shapes)
            d['n'] = 1
            return packdict(get_vars(syms, glm.grad_log_prior(d)))[0]

        def hess(p):
            return packdict(get_vars(syms, glm.hess_log_prior_vec(xn, unpackdict(p, shapes))))[0]

        hv, hu = hess(v), hess(u)
        step = 1e-5 * (1.0 + np.max(np.abs(w0)))
        fd = (grad(w0 + step * v) - grad(w0 - step * v)) / (2 * step)
        assert np.max(np.abs(hv - fd)) <= 1e-7 * np.max(np.abs(hv))
        assert abs(u.dot(hv) - v.dot(hu)) <= 1e-12 * max(abs(u.dot(hv)), abs(v.dot(hu)))


# ---- 2. the reference product against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize('Dstim', [0, 3])
@pytest.mark.parametrize('kind,kw', [('exp', {}), ('explinear', {}), ('explinear', {'bias_mu': 1.0, 'w_scale': 0.5})])
@pytest.mark.parametrize('seed', [3, 5])
def test_reference_product_is_the_oracles_second_derivative(kind, kw, Dstim, seed):
    """F^T (c o (F v)) equals the central difference (step 1e-5 along a standard-normal v) of the oracle's glm_ll_grad to
    1e-7 max|H v|.  (The oracle alone gives 4.5e-11 .. 7.2e-10 on these inputs; differencing noise is 1.2e-8 at step
    1e-6 and truncation 2.3e-8 at 1e-4: 1e-7 can only fail on a wrong formula.)"""
    p = H.Problem(6, 2000, H.std_ibasis(200), kind=kind, Dstim=Dstim, seed=seed, weighted=True, **kw)
    rng = np.random.default_rng(100 + seed)
    V = rng.standard_normal((p.N, p.P))
    hv = ref_hvp(p, V)
    if kind == 'explinear':                                   # the two regimes the GPU tests run: large currents / around zero
        x = np.array([features(p, n).dot(p.theta[n]) for n in range(p.N)])
        print("currents %.2f .. %.2f" % (x.min(), x.max()))
        assert (np.median(x) > 12.0) if not kw else (x.min() < 0.0 < x.max())
    step = 1e-5
    th0 = p.theta
    try:
        p.theta = th0 + step * V
        _, gp = p.oracle_ll_grad()
        p.theta = th0 - step * V
        _, gm = p.oracle_ll_grad()
    finally:
        p.theta = th0
    fd = (gp - gm) / (2 * step)
    err = np.max(np.abs(hv - fd)) / np.max(np.abs(hv))
    print("%s %s Dstim=%d seed=%d: max|Hv - fd| / max|Hv| = %.3e" % (kind, kw, Dstim, seed, err))
    assert err <= 1e-7
    if kind == 'exp' or kw:
        assert np.all(np.einsum('ij,ij->i', V, hv) < 0.0)


# ---- 3. error paths ---------------------------------------------------------------------------------------------------------
def test_fit_glm_use_hessian_raises():
    from theano_pyglm_amd.inference import coord_descent as cd
    with pytest.raises(NotImplementedError, match="dense"):
        cd.fit_glm({'glm': {}}, 0, (None, None, None), use_hessian=True)
    # Rop takes precedence over the dense Hessian (parallel_coord_descent.py:75-76): no NotImplementedError then
    with pytest.raises(ValueError, match="hessp"):
        cd.fit_glm({'glm': {}}, 0, (None, None, None), use_hessian=True, use_rop=True)


@pytest.mark.parametrize('name', ['sparse_weighted_model', 'spatiotemporal_glm'])
def test_compute_hvp_of_unserved_packing_raises(name):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.utils.packvec import packdict, get_vars
    popn = Population(make_model(name, N=2, dt=0.001))
    x = popn.sample(np.random.RandomState(1))
    v = np.ones(packdict(get_vars(popn.glm_syms(), x['glms'][0]))[0].size)
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        popn.compute_hvp(x, 0, v)
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        popn.compute_hvp_packed(x, np.ones((2, v.size)))


def test_hvp_symbols_and_version():
    import ctypes
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ('pgl_hvp_prepare_dev', 'pgl_hvp_prepare_list_dev', 'pgl_hvp_apply_dev', 'pgl_hvp'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert _lib.load().pgl_version() >= 101
    for m in ('hvp_prepare', 'hvp_apply', 'hvp'):
        assert hasattr(_lib.DeviceGlm, m)
