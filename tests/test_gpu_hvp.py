"""Device Hessian-vector products of ll (pgl_hvp, pgl_hvp_prepare_* / pgl_hvp_apply_dev) through the C ABI against the
numpy product F^T (c o (F v)) of tests/test_hvp_host.py (itself held to the oracle's second derivative there), the host
mirror on top of them, and the Newton-CG MAP fit (fit_glm(use_rop=True))."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests.test_hvp_host import ref_hvp
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-9          # of max|H v|: the bound the gradient is held to (README "Parity status")


def _torch():
    import torch
    return torch


def _dev_apply(d, theta, Weff, V, n_lo=0, n_hi=None, idx=None, napply=1):
    """prepare + apply with device buffers (torch tensors as the allocator); returns the products of `napply` applies."""
    torch = _torch()
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W, d_v = t(theta), t(Weff), t(V)
    d_hv = torch.full(V.shape, float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    if idx is not None:
        d_idx = torch.tensor(np.asarray(idx), dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), d_idx=d_idx.data_ptr(), count=len(idx))
    else:
        d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), n_lo, n_hi)
    outs = []
    for _ in range(napply):
        d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
        d.sync()
        outs.append(d_hv.cpu().numpy().copy())
    return outs


def _err(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


CASES = [
    # (name, N, nT, kind, problem kwargs, Dstim)
    ('N4-explinear', 4, 3000, 'explinear', {}, 0),
    ('N4-explinear-zero', 4, 3000, 'explinear', {'bias_mu': 1.0, 'w_scale': 0.5}, 0),
    ('N4-exp', 4, 3000, 'exp', {}, 0),
    ('N32-explinear', 32, 3000, 'explinear', {}, 0),
    ('N32-explinear-zero', 32, 3000, 'explinear', {'bias_mu': 1.0, 'w_scale': 0.5}, 0),
    ('N32-exp', 32, 3000, 'exp', {}, 0),
    ('N64-Dstim9', 64, 3000, 'explinear', {}, 9),
    ('N144-wide', 144, 2000, 'explinear', {}, 0),
    ('N144-wide-exp', 144, 2000, 'exp', {}, 0),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_hvp_matches_reference(case):
    name, N, nT, kind, kw, Dstim = case
    ib = H.std_ibasis(200)
    p = H.Problem(N, nT, ib, kind=kind, Dstim=Dstim, seed=17, weighted=True, **kw)
    V = np.random.default_rng(23).standard_normal((N, p.P))
    ref = ref_hvp(p, V)
    d = p.device(0)
    try:
        hv = d.hvp(p.theta, V, p.Weff)
        e1 = _err(hv, ref)
        hv2 = _dev_apply(d, p.theta, p.Weff, V, 0, N)[0]
        e2 = _err(hv2, ref)
        print("%s: one-shot %.3e, prepare + apply %.3e of max|Hv|" % (name, e1, e2))
        assert e1 <= TOL and e2 <= TOL
    finally:
        d.close()


@pytest.mark.parametrize('kind,kw', [('explinear', {}), ('explinear', {'bias_mu': 1.0, 'w_scale': 0.5}), ('exp', {})],
                         ids=['explinear', 'explinear-zero', 'exp'])
def test_hvp_c3_class_takes_the_fused_apply_kernel(kind, kw):
    """N = 128 at a short recording (4 800 bins = 300 tiles: more tiles than chunks): the fused apply on resident tiles."""
    N, nT = 128, 4800
    p = H.Problem(N, nT, H.std_ibasis(200), kind=kind, seed=29, weighted=True, **kw)
    V = np.random.default_rng(31).standard_normal((N, p.P))
    ref = ref_hvp(p, V)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        outs = _dev_apply(d, p.theta, p.Weff, V, 0, N, napply=2)
        names = d.last_kernels()
        print("N=128 %s %s: %.3e of max|Hv|; kernels %s" % (kind, kw, _err(outs[0], ref), names))
        assert names == ['k_hvp5<18, 22, 0>', 'k_fused5<18, 22, 2, 0, 0, 0>']
        assert _err(outs[0], ref) <= TOL
        assert np.array_equal(outs[0], outs[1])                # two applies after one prepare: bit-identical
        hv = d.hvp(p.theta, V, p.Weff)
        assert _err(hv, ref) <= TOL
        # a sub-range of five post tiles with a ragged last tile (helper form of pass 2) and a neuron list
        lo, hi = 40, 113
        o = _dev_apply(d, p.theta[lo:hi], p.Weff, V[lo:hi], lo, hi)[0]
        assert d.last_kernels()[0] == 'k_hvp5<18, 22, 0>'
        assert _err(o, ref[lo:hi]) <= TOL
        idx = np.random.default_rng(37).permutation(N)[:70]
        o = _dev_apply(d, p.theta[idx], p.Weff, V[idx], idx=idx)[0]
        assert d.last_kernels()[0] == 'k_hvp5<18, 22, 0>'
        assert _err(o, ref[idx]) <= TOL
    finally:
        d.close()


def test_hvp_subrange_and_list_small():
    p = H.Problem(32, 3000, H.std_ibasis(200), kind='explinear', seed=41, weighted=True, bias_mu=1.0, w_scale=0.5)
    V = np.random.default_rng(43).standard_normal((32, p.P))
    ref = ref_hvp(p, V)
    d = p.device(0)
    try:
        hv = d.hvp(p.theta[5:22], V[5:22], p.Weff, 5, 22)
        assert _err(hv, ref[5:22]) <= TOL
        idx = np.array([30, 2, 17, 9, 4], dtype=np.int32)
        o = _dev_apply(d, p.theta[idx], p.Weff, V[idx], idx=idx)[0]
        assert _err(o, ref[idx]) <= TOL
    finally:
        d.close()


@pytest.mark.parametrize('N', [32, 128])
def test_hvp_structure(N):
    """Symmetry, negative semi-definiteness (exp), determinism, linearity."""
    for kind in ('exp', 'explinear'):
        p = H.Problem(N, 3200, H.std_ibasis(200), kind=kind, seed=47, weighted=True)
        rng = np.random.default_rng(53)
        U, V = rng.standard_normal((N, p.P)), rng.standard_normal((N, p.P))
        a, b = 0.7, -1.9
        d = p.device(0)
        try:
            hu, hv, hl = d.hvp(p.theta, U, p.Weff), d.hvp(p.theta, V, p.Weff), d.hvp(p.theta, a * V + b * U, p.Weff)
            hv_again = d.hvp(p.theta, V, p.Weff)
        finally:
            d.close()
        uhv, vhu = np.einsum('ij,ij->i', U, hv), np.einsum('ij,ij->i', V, hu)
        assert np.all(np.abs(uhv - vhu) <= 1e-9 * np.maximum(np.abs(uhv), np.abs(vhu)))
        if kind == 'exp':
            assert np.all(np.einsum('ij,ij->i', V, hv) <= 0.0)
        assert np.array_equal(hv, hv_again)
        assert _err(hl, a * hv + b * hu) <= 1e-9


@pytest.mark.parametrize('N', [16, 128])
def test_hvp_time_range(N):
    nT, t = 4800, 2000 - 2000 % 16
    p = H.Problem(N, nT, H.std_ibasis(200), kind='explinear', seed=59, weighted=True, bias_mu=1.0, w_scale=0.5)
    V = np.random.default_rng(61).standard_normal((N, p.P))
    d = p.device(0)
    try:
        whole = d.hvp(p.theta, V, p.Weff)
        d.set_time_range(0, t)
        first = d.hvp(p.theta, V, p.Weff)
        assert _err(first, ref_hvp(p, V, t_lo=0, t_hi=t)) <= TOL
        d.set_time_range(t, nT)
        second = d.hvp(p.theta, V, p.Weff)
        assert _err(first + second, whole) <= 1e-9
        # apply after a changed time range without a new prepare
        torch = _torch()
        d_v = torch.tensor(V, dtype=torch.float64, device='cuda')
        d_hv = torch.empty_like(d_v)
        torch.cuda.synchronize()
        d.set_time_range(0, nT)
        with pytest.raises(_lib.PglError, match="error -3"):
            d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
    finally:
        d.close()


def test_hvp_state_and_unsupported():
    torch = _torch()
    p = H.Problem(8, 2000, H.std_ibasis(200), seed=67)
    d = p.device(0)
    try:
        d_v = torch.zeros((8, p.P), dtype=torch.float64, device='cuda')
        d_hv = torch.empty_like(d_v)
        torch.cuda.synchronize()
        with pytest.raises(_lib.PglError, match="error -3"):          # apply before prepare
            d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
        d.hvp(p.theta, np.ones((8, p.P)), p.Weff)
        d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())                  # prepared now
        d.sync()
        d.set_spikes(p.S)                                              # new spikes: stale
        with pytest.raises(_lib.PglError, match="error -3"):
            d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
        stim = np.random.default_rng(71).standard_normal((20, 6))
        d.set_stimulus_separable(stim, 0.1, H.std_ibasis(200)[:, :3])
        with pytest.raises(_lib.PglError, match="error -4.*separable"):
            d.hvp(np.zeros((8, d.P)), np.zeros((8, d.P)), p.Weff)
    finally:
        d.close()


# ---- host mirror -------------------------------------------------------------------------------------------------------
def _std_population(N, T, seed, basis_stim=False, nlin=None, bias_mu=None):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    if basis_stim:
        model['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': model['bkgd']['basis']}
    if nlin:
        model['nonlinearity']['type'] = nlin
    if bias_mu is not None:
        model['bias']['mu'] = bias_mu
    popn = Population(model)
    nT = int(round(T / 0.001))
    rng = np.random.default_rng(seed)
    S = np.minimum(rng.poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    data = {'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': None, 'dt_stim': 0.1}
    if basis_stim:
        data['stim'] = rng.standard_normal((int(round(T / 0.1)), 2))
    popn.add_data(data)
    return popn


@pytest.mark.parametrize('basis_stim', [False, True], ids=['standard_glm', 'basis_stimulus'])
def test_population_compute_hvp_matches_difference_of_compute_grad(basis_stim):
    from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars, set_vars
    N = 4
    popn = _std_population(N, 6.0, 73, basis_stim=basis_stim)
    try:
        x = popn.sample(np.random.RandomState(79))
        rng = np.random.default_rng(83)
        for n in range(N):                                     # away from a zero group (see tests/test_hvp_host.py)
            x['glms'][n]['imp']['w_ir'] = 0.5 + rng.standard_normal(np.size(x['glms'][n]['imp']['w_ir']))
        syms = popn.glm_syms()
        n = 2
        w0, shapes = packdict(get_vars(syms, x['glms'][n]))
        v = rng.standard_normal(w0.size)
        hv = popn.compute_hvp(x, n, v)
        step = 1e-5 * (1.0 + np.max(np.abs(w0)))

        def grad(w):
            xx = copy.deepcopy(x)
            set_vars(syms, xx['glms'][n], unpackdict(w, shapes))
            return popn.compute_grad(xx, n)

        gp, gm = grad(w0 + step * v), grad(w0 - step * v)
        fd = (gp - gm) / (2 * step)
        # bound: 1e-7 max|Hv| for the truncation of the exact-f64 difference (as for the priors) plus what the device
        # gradient's own 1e-9 relative error allows in the difference: 2 * 1e-9 * max|g| / (2 * step)
        bound = 1e-7 * np.max(np.abs(hv)) + 1e-9 * max(np.max(np.abs(gp)), np.max(np.abs(gm))) / step
        print("compute_hvp: max|Hv - fd| = %.3e, bound %.3e, max|Hv| = %.3e" % (np.max(np.abs(hv - fd)), bound, np.max(np.abs(hv))))
        assert np.max(np.abs(hv - fd)) <= bound
        Vall = rng.standard_normal((N, w0.size))
        Vall[n] = v
        HV = popn.compute_hvp_packed(x, Vall)
        for m in range(N):
            assert np.array_equal(HV[m], popn.compute_hvp(x, m, Vall[m])) or \
                _err(HV[m], popn.compute_hvp(x, m, Vall[m])) <= 1e-12
        assert _err(HV[n], hv) <= 1e-12
    finally:
        popn.release_data()


def test_newton_cg_fit_reaches_the_bfgs_optimum():
    """fit_glm(use_rop=True) -- Newton-CG on device Hessian-vector products -- against today's BFGS fit_glm from the same
    point, on a seeded standard_glm with the exp nonlinearity at C1 size (N = 4, 60 s; bias prior centred on log 20 so
    that the prior's sample is a sane start for exp).  Newton-CG must succeed and its objective must not be worse than
    BFGS's beyond ten times the slack of BFGS's own stopping rule, measured by restarting BFGS from its optimum."""
    from theano_pyglm_amd.inference import coord_descent as cd
    popn = _std_population(4, 60.0, 89, nlin='exp', bias_mu=3.0)
    try:
        x0 = popn.sample(np.random.RandomState(97))
        prms = cd.prep_first_order_glm_inference(popn)
        hessp = cd.prep_second_order_glm_inference(popn)
        for n in range(2):
            nv_b = popn.extract_vars(copy.deepcopy(x0), n)
            res_b = cd.fit_glm(nv_b, n, prms)
            res_b2 = cd.fit_glm(nv_b, n, prms)                 # restart from BFGS's own optimum
            slack = max(res_b.fun - res_b2.fun, np.spacing(abs(res_b.fun)))
            nv_n = popn.extract_vars(copy.deepcopy(x0), n)
            res_n = cd.fit_glm(nv_n, n, prms, use_rop=True, hessp=hessp)
            print("neuron %d: BFGS nlp %.12g (nit %d, restart finds %.3e), Newton-CG nlp %.12g (nit %d, nhev %d, success %s: %s); "
                  "slack %.3e" % (n, res_b.fun, res_b.nit, res_b.fun - res_b2.fun, res_n.fun, res_n.nit, res_n.nhev,
                                  res_n.success, res_n.message, slack))
            assert res_n.success, res_n.message
            # measured (MI355X, this test): the restarted BFGS finds no decrease on either neuron (0.0), so the slack is
            # the f64 spacing at |nlp| ~ 2.4e3 = 4.5e-13; BFGS -2378.64925953 in 39 iterations, Newton-CG
            # -2378.64925953 in 11 iterations and 23 products (neuron 1: 38 against 12 iterations, 20 products)
            assert res_n.fun <= res_b.fun + 10.0 * slack
    finally:
        popn.release_data()
