"""Stimulus decoding on the device (pgl_decode_*; csrc/pglm_decode.hip.h): the kernels against the longdouble reference over the
whole case table within the derived bound (tests/decode_reference.py), repeatability and independence of the launch cut bit for
bit, the ties to the existing ll+grad path on a population built through add_data, the end-to-end decode of a simulated
recording, and what is not served."""
import functools

import numpy as np
import pytest

from tests import decode_reference as DR
from tests import helpers as H
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu


def _handle(name):
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    d = _lib.DeviceGlm(c['N'], c['nT'], DR.B_IMP, DR.R_IMP, c['nlin'], DR.DT)
    d.set_spikes(m['S'])
    d.set_basis(m['ib_imp'])
    d.set_stimulus(np.zeros((c['Tu'], c['D'])), c['q'] * DR.DT, m['basis'], None, layout=1)
    return d


def _run(d, name):
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    d.decode_prepare(m['theta'], m['Weff'])
    F, g = d.decode_eval(m['u'], c['q'], DR.prior_of(c))
    return dict(F=F, g=g, hv1=d.decode_hvp(m['v1']), hv2=d.decode_hvp(m['v2']))


@functools.lru_cache(maxsize=None)
def _device(name):
    """the device's results of a case: a first run, a second run, and a run at another launch cut"""
    d = _handle(name)
    try:
        first = _run(d, name)
        second = _run(d, name)
        d.set_option(_lib.OPT_DECODE_CUT, 3)
        cut = _run(d, name)
    finally:
        d.close()
    return first, second, cut


@pytest.mark.parametrize('name', DR.NAMES)
def test_kernels_within_the_bound_of_the_reference(name):
    ref = DR.reference(name)
    r = _device(name)[0]
    ratios = [DR.check(r['F'][0], ref, 'F', 'device ' + name), DR.check(r['F'][1], ref, 'll', 'device ' + name),
              DR.check(r['F'][2], ref, 'lp', 'device ' + name), DR.check(r['g'], ref, 'g', 'device ' + name),
              DR.check(r['hv1'], ref, 'hv1', 'device ' + name), DR.check(r['hv2'], ref, 'hv2', 'device ' + name)]
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize('name', DR.NAMES)
def test_two_calls_and_another_cut_give_the_same_bits(name):
    first, second, cut = _device(name)
    for key in ('F', 'g', 'hv1', 'hv2'):
        assert first[key].tobytes() == second[key].tobytes(), key
        assert first[key].tobytes() == cut[key].tobytes(), key


def test_eval_without_gradient_and_dev_forms():
    """decode_eval(want_grad=False) gives the same F; the device-pointer forms give the bits of the host forms."""
    import torch
    name = 'n3_q4_high'
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    first = _device(name)[0]
    d = _handle(name)
    try:
        d.decode_prepare(m['theta'], m['Weff'])
        F, g = d.decode_eval(m['u'], c['q'], DR.prior_of(c), want_grad=False)
        assert g is None and F.tobytes() == first['F'].tobytes()
        dev = torch.device('cuda', 0)
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        d_theta, d_Weff, d_u, d_v = t(m['theta']), t(m['Weff']), t(m['u']), t(m['v1'])
        d_F = torch.empty(3, dtype=torch.float64, device=dev)
        d_g, d_hv = torch.empty_like(d_u), torch.empty_like(d_u)
        d.decode_prepare_dev(d_theta, d_Weff)
        d.decode_eval_dev(d_u, c['Tu'], c['q'], DR.prior_of(c), d_F, d_g)
        d.decode_hvp_dev(d_v, d_hv)
        d.sync()
        assert d_F.cpu().numpy().tobytes() == first['F'].tobytes()
        assert d_g.cpu().numpy().tobytes() == first['g'].tobytes()
        assert d_hv.cpu().numpy().tobytes() == first['hv1'].tobytes()
    finally:
        d.close()


# ---- ties to the existing path ---------------------------------------------------------------------------------------------------
def _basis_population(N, T, seed, dt_stim=0.1, D=2, dt_max=0.3, nlin=None, stim=None, S=None):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    model['bkgd'] = {'type': 'basis', 'D_stim': D, 'dt_max': dt_max, 'basis': model['bkgd']['basis']}
    if nlin:
        model['nonlinearity']['type'] = nlin
    popn = Population(model)
    nT = int(round(T / 0.001))
    rng = np.random.default_rng(seed)
    if S is None:
        S = np.minimum(rng.poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    if stim is None:
        stim = rng.standard_normal((int(round(T / dt_stim)), D))
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': stim, 'dt_stim': dt_stim})
    return popn


def _params(popn, seed, w_scale):
    x = popn.sample(np.random.RandomState(seed))
    rng = np.random.default_rng(seed + 1)
    for n in range(popn.N):
        x['glms'][n]['bkgd']['w_stim'] = w_scale * rng.standard_normal(np.size(x['glms'][n]['bkgd']['w_stim']))
    return x


def test_ties_to_the_ll_grad_path():
    """At u = the recorded stimulus the likelihood part of F is sum_n ll_n of pgl_ll_grad (rtol 1e-10, the project's ll parity
    tolerance), and by bilinearity of the stimulus current in (u, w_stim): <g_u^lik, u> = sum_n <d ll_n / d w_stim_n, w_stim_n>,
    to 1e-9 of the sum of the absolute terms (the project's gradient parity tolerance)."""
    popn = _basis_population(4, 6.0, 73)
    try:
        x = _params(popn, 79, 2.0)
        u = np.asarray(popn._current['stim'], dtype=float)
        mu, sigma = 0.25, 1.5
        F, g = popn.compute_stimulus_ll_grad(x, u, mu=mu, sigma=sigma)
        ll, g_theta = popn.compute_ll_grad(x)
        print('log_lik %.12f  sum ll_n %.12f' % (F[1], np.sum(ll)))
        assert abs(F[1] - np.sum(ll)) <= 1e-10 * abs(np.sum(ll))
        g_lik = g + (u - mu) / sigma ** 2                       # the iid prior's gradient taken off again
        theta = popn.theta_matrix(x)
        Dst = popn.glm.Dstim
        lhs_terms, rhs_terms = g_lik * u, g_theta[:, 1:1 + Dst] * theta[:, 1:1 + Dst]
        scale = np.sum(np.abs(lhs_terms)) + np.sum(np.abs(rhs_terms))
        print('<g_u, u> %.12e  sum <g_w, w> %.12e  scale %.3e' % (np.sum(lhs_terms), np.sum(rhs_terms), scale))
        assert abs(np.sum(lhs_terms) - np.sum(rhs_terms)) <= 1e-9 * scale
        # the product through the population: H is symmetric, <H v, w> = <v, H w>, held like the gradient identity above
        rng = np.random.default_rng(5)
        v, w = rng.standard_normal(u.shape), rng.standard_normal(u.shape)
        hv = popn.compute_stimulus_hvp(x, u, v, mu=mu, sigma=sigma)
        hw = popn.compute_stimulus_hvp(x, u, w, mu=mu, sigma=sigma)
        scale = np.sum(np.abs(hv * w)) + np.sum(np.abs(v * hw))
        print('<Hv, w> %.12e  <v, Hw> %.12e  scale %.3e' % (np.sum(hv * w), np.sum(v * hw), scale))
        assert np.all(np.isfinite(hv)) and np.max(np.abs(hv)) > 0
        assert abs(np.sum(hv * w) - np.sum(v * hw)) <= 1e-9 * scale
    finally:
        popn.release_data()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q', [1, 10])
def test_decode_a_simulated_recording(q):
    """N = 5, nT = 3000, D = 1, Rt = 20: spikes simulated from a seeded stimulus with the library's simulator on the host."""
    from theano_pyglm_amd.inference.decode import decode_stimulus, numpy_problem
    N, T, dt = 5, 3.0, 0.001
    dt_stim = q * dt
    rng = np.random.default_rng(100 + q)
    Tu = int(round(T / dt_stim))
    stim = np.repeat(rng.standard_normal((Tu // 5 + 1, 1)), 5, axis=0)[:Tu]          # steps of five frames
    gen = _basis_population(N, T, 7, dt_stim=dt_stim, D=1, dt_max=0.02, stim=stim)
    try:
        assert gen.glm.bkgd_model.ibasis.shape[0] == 20
        x = _params(gen, 11, 6.0)
        S, _ = gen.simulate(x, (0.0, T), dt, stim, dt_stim, rng=np.random.RandomState(3))
    finally:
        gen.release_data()
    popn = _basis_population(N, T, 7, dt_stim=dt_stim, D=1, dt_max=0.02, stim=stim, S=np.asarray(S)[:3000].astype(np.uint8))
    try:
        res = decode_stimulus(popn, x, sigma=1.0, rho=np.inf if q == 1 else 2.0)
        print(q, dict((k, v) for k, v in res.items() if k != 'stim'))
        assert res['status'] == 0 and res['grad_max'] <= 1e-5
        assert res['stim'].shape == (Tu, 1) and res['route'].startswith('device')
        rho = np.inf if q == 1 else 2.0
        F_rec = popn.compute_stimulus_ll_grad(x, stim, sigma=1.0, rho=rho)[0][0]
        print('F(decoded) %.9f  F(recorded) %.9f  corr %.3f' % (res['F'], F_rec, np.corrcoef(res['stim'][:, 0], stim[:, 0])[0, 1]))
        assert res['F'] >= F_rec
        # the numpy route reaches the same F: both ends at max |grad| <= 1e-8, F within the evaluation bound of the sum
        # (n_addends + A) 2^-53 sum |addends| times the number of evaluations
        tight = decode_stimulus(popn, x, sigma=1.0, rho=rho, gtol=1e-8)
        host = decode_stimulus(popn, x, sigma=1.0, rho=rho, gtol=1e-8, device=False)
        assert tight['status'] == 0 and host['status'] == 0 and host['route'] == 'numpy'
        prob, _, _ = numpy_problem(popn, x, 0.0, 1.0, rho)
        lam = prob.rate(prob.c + prob.conv(prob.L(host['stim'])))
        term_abs = np.abs(prob.S * np.log(np.maximum(lam, 1e-300))).sum() + prob.dt * lam.sum()
        n_add = 2 * prob.nT * prob.N + 2 * Tu
        bound = (n_add + DR.A) * DR.U * (term_abs + abs(host['log_prior'])) * max(tight['n_eval'], host['n_eval'])
        print('F device %.12f  F numpy %.12f  bound %.3e' % (tight['F'], host['F'], bound))
        assert abs(tight['F'] - host['F']) <= bound
    finally:
        popn.release_data()


# ---- what is not served ----------------------------------------------------------------------------------------------------------
def test_what_is_not_served_raises():
    p = H.Problem(8, 2000, H.std_ibasis(), seed=5)
    d = p.device(0)
    try:
        u = np.zeros((20, 2))
        with pytest.raises(_lib.PglError, match="error -4.*'basis' stimulus"):                       # no stimulus
            d.decode_prepare(p.theta, p.Weff)
            d.decode_eval(u, 100, (0.0, 1.0, np.inf))
        basis_t = H.std_ibasis(200)[:, :3]
        stim = np.random.default_rng(71).standard_normal((20, 2))
        d.set_stimulus(stim, 0.1, basis_t, None, layout=0)                                           # 'spatiotemporal', dense
        theta = np.zeros((8, d.P))
        with pytest.raises(_lib.PglError, match="error -4.*'basis' stimulus"):
            d.decode_prepare(theta, p.Weff)
            d.decode_eval(u, 100, (0.0, 1.0, np.inf))
        d.set_stimulus_separable(stim, 0.1, basis_t)                                                 # separable
        theta = np.zeros((8, d.P))
        with pytest.raises(_lib.PglError, match="error -4.*separable"):
            d.decode_prepare(theta, p.Weff)
            d.decode_eval(u, 100, (0.0, 1.0, np.inf))
        d.set_stimulus(stim, 0.1, basis_t, None, layout=1)
        theta = np.zeros((8, d.P))
        d.set_time_range(0, 1024)                                                                    # a time shard
        with pytest.raises(_lib.PglError, match="error -4.*time range"):
            d.decode_prepare(theta, p.Weff)
            d.decode_eval(u, 100, (0.0, 1.0, np.inf))
        d.set_time_range(0, 2000)
        with pytest.raises(_lib.PglError, match="error -3.*before pgl_decode_eval"):                 # a product without a point
            d.decode_hvp(u)
        with pytest.raises(_lib.PglError, match="error -1"):
            d.decode_prepare(theta, p.Weff)
            d.decode_eval(u, 0, (0.0, 1.0, np.inf))
        d.decode_prepare(theta, p.Weff)
        F, g = d.decode_eval(u, 100, (0.0, 1.0, np.inf))                                             # and the served form works
        assert np.all(np.isfinite(F)) and g.shape == u.shape
    finally:
        d.close()


def test_host_forms_check_the_shape_of_the_stimulus():
    """The host forms move Tu * D doubles each way: DeviceGlm and the library itself turn down an array of another shape, and
    Population a vector on a D = 2 model (it would become (Tu, 1))."""
    import ctypes as C
    name = 'n3_q4_high'                                   # D = 3
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    d = _handle(name)
    try:
        assert d.dec_D == 3
        d.decode_prepare(m['theta'], m['Weff'])
        with pytest.raises(ValueError, match=r"u must be \(Tu, D\) = \(Tu, 3\), got \(240, 1\)"):
            d.decode_eval(m['u'][:, :1], c['q'], DR.prior_of(c))
        with pytest.raises(ValueError, match=r"u must be \(Tu, D\)"):
            d.decode_eval(m['u'][:, 0], c['q'], DR.prior_of(c))
        F, g = d.decode_eval(m['u'], c['q'], DR.prior_of(c))
        with pytest.raises(ValueError, match=r"v must be \(Tu, D\) = \(240, 3\), got \(240, 2\)"):
            d.decode_hvp(m['v1'][:, :2])
        with pytest.raises(ValueError, match=r"v must be \(Tu, D\) = \(240, 3\), got \(100, 3\)"):
            d.decode_hvp(m['v1'][:100])
        # the library's own check, past the binding: nothing is copied
        u = np.ascontiguousarray(m['u'])
        out, F3 = np.full(u.shape, 7.0), np.empty(3)
        pr = _lib.as_decode_prior(DR.prior_of(c))
        rc = d.lib.pgl_decode_eval(d.h, _lib._ptr(u), u.shape[0], 1, c['q'], C.byref(pr), _lib._ptr(F3), _lib._ptr(out))
        assert rc == -1 and b"1 columns" in d.lib.pgl_last_error() and np.all(out == 7.0)
        rc = d.lib.pgl_decode_hvp(d.h, _lib._ptr(u), u.shape[0], 2, _lib._ptr(out))
        assert rc == -1 and b"2 columns" in d.lib.pgl_last_error() and np.all(out == 7.0)
        rc = d.lib.pgl_decode_hvp(d.h, _lib._ptr(u), 100, 3, _lib._ptr(out))
        assert rc == -1 and b"100 frames" in d.lib.pgl_last_error() and np.all(out == 7.0)
        assert d.decode_hvp(m['v1']).tobytes() == _device(name)[0]['hv1'].tobytes()
        d.set_stim_features(None)
        with pytest.raises(ValueError, match="needs a 'basis' stimulus on the handle"):
            d.decode_eval(m['u'], c['q'], DR.prior_of(c))
    finally:
        d.close()
    popn = _basis_population(4, 2.0, 3)                   # D = 2
    try:
        x = popn.sample(np.random.RandomState(1))
        with pytest.raises(ValueError, match=r"stim must be \(Tu, D\) with D = 2 stimulus dimensions, got \(20, 1\)"):
            popn.compute_stimulus_ll_grad(x, np.zeros(20))
        with pytest.raises(ValueError, match=r"v must be \(Tu, D\) with D = 2"):
            popn.compute_stimulus_hvp(x, np.zeros((20, 2)), np.zeros(20))
    finally:
        popn.release_data()


def test_population_turns_down_what_is_not_served():
    from theano_pyglm_amd.inference.decode import decode_stimulus
    from tests.test_gpu_hvp import _std_population
    plain = _std_population(4, 2.0, 3)
    try:
        x = plain.sample(np.random.RandomState(1))
        with pytest.raises(ValueError, match="not implemented for the NoStimulus background"):
            decode_stimulus(plain, x)
        with pytest.raises(ValueError, match="not implemented for the NoStimulus background"):
            plain.compute_stimulus_ll_grad(x, np.zeros((20, 1)))
    finally:
        plain.release_data()
    popn = _basis_population(4, 2.0, 3)
    try:
        x = popn.sample(np.random.RandomState(1))
        popn.set_time_shard(0, 2)
        with pytest.raises(ValueError, match="time-sharded population is not implemented"):
            decode_stimulus(popn, x)
        popn.set_time_shard(None)
        popn._current['dt_stim'] = 0.1 + 0.0004
        with pytest.raises(ValueError, match="integer multiple of dt"):
            decode_stimulus(popn, x)
    finally:
        popn.release_data()
