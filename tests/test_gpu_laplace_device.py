"""The device route of the Laplace posterior end to end (laplace_glms(device=True), sample_glms_hmc(factor_on_device=True))
against the host route on the small fitted population of tests/test_gpu_laplace.py (N = 4, 3 000 bins, the same spikes)
under a Gaussian(0, 1) prior on the impulse weights: under standard_glm's group-lasso prior the equilibrated matrix of that
fit has cond(C) = 7e15 (the norm's Hessian is flat along every group), which no bound of this kind survives.

Both routes factor the same A = minus the Hessian and both are backward stable, so they agree to c P u cond(C), C the
equilibrated matrix of the host route: the bound is 64 P 2^-53 cond(C) -- relative for the standard errors, absolute for
the log evidence, times sqrt(cov_ii cov_jj) for the covariance and times sqrt(cov_ii) for row i of the factor W of the
dense mass matrix -- and cond(C) <= 1e8 is asserted so that the bound cannot hide a failure."""
import numpy as np
import pytest

from tests import chol_cases as CC

pytestmark = pytest.mark.gpu

N = 4


def _population():
    """tests.test_gpu_hvp._std_population(4, 3.0, 101) with a Gaussian prior on the impulse weights."""
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    popn = Population(model)
    S = np.minimum(np.random.default_rng(101).poisson(20.0 * 0.001, size=(3000, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': 3.0, 'stim': None, 'dt_stim': 0.1})
    return popn


@pytest.fixture(scope='module')
def fitted():
    from theano_pyglm_amd.inference.coord_descent import coord_descent
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    x = coord_descent(popn, x0=popn.sample(np.random.RandomState(103)), maxiter=1)
    host = laplace_glms(popn, x)
    tol = []
    for r in host:
        cond = np.linalg.cond(CC.equilibrated(r['A'])[0])
        print("cond(C) = %.3e" % cond)
        assert r['pd'] and cond <= 1e8
        tol.append(64.0 * r['A'].shape[0] * CC.U * cond)
    yield popn, x, host, np.array(tol)
    popn.release_data()


def test_laplace_glms_device_against_host(fitted):
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn, x, host, tol = fitted
    dev = laplace_glms(popn, x, device=True, cov=True)
    assert len(dev) == N
    for m, (h, d) in enumerate(zip(host, dev)):
        assert d['pd'] is True and d['info'] == 0 and 'chol' not in d and 'A' not in d
        assert d['log_post'] == h['log_post']
        e_sd = np.max(np.abs(d['stderr_vec'] - h['stderr_vec']) / h['stderr_vec'])
        e_ev = abs(d['log_evidence'] - h['log_evidence'])
        sd = h['stderr_vec']
        e_cov = np.max(np.abs(d['cov'] - h['cov']) / (sd[:, None] * sd[None, :]))
        print("neuron %d: tol %.2e; stderr %.2e log evidence %.2e cov %.2e" % (m, tol[m], e_sd, e_ev, e_cov))
        assert e_sd <= tol[m] and e_ev <= tol[m] and e_cov <= tol[m]
        assert np.shape(d['stderr']['imp']['w_ir']) == np.shape(h['stderr']['imp']['w_ir'])
    plain = laplace_glms(popn, x, 1, 3, device=True)
    assert len(plain) == 2 and 'cov' not in plain[0] and plain[0]['log_evidence'] == dev[1]['log_evidence']
    more = laplace_glms(popn, x, 1, 2, device=True, extras=('A', 'chol'))[0]
    A = host[1]['A']
    assert np.allclose(more['A'], A, rtol=1e-12, atol=0.0)
    sd = np.sqrt(np.diag(A))
    P = A.shape[0]
    # (the factor bound of test_gpu_chol.py, plus the 1e-12 by which the two routes' A may differ: the line above)
    assert np.max(np.abs(more['chol'].dot(more['chol'].T) - A) / (sd[:, None] * sd[None, :])) <= (P + 8) * 2.0 ** -52 + 1e-12


def test_dense_mass_factor_on_device_against_host(fitted):
    from theano_pyglm_amd.inference import batched_hmc as BH
    popn, x, host, tol = fitted
    Wh, dense_h = BH._laplace_dense_factor(popn, x, 0, N, 1e-8)
    Wd, dense_d = BH._laplace_dense_factor_device(popn, x, 0, N, 1e-8)
    Wd = Wd.cpu().numpy()
    assert np.array_equal(dense_h, dense_d) and np.all(dense_d)
    for m in range(N):
        sd = np.sqrt(np.sum(Wh[m] ** 2, axis=1))
        err = np.max(np.abs(Wd[m] - Wh[m]) / sd[:, None])
        print("neuron %d: W differs by %.2e of sqrt(cov_ii), tol %.2e" % (m, err, tol[m]))
        assert err <= tol[m]
        assert np.all(Wd[m][np.triu_indices(Wd.shape[1], 1)] == 0.0)
    res = BH.sample_glms_hmc(popn, x, 5, n_warmup=5, n_leapfrog=3, mass='laplace_dense', factor_on_device=True, seed=3)
    assert res['samples'].shape[:2] == (5, N) and np.all(np.isfinite(res['samples']))
    assert np.all(res['dense_rows']) and popn.last_fit_stats['mass'] == 'dense'


def test_a_row_that_is_not_positive_definite_falls_back_on_both_routes(fitted, monkeypatch):
    from theano_pyglm_amd.inference import batched_hmc as BH
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn, x, host, tol = fitted
    orig = popn.glm.hess_log_prior
    bad = x['glms'][1]

    def patched(xn):
        Hn = np.array(orig(xn))
        if xn is bad:
            Hn[3, 3] += 1e9                                    # A_33 < 0: not a mode
        return Hn

    monkeypatch.setattr(popn.glm, 'hess_log_prior', patched)
    h = laplace_glms(popn, x)
    d = laplace_glms(popn, x, device=True, cov=True)
    assert [r['pd'] for r in h] == [r['pd'] for r in d] == [True, False, True, True]
    assert d[1]['info'] != 0 and np.isnan(d[1]['log_evidence'])
    assert np.all(np.isnan(d[1]['stderr_vec'])) and np.all(np.isnan(d[1]['cov']))
    for m in (0, 2, 3):
        assert np.max(np.abs(d[m]['stderr_vec'] - h[m]['stderr_vec']) / h[m]['stderr_vec']) <= tol[m]
    Wh, dense_h = BH._laplace_dense_factor(popn, x, 0, N, 1e-8)
    Wd, dense_d = BH._laplace_dense_factor_device(popn, x, 0, N, 1e-8)
    Wd = Wd.cpu().numpy()
    assert dense_h.tolist() == dense_d.tolist() == [True, False, True, True]
    assert np.array_equal(Wd[1] != 0.0, np.eye(Wd.shape[1], dtype=bool))
    assert np.allclose(Wd[1], Wh[1], rtol=1e-12, atol=0.0)     # the 'laplace' rule: diag sqrt(1 / max(A_ii, floor))
