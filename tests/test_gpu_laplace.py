"""The host mirror of the dense Hessian (Population.compute_hessian) against the matrix of compute_hvp columns, and the
Laplace posterior (inference/laplace.py) of a fitted standard_glm."""
import numpy as np
import pytest

from tests.test_gpu_hvp import _std_population

pytestmark = pytest.mark.gpu


def test_compute_hessian_and_laplace_of_a_fitted_standard_glm():
    from theano_pyglm_amd.inference.coord_descent import coord_descent
    from theano_pyglm_amd.inference.laplace import laplace_glms
    from theano_pyglm_amd.utils.packvec import packdict, get_vars
    N = 4
    popn = _std_population(N, 3.0, 101)                         # nT = 3000
    try:
        x = coord_descent(popn, x0=popn.sample(np.random.RandomState(103)), maxiter=1)
        syms = popn.glm_syms()
        n = 2
        w0, shapes = packdict(get_vars(syms, x['glms'][n]))
        P = w0.size
        Hn = popn.compute_hessian(x, n)
        assert Hn.shape == (P, P)
        cols = np.stack([popn.compute_hvp(x, n, e) for e in np.eye(P)], axis=1)
        err = np.max(np.abs(Hn - cols)) / np.max(np.abs(cols))
        print("compute_hessian against %d compute_hvp columns: %.3e of the largest entry" % (P, err))
        assert err <= 1e-9
        Hall = popn.compute_hessian_packed(x)
        assert Hall.shape == (N, P, P) and np.max(np.abs(Hall[n] - Hn)) <= 1e-12 * np.max(np.abs(Hn))
        no_prior = popn.compute_hessian_packed(x, n, n + 1, include_prior=False)[0]
        assert np.allclose(Hn - no_prior, popn.glm.hess_log_prior(x['glms'][n]), rtol=1e-9, atol=1e-9 * np.max(np.abs(Hn)))

        res = laplace_glms(popn, x)
        assert len(res) == N
        lps, _ = popn.compute_lp_grad_packed(x)
        for m, r in enumerate(res):
            assert r['pd'] is True
            assert np.allclose(r['A'], -Hall[m], rtol=1e-12, atol=0.0)
            xm = get_vars(syms, x['glms'][m])
            assert np.shape(r['stderr']['bias']['bias']) == np.shape(xm['bias']['bias'])
            assert np.shape(r['stderr']['imp']['w_ir']) == np.shape(xm['imp']['w_ir'])
            assert np.all(r['stderr_vec'] > 0.0)
            assert np.allclose(r['chol'].dot(r['chol'].T), r['A'], rtol=1e-10, atol=1e-12 * np.max(np.abs(r['A'])))
            # (an inverse through a Cholesky factor: |cov A - I| <= c P u cond(A), Higham, Accuracy and Stability, ch. 14)
            resid = np.max(np.abs(r['cov'].dot(r['A']) - np.eye(P)))
            print("neuron %d: |cov A - I| = %.3e, cond(A) = %.3e" % (m, resid, np.linalg.cond(r['A'])))
            assert resid <= 8.0 * P * np.finfo(float).eps * np.linalg.cond(r['A'])
            sign, logdet = np.linalg.slogdet(r['A'])
            want = lps[m] + 0.5 * P * np.log(2 * np.pi) - 0.5 * logdet
            print("neuron %d: log posterior %.6f, log det A %.6f, log evidence %.6f" % (m, lps[m], logdet, r['log_evidence']))
            assert sign > 0 and abs(r['log_evidence'] - want) <= 1e-9 * max(1.0, abs(want))
        two = laplace_glms(popn, x, 1, 3)
        assert len(two) == 2 and two[0]['log_evidence'] == res[1]['log_evidence']
    finally:
        popn.release_data()
