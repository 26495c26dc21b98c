"""CPU tests of the dense-mass HMC chain's core (theano_pyglm_amd/csrc/pglm_hmc_dense.h, compiled for the host with gcc
through tests/csrc/hmc_dense_host.c, tests/hmc_dense_mirror.py, numpy supplying ll and its gradient) and of the host
factorisation of inference/batched_hmc.py: the whitened chain on N(mu, Sigma) IS the identity-mass chain on the standard
normal, a diagonal factor IS the diagonal chain, the factor helper's accuracy and refusals, and the invariant law on a
strongly correlated Gaussian.  No GPU needed."""
import numpy as np
import pytest

from tests import hmc_mirror as HM
from tests import hmc_dense_mirror as HD
from theano_pyglm_amd.inference import batched_hmc as B

SC = HM.SC
U = np.finfo(float).eps / 2.0


def _spd(P, cond, rng):
    """A random symmetric positive definite matrix with the given condition number."""
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    S = (Q * np.logspace(0.0, -np.log10(cond), P)).dot(Q.T)
    return 0.5 * (S + S.T)


def _gauss_target(mu, prec):
    """ll and gradient of N(mu_m, prec_m^-1), row by row."""
    def target(X):
        d = X - mu
        g = -np.einsum('mij,mj->mi', prec, d)
        return 0.5 * np.einsum('mi,mi->m', d, g), g
    return target


def _std_normal(X):
    return -0.5 * np.sum(X * X, axis=1), -X


def test_mirror_products_read_the_lower_triangle_only():
    rng = np.random.default_rng(3)
    M, P = 2, 9
    W = rng.standard_normal((M, P, P))
    x = rng.standard_normal((M, P))
    Wn = W.copy()
    Wn[:, np.triu_indices(P, 1)[0], np.triu_indices(P, 1)[1]] = np.nan
    L = np.tril(W)
    for trans in (0, 1):
        ref = np.einsum('mji,mj->mi' if trans else 'mij,mj->mi', L, x)
        y = HD.tri_matvec(Wn, x, trans)
        assert np.all(np.isfinite(y)) and np.allclose(y, ref, rtol=0.0, atol=1e-13)


def test_whitened_chain_on_a_gaussian_is_the_identity_chain_on_the_standard_normal():
    """P = 7, cond(Sigma) = 1e4, W = chol(Sigma): u = W^-1 (q - mu) follows the identity-mass chain on N(0, I) -- the same
    draws, the same energies, so the same decisions; positions agree to 1e-10."""
    rng = np.random.default_rng(11)
    M, P, L, n_trans, n_warm = 2, 7, 4, 12, 5
    Sig = np.array([_spd(P, 1e4, rng) for _ in range(M)])
    assert 0.5e4 < np.linalg.cond(Sig[0]) < 2e4
    mu = rng.standard_normal((M, P))
    W = np.linalg.cholesky(Sig)
    prec = np.linalg.inv(Sig)
    u0 = rng.standard_normal((M, P))
    q0 = mu + np.einsum('mij,mj->mi', W, u0)
    dense = HD.DenseMirror(_gauss_target(mu, prec), q0, W, step0=0.9, seed=5)
    ident = HM.Mirror(_std_normal, u0, step0=0.9, seed=5)
    sd, ad, md = dense.run(n_trans, L, n_warm)
    si, ai, mi = ident.run(n_trans, L, n_warm)
    print("accepted %d of %d, smallest margin %.3e" % (ai.sum(), ai.size, mi.min()))
    assert mi.min() > 1e-6 and ai.any() and not ai.all()
    assert np.array_equal(ad, ai)
    u = np.array([[np.linalg.solve(W[m], sd[t, m] - mu[m]) for m in range(M)] for t in range(n_trans)])
    err = np.max(np.abs(u - si))
    print("largest |W^-1 (q - mu) - u| = %.3e" % err)
    assert err <= 1e-10
    assert np.array_equal(dense.sc[SC['step']], ident.sc[SC['step']])
    assert np.array_equal(dense.sc[SC['t']], ident.sc[SC['t']])


def test_diagonal_factor_is_the_diagonal_chain():
    """W = diag(sqrt(minv)) against HM.Mirror(minv=minv) on a correlated Gaussian likelihood under the row priors (both
    kinds): equal decisions, samples to 1e-10 of the row's largest entry."""
    rng = np.random.default_rng(17)
    M, N, Bn, D = 3, 2, 2, 2
    P = 1 + D + N * Bn
    prec = np.linalg.inv(np.array([_spd(P, 50.0, rng) for _ in range(M)]))
    mu = rng.standard_normal((M, P))
    minv = 0.25 + 1.5 * rng.random((M, P))
    W = np.zeros((M, P, P))
    W[:, np.arange(P), np.arange(P)] = np.sqrt(minv)
    X0 = mu + 0.3 * rng.standard_normal((M, P))
    for kind in (0, 1):
        prior = (kind, N, Bn, D, (0.5, 1.0, 1.0, 0.0, 2.0, 3.0))
        dense = HD.DenseMirror(_gauss_target(mu, prec), X0, W, n_lo=2, prior=prior, step0=0.15, seed=3)
        diag = HM.Mirror(_gauss_target(mu, prec), X0, n_lo=2, prior=prior, step0=0.15, seed=3, minv=minv)
        sd, ad, md = dense.run(10, 3, 4)
        sg, ag, mg = diag.run(10, 3, 4)
        print("kind %d: accepted %d of %d, smallest margin %.3e" % (kind, ag.sum(), ag.size, mg.min()))
        assert mg.min() > 1e-6 and ag.any() and not ag.all()
        assert np.array_equal(ad, ag)
        err = np.max(np.abs(sd - sg) / np.max(np.abs(sg), axis=2, keepdims=True))
        print("kind %d: largest error relative to the row's largest entry %.3e" % (kind, err))
        assert err <= 1e-10
        assert np.allclose(dense.sc[SC['step']], diag.sc[SC['step']], rtol=1e-15, atol=0.0)
        assert np.array_equal(dense.sc[SC['n_accept']], diag.sc[SC['n_accept']])


def test_factor_helper():
    """W W^T reproduces Sigma entry by entry to 8 (P + 1) u sqrt(Sigma_ii Sigma_jj): the componentwise backward error of a
    Cholesky factorisation, |L L^T - A| <= gamma_{P+1} |L| |L|^T (Higham, Accuracy and Stability, thm 10.3) with
    (|L| |L|^T)_ij <= sqrt(a_ii a_jj), which the equilibration keeps on the scale of every entry.  It implies the bound
    c P u cond(Sigma) max|Sigma| for every condition number."""
    rng = np.random.default_rng(23)
    P = 40
    scale = np.logspace(-6.0, 3.0, P)[rng.permutation(P)]     # parameters on scales nine orders of magnitude apart
    for S in (_spd(P, 1e4, rng), _spd(P, 1e6, rng) * scale[:, None] * scale[None, :]):
        S = 0.5 * (S + S.T)
        W = B.factor_inverse_mass(S)
        assert W.shape == (P, P) and np.array_equal(W, np.tril(W)) and np.all(np.diag(W) > 0.0)
        d = np.sqrt(np.diag(S))
        resid = np.max(np.abs(W.dot(W.T) - S) / (d[:, None] * d[None, :]))
        print("cond %.2e: scaled |W W^T - Sigma| = %.3e (bound %.3e)" % (np.linalg.cond(S), resid, 8 * (P + 1) * U))
        assert resid <= 8 * (P + 1) * U
    S3 = np.array([_spd(5, 10.0, rng) for _ in range(3)])
    W3 = B.factor_inverse_mass(S3)
    assert W3.shape == (3, 5, 5) and W3.flags['C_CONTIGUOUS']
    for m in range(3):
        assert np.array_equal(W3[m], B.factor_inverse_mass(S3[m]))
    # a computed inverse is symmetric to rounding only: accepted
    A = _spd(12, 1e5, rng)
    B.factor_inverse_mass(np.linalg.inv(A))
    bad_pd = S3.copy()
    bad_pd[1] = -bad_pd[1]
    indef = np.array([[1.0, 2.0], [2.0, 1.0]])
    asym = S3[0].copy()
    asym[0, 1] += 1e-3
    nan = S3[0].copy()
    nan[2, 2] = np.nan
    for bad in (bad_pd, indef, asym, nan, np.ones(4), np.ones((2, 3)), np.ones((2, 3, 4)), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError):
            B.factor_inverse_mass(bad)


def test_invariant_law_on_a_strongly_correlated_gaussian():
    """rho = 0.99, 2 000 transitions with W = chol(Sigma): the sample mean and the sample second moments about the true mean
    lie within 4 Monte-Carlo standard errors, sd / sqrt(ESS) with the true sd of each statistic and
    effective_sample_size of its chain."""
    Sig = np.array([[1.0, 0.99 * 2.0], [0.99 * 2.0, 4.0]])
    mu = np.array([[1.0, -2.0]])
    W = B.factor_inverse_mass(Sig)[None]
    mir = HD.DenseMirror(_gauss_target(mu, np.linalg.inv(Sig)[None]), mu.copy(), W, step0=0.3, seed=0)
    s, a, _ = mir.run(2000, 5)
    x = s[:, 0, :]
    print("accept rate %.3f" % a.mean())
    assert a.mean() > 0.6
    d = x - mu[0]
    for j in range(2):
        se = np.sqrt(Sig[j, j] / B.effective_sample_size(x[:, j]))
        print("mean %d: %.4f (true %.1f, se %.4f)" % (j, x[:, j].mean(), mu[0, j], se))
        assert abs(x[:, j].mean() - mu[0, j]) <= 4.0 * se
    for i, j in ((0, 0), (0, 1), (1, 1)):
        prod = d[:, i] * d[:, j]
        sd = np.sqrt(Sig[i, i] * Sig[j, j] + Sig[i, j] ** 2)       # of a product of two jointly normal deviations
        se = sd / np.sqrt(B.effective_sample_size(prod))
        print("cov %d%d: %.4f (true %.4f, se %.4f)" % (i, j, prod.mean(), Sig[i, j], se))
        assert abs(prod.mean() - Sig[i, j]) <= 4.0 * se
