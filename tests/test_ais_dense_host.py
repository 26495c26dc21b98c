"""CPU tests of annealed importance sampling with a dense, tempered mass matrix (theano_pyglm_amd/csrc/pglm_ais_dense.h over
pglm_ais.h and pglm_hmc_dense.h, compiled for the host with gcc through tests/csrc/ais_dense_host.c, tests/ais_dense_mirror.py;
inference/batched_ais.py: tempered_factor on its numpy backend and the argument checks of ais_glms): a diagonal factor
against the diagonal mirror, an evidence known in closed form under the exact tempered mass, the tempered factors against
numpy.linalg, subsets and repeats, bad arguments.  No GPU needed."""
import numpy as np
import pytest

from tests import ais_mirror as AM
from tests import ais_dense_mirror as AD
from tests import chol_cases as CC
from tests.test_ais_host import P, PRIOR, prior_mean_sd, quad_log_Z, quad_params, quadratic
from theano_pyglm_amd.inference import batched_ais as BA
from theano_pyglm_amd.inference import laplace as LP


def _diag_stack(d):
    """(M, P) -> (M, P, P) diagonal matrices."""
    W = np.zeros(d.shape + (d.shape[1],))
    W[:, np.arange(d.shape[1]), np.arange(d.shape[1])] = d
    return W


def _factors(M, Pn, seed):
    """Random well-conditioned lower-triangular factors (tests/test_gpu_hmc_dense.py: _factor)."""
    rng = np.random.default_rng(seed)
    W = np.tril(rng.standard_normal((M, Pn, Pn)), -1) * (0.3 / np.sqrt(Pn))
    W[:, np.arange(Pn), np.arange(Pn)] = 0.7 + 0.6 * rng.random((M, Pn))
    return W


def _tempered(G, lam, beta, floor=1e-8):
    return BA.tempered_factor(G, lam, beta, floor, LP.numpy_factor, LP.numpy_inverse, np, np.eye(G.shape[1]))


def test_diagonal_factor_reproduces_the_diagonal_mirror():
    """W = diag(sqrt(minv)): the same decisions, accept counts and steps as tests/ais_mirror.py with minv -- frozen and
    adapting -- and points and log weights to rounding (the whitened run multiplies by sqrt(minv) twice where the diagonal
    one multiplies by minv once)."""
    a, d, c = quad_params(12)
    m, s = prior_mean_sd()
    minv = (0.5 + np.random.default_rng(13).random((2, P))) * s ** 2
    betas = [0.0, 0.05, 0.3, 0.7, 1.0]
    table = np.array([[0.3, 0.25], [0.2, 0.3], [0.25, 0.2]])
    for adapt in (False, True):
        kw = dict(adapt=adapt, step_table=None if adapt else table)
        ref = AM.Mirror(quadratic(a, d, c), 4, 2, PRIOR, seed=17, step0=0.3, minv=minv).run(betas, 3, 4, **kw)
        out = AD.DenseMirror(quadratic(a, d, c), 4, 2, PRIOR, _diag_stack(np.sqrt(minv)), seed=17, step0=0.3).run(betas, 3, 4, **kw)
        print("adapt %d: accepted %d of %d, smallest margin %.3e" % (adapt, ref['accepted'].sum(), ref['accepted'].size,
                                                                    ref['margins'].min()))
        assert ref['accepted'].any() and not ref['accepted'].all()
        assert np.array_equal(out['accepted'], ref['accepted']) and np.array_equal(out['accepts'], ref['accepts'])
        assert np.allclose(out['steps'], ref['steps'], rtol=1e-15, atol=0.0)
        err = np.max(np.abs(out['samples'] - ref['samples']) / np.max(np.abs(ref['samples']), axis=2, keepdims=True))
        werr = np.max(np.abs(out['log_weights'] - ref['log_weights']) / np.maximum(1.0, np.abs(ref['log_weights'])))
        print("points %.3e of the row's largest entry, log w %.3e" % (err, werr))
        assert err <= 1e-12 and werr <= 1e-12


def test_analytic_evidence_under_the_exact_tempered_mass():
    """The case of tests/test_ais_host.py: test_analytic_evidence (diagonal quadratic ll, P = 6, K = 256, 20 temperatures,
    n_leapfrog = 5, pilot steps, seed 1 -- the seed the diagonal reference test passes with), at that test's tolerance.
    G = diag(d) and Lambda = 1 / s^2, so the tempered mass IS the target's covariance at every temperature.
    The pilot starts at step 0.3, not that test's 0.5.  Under an exact mass every direction of the whitened target turns
    with period 2 pi, so a trajectory of length n_leapfrog x step = pi maps a point to its mirror image about the mean and
    keeps its distance from it: no mixing at all, and 5 x 0.5 .. 0.7 (the pilot's range over 18 transitions of 2 %) straddles
    pi.  A quarter period, pi / 2 = 5 x 0.31, replaces the point by the fresh momentum; the steps here span 5 x 0.3 .. 0.43.
    Run on the CPU with seed 1, this test and the reference test: both pass; here |log_Z - exact| = (0.012, 0.070) against
    4 se = (0.190, 0.169), ess = (162, 176) of 256 (the identity-mass reference: 105 and 98).  At step 0.5 the same run
    gives ess = (36, 119): the half-period trajectory, measured."""
    a, d, c = quad_params(4)
    m, s = prior_mean_sd()
    K = 256
    betas = np.linspace(0.0, 1.0, 20) ** 2
    G = _diag_stack(d)
    lam = BA.prior_precision((0,) + PRIOR[3], PRIOR[0], PRIOR[1], PRIOR[2])
    assert np.array_equal(lam, 1.0 / (s * s))

    def factors(j):
        W, info = _tempered(G, lam, betas[j])
        assert np.all(info == 0)
        return W
    out = AD.run_with_pilot(quadratic(a, d, c), K, 2, PRIOR, factors, betas, 1, 5, step0=0.3, seed=1)
    log_Z, se, ess = BA.weights_summary(out['log_weights'])
    exact = quad_log_Z(a, d, c)
    print("log_Z", log_Z, "exact", exact, "|diff|", np.abs(log_Z - exact), "4 se", 4.0 * se, "ess", ess)
    assert np.all(ess >= K / 4.0)
    assert np.all(np.abs(log_Z - exact) <= 4.0 * se)


@pytest.mark.parametrize('NBD', [(4, 3, 2), (8, 4, 0)])
def test_tempered_factors_against_numpy_linalg(NBD):
    """W_j W_j^T = (beta_j G + Lambda)^-1: the factor against numpy.linalg's route (the inverse by laplace_from_hessian,
    factored by factor_inverse_mass) and the residual W^T A W - I, at the bound of tests/test_laplace_device_host.py,
    64 P 2^-53 cond(C), C the equilibrated A (cond(C) <= 1e3 asserted).  At beta = 0, W = Lambda^-1/2 exactly, and the
    factorisation route gives the same diagonal matrix within 2 ulp; the per-element statements of csrc/pglm_ais_dense.h
    agree with the arrays."""
    from theano_pyglm_amd.inference.batched_hmc import factor_inverse_mass
    N, B, D = NBD
    Pn = 1 + D + N * B
    prm = (0, 0.5, 0.3, 2.0, -0.2, 0.1, 0.0)
    lam = BA.prior_precision(prm, N, B, D)
    assert lam.shape == (Pn,) and lam[0] == 1.0 / 0.09 and lam[-1] == 1.0 / (0.1 * 0.1) and (D == 0 or lam[1] == 0.25)
    G = CC.spd_stack(3, Pn, 7000 + Pn)
    iu = np.triu_indices(Pn, 1)
    for beta in (1e-4, 0.01, 0.3, 1.0):
        W, info = _tempered(G, lam, beta)
        assert np.all(info == 0)
        for mrow in range(3):
            A = beta * G[mrow] + np.diag(lam)
            cond = np.linalg.cond(CC.equilibrated(A)[0])
            assert cond <= 1e3
            tol = 64.0 * Pn * CC.U * cond
            host = LP.laplace_from_hessian(A, 0.0)
            assert host['pd']
            Wh = factor_inverse_mass(host['cov'])
            sd = np.sqrt(np.diag(host['cov']))
            errW = np.max(np.abs(W[mrow] - Wh) / sd[:, None])
            Ws = (W[mrow] / sd[:, None]).astype(np.longdouble)                  # W^T A W = I, scaled to the unit diagonal
            As = (A * sd[:, None] * sd[None, :]).astype(np.longdouble)
            res = float(np.max(np.abs(Ws.T.dot(As).dot(Ws) - np.eye(Pn))))
            print("P = %d beta = %g row %d: cond(C) = %.2e tol = %.2e; W %.2e residual %.2e" % (Pn, beta, mrow, cond, tol, errW, res))
            assert np.all(W[mrow][iu] == 0.0) and np.all(np.diag(W[mrow]) > 0.0)
            assert errW <= tol and res <= tol
            dg, fb = AD.tempered_diag(Pn, D, prm[1:], beta, np.diag(G[mrow]), 1e-8)
            assert np.allclose(dg, np.diag(A), rtol=4 * CC.U, atol=0.0) and np.allclose(fb, 1.0 / np.sqrt(np.diag(A)), rtol=8 * CC.U, atol=0.0)
    W0, info0 = _tempered(G, lam, 0.0)
    assert np.all(info0 == 0)
    assert np.array_equal(W0, np.broadcast_to(np.diag(1.0 / np.sqrt(lam)), W0.shape))
    route = LP.laplace_from_factor(np.broadcast_to(np.diag(lam), G.shape).copy(), LP.numpy_factor, LP.numpy_inverse, np)['W']
    off = route.copy()
    off[:, np.arange(Pn), np.arange(Pn)] = 0.0
    assert np.all(off == 0.0)
    assert np.allclose(np.diagonal(route, 0, 1, 2), 1.0 / np.sqrt(lam)[None], rtol=4 * CC.U, atol=0.0)


def test_a_row_that_does_not_factor_falls_back_alone():
    """A NaN Hessian and an indefinite one: those rows get diag(1 / sqrt(max(diag A, floor))) -- a non-finite or non-positive
    diagonal entry counting as floor -- and the other row's bits are those of the clean stack."""
    N, B, D = 2, 2, 1
    lam = BA.prior_precision((0, 0.5, 1.0, 0.5, -0.2, 2.0, 0.0), N, B, D)
    G = CC.spd_stack(3, 6, 31)
    clean, _ = _tempered(G, lam, 0.4)
    bad = G.copy()
    bad[0, 2, 3] = bad[0, 3, 2] = np.nan
    bad[0, 4, 4] = np.nan
    bad[2] = -bad[2]
    bad[2, 1, 1] = G[2, 1, 1]
    W, info = _tempered(bad, lam, 0.4, floor=1e-3)
    assert info[0] != 0 and info[1] == 0 and info[2] != 0
    assert np.array_equal(W[1], clean[1])
    for mrow in (0, 2):
        dg = 0.4 * np.diag(bad[mrow]) + lam
        want = 1.0 / np.sqrt(np.where(np.isfinite(dg) & (dg > 1e-3), dg, 1e-3))
        assert np.array_equal(W[mrow], np.diag(want)) and np.all(np.isfinite(W[mrow]))
        assert np.array_equal(AD.tempered_diag(6, D, (0.5, 1.0, 0.5, -0.2, 2.0, 0.0), 0.4, np.diag(bad[mrow]), 1e-3)[1], want)
    assert W[0][4, 4] == 1.0 / np.sqrt(1e-3) and np.any(W[2] == 1.0 / np.sqrt(1e-3))


def test_subsets_and_repeats_give_equal_bits():
    a, d, c = quad_params(6, M=4)
    betas = [0.0, 0.1, 0.5, 1.0]
    table = np.array([[0.2, 0.3, 0.25, 0.35], [0.15, 0.2, 0.3, 0.1]])
    Ws = [None, _factors(4, P, 51), _factors(4, P, 52)]          # one stack per temperature with moves

    def run(K, n_lo, n_hi, particle0):
        mir = AD.DenseMirror(quadratic(a[n_lo:n_hi], d[n_lo:n_hi], c[n_lo:n_hi]), K, n_hi - n_lo, PRIOR,
                             lambda j: Ws[j][n_lo:n_hi], n_lo=n_lo, particle0=particle0, seed=31)
        return mir.run(betas, 2, 3, step_table=table[:, n_lo:n_hi])
    full, again = run(3, 0, 4, 0), run(3, 0, 4, 0)
    for key in ('log_weights', 'samples', 'accepted'):
        assert np.array_equal(full[key], again[key])
    sub = run(3, 1, 3, 0)
    assert np.array_equal(sub['log_weights'], full['log_weights'][:, 1:3])
    assert np.array_equal(sub['samples'], full['samples'][:, 1:3])
    part = run(2, 0, 4, 1)
    assert np.array_equal(part['log_weights'], full['log_weights'][1:3])
    assert np.array_equal(part['samples'], full['samples'][1:3])
    assert full['accepted'].any() and len(set(full['log_weights'].reshape(-1))) == 12


def _gaussian_population(N=2):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    return Population(model)


def test_ais_glms_checks_its_mass_before_it_touches_a_device():
    """Bad strings, wrong shapes, matrices that are not symmetric positive definite and the group lasso raise ValueError, as
    they do for sample_glms_hmc and for the diagonal forms of ais_glms."""
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = _gaussian_population()
    x = popn.sample(np.random.RandomState(1))
    Pn = popn.glm.P
    eye = np.broadcast_to(np.eye(Pn), (2, Pn, Pn)).copy()
    for bad in ('dense', 'laplace-dense', ''):
        with pytest.raises(ValueError, match="laplace_dense"):
            BA.ais_glms(popn, x, 2, n_temps=5, mass=bad)
    not_pd, asym, nan = -eye, eye.copy(), eye.copy()
    asym[0, 0, 1] += 1.0
    nan[1, 2, 2] = np.nan
    for bad, msg in ((eye[:1], "inverse mass matrices"), (eye[:, :Pn - 1, :Pn - 1], "inverse mass matrices"),
                     (np.ones((2, Pn, Pn + 1)), "inverse mass matrices"), (not_pd, "positive definite"),
                     (asym, "symmetric"), (nan, "NaN")):
        with pytest.raises(ValueError, match=msg):
            BA.ais_glms(popn, x, 2, n_temps=5, mass=bad)
    with pytest.raises(ValueError, match="inverse mass matrices"):
        BA.ais_glms(popn, x, 2, n_temps=5, mass=eye, n_lo=1, n_hi=2)
    lasso = Population(make_model('standard_glm', N=2, dt=0.001))
    for mass in ('laplace_dense', eye):
        with pytest.raises(ValueError, match="Gaussian"):
            BA.ais_glms(lasso, lasso.sample(np.random.RandomState(1)), 2, n_temps=5, mass=mass)
