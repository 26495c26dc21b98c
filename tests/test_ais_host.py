"""CPU tests of the annealed importance sampling core (theano_pyglm_amd/csrc/pglm_ais.h over pglm_hmc.h, compiled for the
host with gcc through tests/csrc/ais_host.c, tests/ais_mirror.py, and driven with numpy supplying ll and its gradient):
the documented prior draw, the one-step ladder, the tempered target, an evidence known in closed form, a real likelihood
against an estimator that shares no code with AIS, dead particles, subsets and the frozen mode.  No GPU needed."""
import numpy as np

from tests import ais_mirror as AM
from tests.test_hmc_host import G, MASK, _key, _mix, _unif
from theano_pyglm_amd.inference import batched_ais as BA

SC = AM.SC
#          N  B  Dstim (mu_b, sg_b, stim_sigma, mu, sigma, lam)
PRIOR = (2, 2, 1, (0.5, 1.0, 0.5, -0.2, 2.0, 0.0))             # P = 6: [bias, one stimulus weight, w_ir (2, 2)]
P = 6


def prior_mean_sd(prior=PRIOR):
    N, B, D, (mu_b, sg_b, ss, mu, sg, _) = prior
    return (np.array([mu_b] + [0.0] * D + [mu] * (N * B)), np.array([sg_b] + [ss] * D + [sg] * (N * B)))


def doc_normal(seed, particle, n, t, j):
    """include/pyglm_hip.h: s_k = mix(seed + G (particle + 1)); key(s_k, n, t); Box-Muller on U(2 j + 1), U(2 j + 2)."""
    key = _key(_mix((seed + G * (particle + 1)) & MASK), n, t)
    return np.sqrt(-2.0 * np.log(_unif(key, 2 * j + 1))) * np.cos(np.float64(6.283185307179586) * _unif(key, 2 * j + 2))


def quadratic(a, d, c=0.0):
    """ll(x) = c - 1/2 sum_j d_j (x_j - a_j)^2 for the rows of one particle block; a, d (M, P), c (M,) or a number."""
    def target(X):
        return c - 0.5 * np.sum(d * (X - a) ** 2, axis=1), -d * (X - a)
    return target


def quad_params(seed, M=2):
    rng = np.random.default_rng(seed)
    m, s = prior_mean_sd()
    a = m + 0.7 * s * rng.standard_normal((M, P))
    d = (1.0 + 3.0 * rng.random((M, P))) / s ** 2              # the posterior is 1.4 to 2 times narrower than the prior
    return a, d, rng.standard_normal(M)


def quad_log_Z(a, d, c):
    """log of the integral of exp(ll) N(x; m, s^2): sum_j -1/2 log(1 + d s^2) - 1/2 d (m - a)^2 / (1 + d s^2), plus c."""
    m, s = prior_mean_sd()
    return c + np.sum(-0.5 * np.log1p(d * s * s) - 0.5 * d * (m - a) ** 2 / (1.0 + d * s * s), axis=1)


def test_prior_draw_is_the_documented_formula_and_the_prior():
    a, d, c = quad_params(1)
    m, s = prior_mean_sd()
    mir = AM.Mirror(quadratic(a[1:], d[1:]), 3, 1, PRIOR, n_lo=1, particle0=2, seed=77)
    for k in range(3):
        z = np.array([doc_normal(77, 2 + k, 1, 0, j) for j in range(P)])
        want = m + s * z
        err = np.max(np.abs(mir.draws[k] - want) / np.abs(want))
        print(k, mir.draws[k], err)
        assert err <= 1e-15
        assert abs(AM.lib().ais_normal(77, 2 + k, 1, 0, 3) - z[3]) <= 1e-15
    assert np.array_equal(mir.sc[SC['t']], np.ones(3)) and np.array_equal(mir.sc[SC['particle']], [2.0, 3.0, 4.0])
    K = 4000
    big = AM.Mirror(lambda X: (np.zeros(1), np.zeros((1, P))), K, 1, PRIOR, seed=5)
    mean, sd = big.draws.mean(axis=0), big.draws.std(axis=0, ddof=1)
    print(mean - m, sd - s)
    assert np.all(np.abs(mean - m) <= 5.0 * s / np.sqrt(K))
    assert np.all(np.abs(sd - s) <= 5.0 * s / np.sqrt(2.0 * K))


def test_one_step_ladder_weighs_the_draw():
    a, d, c = quad_params(2)
    tgt = quadratic(a, d, c)
    mir = AM.Mirror(tgt, 5, 2, PRIOR, seed=3)
    out = mir.run([0.0, 1.0], 1, 5)
    ll = np.array([tgt(mir.draws[k * 2:(k + 1) * 2])[0] for k in range(5)])
    assert np.array_equal(out['log_weights'], ll)               # (1 - 0) ll + 0, exactly
    assert np.array_equal(out['samples'].reshape(10, P), mir.draws)
    assert mir.n_evals == 1 and out['accepted'].size == 0


def test_tempering_recomputes_the_target_from_the_kept_parts():
    a, d, c = quad_params(3)
    base = quadratic(a, d, c)

    def tgt(X):
        ll, g = base(X)
        g[0, 2] = np.nan                                        # neuron 0: a gradient entry that is not a number
        return ll, g
    m, s = prior_mean_sd()
    betas = [0.0, 0.05, 0.3, 0.7, 1.0]
    seen = []

    def on_temper(j, mir):
        beta, sc = betas[j], mir.sc
        assert np.array_equal(sc[SC['beta']], np.full(mir.R, beta))
        assert np.array_equal(sc[SC['U0']], -(beta * sc[SC['ll0']] + sc[SC['lp0']]))
        lp = np.sum(-0.5 * ((mir.q - m) / s) ** 2, axis=1)
        assert np.allclose(sc[SC['lp0']], lp, rtol=1e-13, atol=0.0)
        ll, gll = np.zeros(mir.R), np.zeros((mir.R, P))
        for k in range(mir.K):
            ll[2 * k:2 * k + 2], gll[2 * k:2 * k + 2] = tgt(mir.q[2 * k:2 * k + 2].copy())
        assert np.array_equal(sc[SC['ll0']], ll)                # ll and grad ll AT THE CURRENT POINT, without an evaluation
        assert np.array_equal(np.isnan(mir.gll), np.isnan(gll)) and np.array_equal(np.nan_to_num(mir.gll), np.nan_to_num(gll))
        gu = -(beta * gll + -(mir.q - m) / s ** 2)
        gu[~np.isfinite(gu)] = 0.0
        assert np.all(gu[0::2, 2] == 0.0) and np.all(mir.g[0::2, 2] == 0.0)
        assert np.allclose(mir.g, gu, rtol=1e-13, atol=0.0)
        seen.append((j, mir.n_evals))
    mir = AM.Mirror(tgt, 3, 2, PRIOR, seed=11, step0=0.2)
    out = mir.run(betas, 2, 3, on_temper=on_temper)
    assert [j for j, _ in seen] == [1, 2, 3, 4]
    assert [e for _, e in seen] == [1, 7, 13, 19]               # 1 + (j - 1) n_steps n_leapfrog: a change of beta costs none
    assert out['accepted'].any()


def test_analytic_evidence():
    """Diagonal quadratic ll under the Gaussian priors, P = 6, K = 256, 20 temperatures, n_leapfrog = 5, pilot steps.
    Seeded on the CPU: |log_Z - exact| = (0.052, 0.019) against 4 se = (0.300, 0.319); ess = (105, 98) of 256."""
    a, d, c = quad_params(4)
    K = 256
    betas = np.linspace(0.0, 1.0, 20) ** 2
    out = AM.run_with_pilot(quadratic(a, d, c), K, 2, PRIOR, betas, 1, 5, step0=0.5, seed=1)
    log_Z, se, ess = BA.weights_summary(out['log_weights'])
    exact = quad_log_Z(a, d, c)
    print("log_Z", log_Z, "exact", exact, "|diff|", np.abs(log_Z - exact), "4 se", 4.0 * se, "ess", ess)
    assert np.all(ess >= K / 4.0)
    assert np.all(np.abs(log_Z - exact) <= 4.0 * se)


def test_real_likelihood_against_plain_importance_sampling():
    """The oracle's ll at N = 2, a two-column basis, nT = 600 (P = 5).  The reference value is plain importance sampling
    from a widened Gaussian at the mode (20 000 draws; its own standard error is asserted below 0.02), which shares no
    code with AIS.  Seeded on the CPU: log_Z AIS (20.317, 9.032) with se (0.061, 0.103), importance sampling (20.259, 9.105) with se
    0.0089; |difference| (0.057, 0.073) against 4 combined se (0.246, 0.414); ess (51.9, 38.3) of 64."""
    from scipy import optimize
    from oracle import c_oracle as CO
    from tests import helpers as H
    p = H.Problem(2, 600, H.std_ibasis()[:, :2], kind='explinear', seed=3)
    prior = (2, 2, 0, (20.0, 10.0, 1.0, 0.0, 2.0, 0.0))        # a bias prior wider than what 600 bins say about the rate
    m = np.array([20.0, 0.0, 0.0, 0.0, 0.0])
    s = np.array([10.0, 2.0, 2.0, 2.0, 2.0])
    fS = p.fS

    def target(X, n_lo=0, n_hi=2):
        return CO.ll_grad(p.S, fS, X, p.Weff, p.kind, p.dt, n_lo, n_hi)
    ll_np, g_np = p.oracle_ll_grad()
    ll_c, g_c = target(p.theta)
    assert np.allclose(ll_c, ll_np, rtol=1e-12) and np.allclose(g_c, g_np, rtol=1e-9, atol=1e-12)

    # the independent estimator, one neuron at a time, under the NORMALISED prior
    rng = np.random.default_rng(9)
    ref, ref_se = np.zeros(2), np.zeros(2)
    for n in range(2):
        def lpost(th):
            return target(th.reshape(1, 5), n, n + 1)[0] + np.sum(-0.5 * ((th.reshape(-1, 5) - m) / s) ** 2 - np.log(s * np.sqrt(2.0 * np.pi)), axis=1)

        def neg(th):
            ll, g = target(th.reshape(1, 5), n, n + 1)
            return -(ll[0] + np.sum(-0.5 * ((th - m) / s) ** 2)), -(g[0] - (th - m) / s ** 2)
        mode = optimize.minimize(neg, m.copy(), jac=True, method='BFGS', options={'gtol': 1e-8}).x
        h = 1e-4
        Hm = np.array([(neg(mode + h * e)[1] - neg(mode - h * e)[1]) / (2.0 * h) for e in np.eye(5)])
        cov = 1.5 ** 2 * np.linalg.inv(0.5 * (Hm + Hm.T))
        L = np.linalg.cholesky(cov)
        n_draws = 20000
        Z = rng.standard_normal((n_draws, 5))
        logq = -0.5 * np.sum(Z * Z, axis=1) - np.sum(np.log(np.diag(L))) - 2.5 * np.log(2.0 * np.pi)
        lw = np.array([lpost(mode + L.dot(z))[0] for z in Z]) - logq
        w = np.exp(lw - lw.max())
        ref[n] = lw.max() + np.log(w.mean())
        ref_se[n] = w.std(ddof=1) / (w.mean() * np.sqrt(n_draws))
    print("importance sampling: log_Z", ref, "se", ref_se)
    assert np.all(ref_se < 0.02)

    K = 64
    betas = np.linspace(0.0, 1.0, 20) ** 2
    out = AM.run_with_pilot(target, K, 2, prior, betas, 1, 5, step0=0.5, seed=2)
    log_Z, se, ess = BA.weights_summary(out['log_weights'])
    comb = np.sqrt(se ** 2 + ref_se ** 2)
    print("AIS: log_Z", log_Z, "se", se, "ess", ess, "|diff|", np.abs(log_Z - ref), "4 combined se", 4.0 * comb)
    assert np.all(ess >= K / 4.0)
    assert np.all(np.abs(log_Z - ref) <= 4.0 * comb)


def test_dead_particle_is_local_and_counts_in_K():
    a, d, c = quad_params(5)
    base = quadratic(a, d, c)
    betas = [0.0, 0.3, 1.0]
    alive = AM.Mirror(base, 4, 2, PRIOR, seed=21, step0=0.3)
    dead_row = 2 * 2 + 1                                        # particle 2 of neuron 1
    x_dead = alive.draws[dead_row].copy()
    ref = alive.run(betas, 2, 3)

    def tgt(X):
        ll, g = base(X)
        hit = np.all(X == x_dead, axis=1)
        ll[hit] = np.nan
        return ll, g
    mir = AM.Mirror(tgt, 4, 2, PRIOR, seed=21, step0=0.3)
    out = mir.run(betas, 2, 3)
    lw, lw0 = out['log_weights'].reshape(-1), ref['log_weights'].reshape(-1)
    others = np.arange(8) != dead_row
    assert lw[dead_row] == -np.inf and np.all(np.isfinite(lw[others]))
    assert np.array_equal(lw[others], lw0[others])
    assert np.array_equal(out['samples'].reshape(8, P)[others], ref['samples'].reshape(8, P)[others])
    log_Z, se, ess = BA.weights_summary(out['log_weights'])
    three = out['log_weights'][[0, 1, 3], 1]
    assert np.isclose(log_Z[1], np.log(np.sum(np.exp(three)) / 4.0), rtol=1e-14)      # K = 4: the dead one counts
    assert log_Z[0] == BA.weights_summary(ref['log_weights'])[0][0]
    all_dead = BA.weights_summary(np.full((3, 1), -np.inf))
    assert all_dead[0][0] == -np.inf and np.isnan(all_dead[1][0]) and all_dead[2][0] == 0.0


def test_subsets_and_repeats_give_equal_bits():
    a, d, c = quad_params(6, M=4)
    betas = [0.0, 0.1, 0.5, 1.0]
    table = np.array([[0.2, 0.3, 0.25, 0.35], [0.15, 0.2, 0.3, 0.1]])

    def run(K, n_lo, n_hi, particle0):
        mir = AM.Mirror(quadratic(a[n_lo:n_hi], d[n_lo:n_hi], c[n_lo:n_hi]), K, n_hi - n_lo, PRIOR, n_lo=n_lo, particle0=particle0,
                        seed=31)
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


def test_frozen_mode_uses_the_table_and_adapting_mode_the_rule():
    a, d, c = quad_params(7)
    betas = [0.0, 0.1, 0.5, 1.0]
    table = np.array([[0.2, 0.3], [0.15, 0.4]])
    mir = AM.Mirror(quadratic(a, d, c), 3, 2, PRIOR, seed=41, step0=0.05)
    steps_seen = []
    orig = mir.transition

    def transition(*args, **kw):
        steps_seen.append(mir.sc[SC['step']].copy())
        return orig(*args, **kw)
    mir.transition = transition
    out = mir.run(betas, 3, 3, adapt=False, step_table=table)
    assert np.array_equal(out['steps'], np.tile(table, (1, 3)))             # after every temperature's last transition
    assert np.array_equal(np.array(steps_seen), np.repeat(np.tile(table, (1, 3)), 3, axis=0))   # and before each one
    assert np.array_equal(mir.sc[SC['step']], np.tile(table[-1], 3))        # the last change gives no table row
    assert np.array_equal(mir.sc[SC['n_accept']], out['accepts'].sum(axis=0))
    # adapting: every decision moves the step by 2 %
    mir = AM.Mirror(quadratic(a, d, c), 1, 2, PRIOR, particle0=-1, seed=41, step0=0.05)
    out = mir.run(betas, 3, 3, adapt=True)
    assert np.all(out['steps'] != 0.05) and np.all(np.abs(np.log(out['steps'][0] / 0.05)) <= 3 * np.log(1.02) + 1e-12)
    assert np.array_equal(mir.sc[SC['particle']], [-1.0, -1.0])
