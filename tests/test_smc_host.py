"""CPU tests of the adaptive sequential Monte Carlo core (theano_pyglm_amd/csrc/pglm_smc.h over pglm_ais.h, compiled for the
host with gcc through tests/csrc/smc_host.c, tests/smc_mirror.py, driven with numpy supplying ll and its gradient): one
particle, the bisection for the next temperature, dead particles, systematic resampling and what moves between slots, an
evidence known in closed form, neurons with different ladders, subsets and repeats, and the tempered factor with one
temperature per row.  No GPU needed."""
import numpy as np

from tests import smc_mirror as SM
from tests.ais_mirror import SC
from tests.test_ais_host import P, PRIOR, quad_log_Z, quad_params, quadratic
from tests.test_hmc_host import MASK, _key, _mix, _unif
from theano_pyglm_amd.inference import batched_ais as BA

NS = SM.NS


def _cess(W, ll0, d):
    v = np.exp(d * (ll0 - ll0[W > 0].max()))
    v[~(W > 0)] = 0.0
    return W.size * np.sum(W * v) ** 2 / np.sum(W * v * v)


def _set_ll0(mir, ll0, logw=None):
    """ll0 (K, M) (and logw) into the rows of a mirror, as if the draws had evaluated to them."""
    mir.sc[SC['ll0']] = np.asarray(ll0, dtype=float).reshape(-1)
    if logw is not None:
        mir.sc[SC['logw']] = np.asarray(logw, dtype=float).reshape(-1)


def test_one_particle_takes_one_stage_and_weighs_the_draw():
    a, d, c = quad_params(2)
    mir = SM.Mirror(quadratic(a, d, c), 1, 2, PRIOR, seed=3)
    out = mir.run()
    assert np.array_equal(out['log_Z'], mir.ll_draws)           # (1 - 0) ll + log 1, exactly
    assert np.array_equal(out['n_stages'], [1, 1]) and out['finished'].all() and mir.n_evals == 1
    assert np.array_equal(out['betas'], [[1.0, 1.0]]) and np.array_equal(out['samples'].reshape(2, P), mir.draws)


def test_bisection_meets_the_conditional_ess():
    rng = np.random.default_rng(0)
    K = 50
    ll0 = np.stack([-40.0 * rng.random(K), -1e-3 * rng.random(K), -4e8 * rng.random(K)], axis=1)
    mir = SM.Mirror(lambda X: (np.zeros(3), np.zeros((3, P))), K, 3, PRIOR, seed=1, cess=0.9, delta_min=1e-6)
    _set_ll0(mir, ll0)
    mir.stage()
    beta = mir.ns[NS['beta']]
    W = np.full(K, 1.0 / K)
    got = [_cess(W, ll0[:, i], beta[i]) for i in range(3)]
    print(beta, got, mir.rec[SM.REC['cess'], 0])
    assert 0.0 < beta[0] < 1.0 and abs(got[0] - 0.9 * K) <= 1e-9 * K
    assert abs(mir.rec[SM.REC['cess'], 0, 0] - got[0]) <= 1e-9 * K
    assert beta[1] == 1.0 and got[1] >= 0.9 * K and mir.ns[NS['done'], 1] == 1.0    # CESS(1 - beta) >= rho K: the jump
    assert beta[2] == 1e-6 and got[2] < 0.9 * K                                     # the floor is honoured
    logZ = np.log(np.mean(np.exp(beta[0] * ll0[:, 0])))
    assert abs(mir.ns[NS['log_Z'], 0] - logZ) <= 1e-12 * abs(logZ)
    lw = mir.sc[SC['logw']].reshape(K, 3)[:, 0]
    if mir.ns[NS['rs'], 0] == 0.0:
        assert abs(np.sum(np.exp(lw)) - 1.0) <= 1e-12


def test_dead_particles_weigh_nothing_and_an_all_dead_neuron_ends():
    rng = np.random.default_rng(1)
    K = 8
    ll0 = -3.0 * rng.random((K, 2))
    ll0[2, 0] = np.nan
    ll0[:, 1] = np.nan
    mir = SM.Mirror(lambda X: (np.zeros(2), np.zeros((2, P))), K, 2, PRIOR, seed=1, ess_min=0.0)
    logw = np.zeros((K, 2))
    logw[5, 0] = -np.inf
    _set_ll0(mir, ll0, logw)
    before = mir.q.copy()
    mir.stage()
    w = mir.w.reshape(K, 2)
    lw = mir.sc[SC['logw']].reshape(K, 2)
    assert w[2, 0] == 0.0 and w[5, 0] == 0.0 and lw[2, 0] == -np.inf and lw[5, 0] == -np.inf
    live = np.array([k for k in range(K) if k not in (2, 5)])
    assert abs(w[live, 0].sum() - 1.0) <= 1e-14
    beta = mir.ns[NS['beta'], 0]
    want = np.log(np.sum(np.exp(beta * ll0[live, 0])) / 6.0)    # the dead two had weight 0 before: 6 live shares of 1/6
    assert abs(mir.ns[NS['log_Z'], 0] - want) <= 1e-12 * max(1.0, abs(want))
    assert mir.ns[NS['log_Z'], 1] == -np.inf and mir.ns[NS['done'], 1] == 1.0 and mir.ns[NS['live'], 1] == 0.0
    assert np.all(w[:, 1] == 0.0) and np.array_equal(mir.q, before)
    out = mir.result()
    assert out['finished'][1] and out['log_Z'][1] == -np.inf


def _doc_uniform(seed, n, stage):
    """include/pyglm_hip.h: u = U_0 of key(mix(seed ^ 0x5eed5eed5eed5eed), n, stage)."""
    return _unif(_key(_mix((seed ^ 0x5eed5eed5eed5eed) & MASK), n, stage), 0)


def test_systematic_resampling_and_what_moves():
    a, d, c = quad_params(3)
    K, M = 16, 2
    mir = SM.Mirror(quadratic(a, d, c), K, M, PRIOR, n_lo=1, seed=9, step0=0.3, ess_min=1.0, cess=0.5, n_leapfrog=3)
    ident = dict((f, mir.sc[SC[f]].copy()) for f in ('seed_lo', 'seed_hi', 'particle', 't', 'neuron'))
    q0, gll0, ll00, lp00 = mir.q.copy(), mir.gll.copy(), mir.sc[SC['ll0']].copy(), mir.sc[SC['lp0']].copy()
    margins = mir.stage()                                       # ess_min = 1: every stage resamples
    assert np.all(mir.ns[NS['rs']] == 1.0) and np.all(margins[0] > 1e-9)
    w, anc = mir.w.reshape(K, M), mir.anc.reshape(K, M).astype(int)
    for i in range(M):
        u = _doc_uniform(9, 1 + i, 0)
        assert SM.lib().smc_uniform(9, 1 + i, 0) == u and 0.0 < u < 1.0
        want = np.searchsorted(np.cumsum(w[:, i]), (u + np.arange(K)) / K, side='left')
        assert np.array_equal(anc[:, i], want)
        n = np.bincount(anc[:, i], minlength=K)
        assert np.all(np.abs(n - K * w[:, i]) <= 1.0)
        rows, src = np.arange(K) * M + i, anc[:, i] * M + i
        assert np.array_equal(mir.q[rows], q0[src]) and np.array_equal(mir.gll[rows], gll0[src])
        assert np.array_equal(mir.sc[SC['ll0']][rows], ll00[src]) and np.array_equal(mir.sc[SC['lp0']][rows], lp00[src])
    assert np.all(mir.sc[SC['logw']] == 0.0)
    for f, v in ident.items():                                  # the slot keeps its identity
        assert np.array_equal(mir.sc[SC[f]], v)
    assert np.array_equal(mir.sc[SC['step']], np.tile(mir.ns[NS['step']], K))
    assert np.array_equal(mir.sc[SC['beta']], np.tile(mir.ns[NS['beta']], K))
    assert np.array_equal(mir.sc[SC['U0']], -(mir.sc[SC['beta']] * mir.sc[SC['ll0']] + mir.sc[SC['lp0']]))
    i = 0
    n = np.bincount(anc[:, i], minlength=K)
    j = int(np.argmax(n))
    assert n[j] >= 2
    twins = np.where(anc[:, i] == j)[0][:2] * M + i
    assert np.array_equal(mir.q[twins[0]], mir.q[twins[1]])
    mir.transition()
    assert not np.array_equal(mir.q[twins[0]], mir.q[twins[1]])  # copies of one ancestor diverge at the next momentum draw


def test_analytic_evidence():
    """Diagonal quadratic ll under the Gaussian priors, P = 6, M = 2, K = 64, 8 seeds, cess 0.9, n_leapfrog = 5, first step
    0.5.  Seeded on the CPU: mean log_Z (-4.061, -6.458) against exact (-4.013, -6.508); |difference| (0.048, 0.050) against
    4 standard errors of the mean (0.347, 0.117); 7 to 10 stages per neuron."""
    a, d, c = quad_params(4)
    runs = [SM.Mirror(quadratic(a, d, c), 64, 2, PRIOR, step0=0.5, seed=s, S=200).run() for s in range(8)]
    lz = np.array([r['log_Z'] for r in runs])
    assert all(r['finished'].all() for r in runs)
    mean, se = lz.mean(axis=0), lz.std(axis=0, ddof=1) / np.sqrt(8.0)
    exact = quad_log_Z(a, d, c)
    print("mean", mean, "exact", exact, "|diff|", np.abs(mean - exact), "4 se", 4.0 * se, [r['n_stages'] for r in runs])
    assert np.all(np.abs(mean - exact) <= 4.0 * se)


def test_neurons_with_different_ladders_and_done_rows_stay():
    a, d, c = quad_params(5)
    d[1] *= 30.0                                                # neuron 1: a much narrower posterior, a longer ladder
    mir = SM.Mirror(quadratic(a, d, c), 32, 2, PRIOR, step0=0.3, seed=2, S=200)
    kept = {}

    def on_stage(n, m):
        done = m.ns[NS['done']] != 0.0
        for i in np.where(done)[0]:
            rows = np.arange(m.K) * m.M + i
            snap = (m.st[:SM.NVEC * m.R * m.P].reshape(SM.NVEC, m.R, m.P)[:, rows].copy(), m.sc[:, rows].copy(),
                    m.ns[:6, i].copy())
            if i in kept:
                for x, y in zip(kept[i], snap):
                    assert np.array_equal(x, y, equal_nan=True)
            else:
                kept[i] = snap
    out = mir.run(on_stage=on_stage)
    print(out['n_stages'])
    assert out['finished'].all() and out['n_stages'][0] < out['n_stages'][1] and 0 in kept
    assert np.all(np.isnan(out['betas'][out['n_stages'][0]:, 0])) and not out['resampled'][out['n_stages'][0]:, 0].any()
    assert out['betas'][out['n_stages'][0] - 1, 0] == 1.0 and out['betas'][-1, 1] == 1.0


def test_subsets_and_repeats_give_equal_bits():
    a, d, c = quad_params(6, M=4)

    def run(n_lo, n_hi):
        return SM.Mirror(quadratic(a[n_lo:n_hi], d[n_lo:n_hi], c[n_lo:n_hi]), 16, n_hi - n_lo, PRIOR, n_lo=n_lo, step0=0.3,
                         seed=31, S=200).run()
    full, again, sub = run(0, 4), run(0, 4), run(1, 3)
    for key in ('log_Z', 'betas', 'ess', 'log_weights', 'samples', 'step_sz', 'accept_rate', 'resampled', 'n_stages'):
        assert np.array_equal(full[key], again[key], equal_nan=True)
    S = sub['betas'].shape[0]
    assert np.array_equal(sub['log_Z'], full['log_Z'][1:3]) and np.array_equal(sub['n_stages'], full['n_stages'][1:3])
    assert np.array_equal(sub['samples'], full['samples'][:, 1:3]) and np.array_equal(sub['log_weights'], full['log_weights'][:, 1:3])
    assert np.array_equal(sub['betas'], full['betas'][:S, 1:3], equal_nan=True)
    assert full['resampled'].any()


def test_tempered_factor_with_one_temperature_per_row():
    """tempered_factor_rows against tempered_factor called once per row, at the bound of tests/test_ais_dense_host.py:
    64 P 2^-53 cond(C), C the equilibrated A."""
    from theano_pyglm_amd.inference import laplace as LP
    rng = np.random.default_rng(3)
    M, Pn = 4, 9
    Bm = rng.standard_normal((M, Pn, 2 * Pn))
    G = np.einsum('mij,mkj->mik', Bm, Bm)
    lam = 0.5 + rng.random(Pn)
    betas = np.array([0.0, 1e-3, 0.3, 1.0])
    W, info = BA.tempered_factor_rows(G, lam, betas, 1e-8, LP.numpy_factor, LP.numpy_inverse, np, np.eye(Pn))
    assert np.all(info == 0)
    for i in range(M):
        Wi, _ = BA.tempered_factor(G[i:i + 1], lam, float(betas[i]), 1e-8, LP.numpy_factor, LP.numpy_inverse, np, np.eye(Pn))
        A = betas[i] * G[i] + np.diag(lam)
        s = 1.0 / np.sqrt(np.diag(A))
        tol = 64 * Pn * 2.0 ** -53 * np.linalg.cond(A * s[:, None] * s[None, :])
        err = np.max(np.abs(W[i] - Wi[0])) / np.max(np.abs(Wi[0]))
        print(i, err, tol)
        assert err <= tol


def test_real_likelihood_against_plain_importance_sampling():
    """The oracle's ll at N = 2, a two-column basis, nT = 600 (P = 5), the problem and the reference of
    tests/test_ais_host.py: plain importance sampling from a widened Gaussian at the mode (20 000 draws; its own standard
    error is asserted below 0.02), which shares no code with the sampler.  SMC gives no standard error from one run, so the
    bound has the form of that test's with the standard error of the mean over 8 seeds in the place of the AIS one:
    |mean log_Z - reference| <= 4 sqrt(se_mean^2 + se_ref^2), K = 64, cess 0.9, n_leapfrog = 5, first step 0.5.
    Seeded on the CPU: mean log_Z (20.262, 9.127) with se of the mean (0.053, 0.036), importance sampling (20.259, 9.105) with
    se 0.0089; |difference| (0.003, 0.023) against 4 combined se (0.215, 0.149); 2 to 4 stages per neuron."""
    from scipy import optimize
    from oracle import c_oracle as CO
    from tests import helpers as H
    p = H.Problem(2, 600, H.std_ibasis()[:, :2], kind='explinear', seed=3)
    prior = (2, 2, 0, (20.0, 10.0, 1.0, 0.0, 2.0, 0.0))
    m = np.array([20.0, 0.0, 0.0, 0.0, 0.0])
    s = np.array([10.0, 2.0, 2.0, 2.0, 2.0])
    fS = p.fS

    def target(X, n_lo=0, n_hi=2):
        return CO.ll_grad(p.S, fS, X, p.Weff, p.kind, p.dt, n_lo, n_hi)
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
        L = np.linalg.cholesky(1.5 ** 2 * np.linalg.inv(0.5 * (Hm + Hm.T)))
        n_draws = 20000
        Z = rng.standard_normal((n_draws, 5))
        logq = -0.5 * np.sum(Z * Z, axis=1) - np.sum(np.log(np.diag(L))) - 2.5 * np.log(2.0 * np.pi)
        lw = np.array([lpost(mode + L.dot(z))[0] for z in Z]) - logq
        w = np.exp(lw - lw.max())
        ref[n] = lw.max() + np.log(w.mean())
        ref_se[n] = w.std(ddof=1) / (w.mean() * np.sqrt(n_draws))
    print("importance sampling: log_Z", ref, "se", ref_se)
    assert np.all(ref_se < 0.02)
    runs = [SM.Mirror(target, 64, 2, prior, step0=0.5, seed=sd, S=400, n_leapfrog=5).run() for sd in range(8)]
    assert all(r['finished'].all() for r in runs)
    lz = np.array([r['log_Z'] for r in runs])
    mean, se = lz.mean(axis=0), lz.std(axis=0, ddof=1) / np.sqrt(8.0)
    comb = np.sqrt(se ** 2 + ref_se ** 2)
    print("SMC: mean log_Z", mean, "se of the mean", se, "|diff|", np.abs(mean - ref), "4 combined se", 4.0 * comb,
          "stages", [r['n_stages'] for r in runs])
    assert np.all(np.abs(mean - ref) <= 4.0 * comb)
