"""CPU tests of the lock-step HMC chain's core (theano_pyglm_amd/csrc/pglm_hmc.h, compiled for the host with gcc through
tests/csrc/hmc_host.c, tests/hmc_mirror.py, and driven with numpy supplying ll and its gradient): the documented random
numbers, reversibility of the leapfrog, the transitions of inference/hmc.py: hmc_lockstep from the same momenta and
uniforms, the invariant law, the warm-up rule and the NaN rules; plus the host-only helpers of inference/batched_hmc.py.
No GPU needed."""
import numpy as np
import pytest

from tests import hmc_mirror as HM
from theano_pyglm_amd.inference import hmc as PH

SC = HM.SC
MASK = (1 << 64) - 1
G = 0x9e3779b97f4a7c15


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def _key(seed, n, t):
    return _mix((_mix((_mix((seed + G) & MASK) + G * (n + 1)) & MASK) + G * (t + 1)) & MASK)


def _unif(key, k):
    """include/pyglm_hip.h: U(k) = ((double)(mix(key + G (k + 1)) >> 11) + 0.5) * 2^-53, IEEE double operations."""
    z = _mix((key + G * (k + 1)) & MASK)
    return (np.float64(z >> 11) + np.float64(0.5)) * np.float64(2.0 ** -53)


def doc_uniform(seed, n, t):
    return _unif(_key(seed, n, t), 0)


def doc_normal(seed, n, t, j):
    key = _key(seed, n, t)
    return np.sqrt(-2.0 * np.log(_unif(key, 2 * j + 1))) * np.cos(np.float64(6.283185307179586) * _unif(key, 2 * j + 2))


def test_random_numbers_are_the_documented_formula():
    lib = HM.lib()
    cases = [(0, 0, 0, 0), (1, 2, 3, 4), (12345, 127, 999, 640), (2 ** 63 + 17, 5, 0, 1), (2 ** 64 - 1, 1023, 2 ** 20, 1220),
             (7, 0, 1, 0), (7, 1, 0, 0), (7, 0, 0, 1)]
    zs = []
    for seed, n, t, j in cases:
        z, u = lib.hmc_normal(seed, n, t, j), lib.hmc_uniform(seed, n, t)
        print(seed, n, t, j, z, z - doc_normal(seed, n, t, j), u - doc_uniform(seed, n, t))
        assert abs(z - doc_normal(seed, n, t, j)) <= 1e-15
        assert abs(u - doc_uniform(seed, n, t)) <= 1e-15
        assert 0.0 < u <= 1.0
        zs.append(z)
    assert len(set(zs)) == len(zs)                              # every index of the key matters
    # the draws are standard normal / uniform (a coarse check of the formula as a whole)
    z = np.array([lib.hmc_normal(3, 1, t, j) for t in range(200) for j in range(50)])
    u = np.array([lib.hmc_uniform(3, n, t) for n in range(100) for t in range(100)])
    assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / z.size)
    assert abs(u.mean() - 0.5) < 5.0 / np.sqrt(12.0 * u.size)


def _quadratic(A, m):
    """ll(x) = -1/2 (x - m)^T A (x - m) for every row (A (P,P) or (M,P,P))."""
    def target(X):
        D = X - m
        AD = np.einsum('...ij,...j->...i', A, D) if A.ndim == 2 else np.einsum('mij,mj->mi', A, D)
        return -0.5 * np.sum(D * AD, axis=1), -AD
    return target


def _spd(rng, P, lo=0.5, hi=3.0):
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    return (Q * np.linspace(lo, hi, P)).dot(Q.T)


def test_leapfrog_is_reversible():
    rng = np.random.default_rng(5)
    M, P, L = 2, 6, 7
    A = _spd(rng, P)
    minv = 0.5 + rng.random((M, P))
    X0 = rng.standard_normal((M, P))
    p0 = rng.standard_normal((M, P))
    mir = HM.Mirror(_quadratic(A, np.zeros(P)), X0, step0=0.05, seed=1, minv=minv)
    q1, acc, _ = mir.transition(L, p_in=p0)
    assert np.all(acc)                                          # (dH ~ 1e-4 at this step size)
    p1 = mir.p.copy()
    assert np.max(np.abs(q1 - X0)) > 0.05
    q2, acc, _ = mir.transition(L, p_in=-p1)
    assert np.all(acc)
    print("reversibility: |q - q0| = %.3e, |p + p0| = %.3e" % (np.max(np.abs(q2 - X0)), np.max(np.abs(mir.p + p0))))
    assert np.max(np.abs(q2 - X0)) <= 1e-12
    assert np.max(np.abs(mir.p + p0)) <= 1e-12


class _Replay(object):
    """rng stub for hmc_lockstep: replays the stateless draws of transition t for neurons n_lo .. n_lo + M - 1."""

    def __init__(self, seed, n_lo):
        self.lib, self.seed, self.n_lo, self.t = HM.lib(), seed, n_lo, 0

    def standard_normal(self, shape):
        M, d = shape
        return np.array([[self.lib.hmc_normal(self.seed, self.n_lo + r, self.t, j) for j in range(d)] for r in range(M)])

    def random_sample(self, M):
        return np.array([self.lib.hmc_uniform(self.seed, self.n_lo + r, self.t) for r in range(M)])


def test_transitions_equal_hmc_lockstep():
    """M = 3, d = 4 (bias, one stimulus weight, one presynaptic group of two), L = 3, Gaussian priors, a quadratic ll."""
    rng = np.random.default_rng(11)
    M, L, seed, n_lo, step = 3, 3, 77, 2, 0.9
    N, B, D = 1, 2, 1
    P = 1 + D + N * B
    mu_b, sg_b, s_stim, mu, sigma = -1.0, 2.0, 0.7, 0.3, 1.5
    A = np.array([_spd(rng, P) for _ in range(M)])
    m = rng.standard_normal((M, P))
    ll = _quadratic(A, m)

    def UG(Q):                                                  # numpy restatement of U = -(ll + log prior)
        l, g = ll(Q)
        mus = np.array([mu_b, 0.0, mu, mu])
        is2 = 1.0 / np.array([sg_b, s_stim, sigma, sigma]) ** 2
        lp = l + np.sum(-0.5 * is2 * (Q - mus) ** 2, axis=1)
        return -lp, -(g - (Q - mus) * is2)

    X0 = rng.standard_normal((M, P))
    mir = HM.Mirror(ll, X0, n_lo=n_lo, prior=(0, N, B, D, (mu_b, sg_b, s_stim, mu, sigma, 0.0)), step0=step, seed=seed)
    stub = _Replay(seed, n_lo)
    Q = X0.copy()
    n_acc = 0
    for t in range(12):
        stub.t = t
        Q, acc, _ = PH.hmc_lockstep(UG, step, L, Q, rng=stub)
        q, acc_m, _ = mir.transition(L)
        assert np.array_equal(acc, acc_m)
        print(t, acc, np.max(np.abs(q - Q)))
        assert np.max(np.abs(q - Q)) <= 1e-13
        n_acc += int(acc.sum())
    assert 0 < n_acc < 12 * M                                   # both outcomes of the decision
    assert mir.n_evals == 1 + 12 * L                            # the UG_curr shortcut: no evaluation at the start of a transition


def test_invariant_law_gaussian():
    """20 000 transitions on a 3-dimensional Gaussian with a non-diagonal covariance and a non-identity minv: mean and
    covariance within 5 Monte-Carlo standard errors, from the chain's own effective sample sizes."""
    from theano_pyglm_amd.inference.batched_hmc import effective_sample_size
    S = np.array([[1.0, 0.6, -0.3], [0.6, 2.0, 0.5], [-0.3, 0.5, 0.5]])
    mean = np.array([0.5, -1.0, 2.0])
    minv = np.array([[0.7, 1.6, 0.4]])
    mir = HM.Mirror(_quadratic(np.linalg.inv(S), mean), mean[None, :] + 0.1, step0=0.45, seed=2024, minv=minv)
    n = 20000
    samples, acc, _ = mir.run(n, 4)
    x = samples[:, 0, :]
    print("acceptance %.3f" % acc.mean())
    assert 0.6 < acc.mean() < 1.0
    for i in range(3):
        ess = effective_sample_size(x[:, i])
        se = np.sqrt(S[i, i] / ess)
        print("mean[%d] %.4f (true %.4f) ess %.0f se %.4f" % (i, x[:, i].mean(), mean[i], ess, se))
        assert ess > 500
        assert abs(x[:, i].mean() - mean[i]) <= 5.0 * se
    d = x - mean
    for i in range(3):
        for j in range(i, 3):
            y = d[:, i] * d[:, j]
            ess = effective_sample_size(y)
            se = np.sqrt((S[i, i] * S[j, j] + S[i, j] ** 2) / ess)          # variance of a product of Gaussians
            print("cov[%d,%d] %.4f (true %.4f) ess %.0f se %.4f" % (i, j, y.mean(), S[i, j], ess, se))
            assert ess > 500
            assert abs(y.mean() - S[i, j]) <= 5.0 * se


def test_warmup_follows_adapt_step_size_then_freezes():
    rng = np.random.default_rng(3)
    M, P, L, n_warmup = 3, 5, 3, 40
    A = _spd(rng, P, 0.5, 40.0)                                 # stiff enough for rejections at the larger steps
    mir = HM.Mirror(_quadratic(A, np.zeros(P)), rng.standard_normal((M, P)), step0=0.3, seed=9)
    step, avg = np.full(M, 0.3), np.full(M, 0.9)
    n_post = np.zeros(M)
    seen = set()
    for t in range(60):
        _, acc, _ = mir.transition(L, n_warmup=n_warmup)
        for r in range(M):
            if t < n_warmup:
                step[r], avg[r] = PH.adapt_step_size(step[r], avg[r], bool(acc[r]))
            else:
                n_post[r] += acc[r]
            seen.add(bool(acc[r]))
        assert np.array_equal(mir.sc[SC['step']], step), t
        assert np.array_equal(mir.sc[SC['avg_accept']], avg), t
        assert np.array_equal(mir.sc[SC['n_accept']], n_post)
        assert np.all(mir.sc[SC['t']] == t + 1)
    assert seen == {True, False}
    assert len(set(step)) > 1                                   # one step size per row
    # the clip at both ends
    for s0, lo in ((1.0, False), (1e-3, True)):
        tgt = _quadratic(A * (1e6 if lo else 1e-6), np.zeros(P))
        m2 = HM.Mirror(tgt, 1e-3 * rng.standard_normal((1, P)), step0=s0, seed=4)
        for t in range(30):
            m2.transition(L, n_warmup=1000)
            assert 1e-3 <= m2.sc[SC['step'], 0] <= 1.0
        assert m2.sc[SC['step'], 0] == (1e-3 if lo else 1.0)


def test_nan_rules():
    rng = np.random.default_rng(8)
    M, P, L = 2, 4, 3
    A = _spd(rng, P)
    base = _quadratic(A, np.zeros(P))
    X0 = rng.standard_normal((M, P))

    # a non-finite energy at the end of the trajectory rejects (row 0: -inf, nan and +inf ll in turn; row 1 untouched)
    for bad in (-np.inf, np.nan, np.inf):
        calls = [0]

        def tgt(X):
            ll, g = base(X)
            calls[0] += 1
            if calls[0] > 1:
                ll[0] = bad
            return ll, g
        mir = HM.Mirror(tgt, X0, step0=0.1, seed=5)
        ref = HM.Mirror(base, X0, step0=0.1, seed=5)
        for t in range(3):
            q, acc, _ = mir.transition(L)
            qr, accr, _ = ref.transition(L)
            assert not acc[0] and np.array_equal(q[0], X0[0])
            assert accr[1] == acc[1] and np.array_equal(q[1], qr[1])
        assert np.isfinite(mir.sc[SC['U0'], 0])

    # a NaN or infinite gradient entry counts as 0
    def tgt_nan(X):
        ll, g = base(X)
        g[:, 2] = np.nan
        g[0, 1] = np.inf
        return ll, g

    def tgt_zero(X):
        ll, g = base(X)
        g[:, 2] = 0.0
        g[0, 1] = 0.0
        return ll, g
    a, b = HM.Mirror(tgt_nan, X0, step0=0.1, seed=6), HM.Mirror(tgt_zero, X0, step0=0.1, seed=6)
    sa, acca, _ = a.run(4, L)
    sb, accb, _ = b.run(4, L)
    assert np.array_equal(sa, sb) and np.array_equal(acca, accb) and np.all(np.isfinite(sa))
    assert acca.any()

    # the group-lasso prior at an exactly zero group: its NaN derivative is 0, the chain goes on
    N, B = 2, 2
    Pg = 1 + N * B
    Ag = _spd(rng, Pg)
    Xg = rng.standard_normal((1, Pg))
    Xg[0, 1:3] = 0.0
    mg = HM.Mirror(_quadratic(Ag, np.zeros(Pg)), Xg, prior=(1, N, B, 0, (0.0, 1.0, 1.0, 0.0, 1.0, 2.0)), step0=0.1, seed=7)
    assert np.all(mg.g[0, 1:3] == 0.0) and np.all(mg.g[0, 3:] != 0.0)        # nan_to_num of the entries of grad (ll + log prior)
    sg, accg, _ = mg.run(5, L)
    assert np.all(np.isfinite(sg)) and accg.any()


def test_summarize_and_effective_sample_size():
    from theano_pyglm_amd.inference.batched_hmc import effective_sample_size, summarize
    rng = np.random.default_rng(21)
    n = 40000
    e = rng.standard_normal((n, 2, 3))
    x = np.empty_like(e)
    phi = 0.8
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + np.sqrt(1 - phi * phi) * e[i]
    x[:, 1, 2] = e[:, 1, 2]                                     # one white component
    s = summarize(x)
    assert s['mean'].shape == (2, 3) and s['ess'].shape == (2, 3)
    theory = n * (1 - phi) / (1 + phi)
    ar = np.delete(s['ess'].reshape(-1), 5)
    assert np.all(np.abs(ar / theory - 1.0) < 0.25), ar / theory
    assert abs(s['ess'][1, 2] / n - 1.0) < 0.1
    assert np.all(np.abs(s['mean']) < 5.0 / np.sqrt(ar.min())) and np.all(np.abs(s['sd'] - 1.0) < 0.05)
    assert np.all(np.abs(s['q025'] + 1.96) < 0.1) and np.all(np.abs(s['q975'] - 1.96) < 0.1)
    assert effective_sample_size(np.ones(100)) == 0.0
