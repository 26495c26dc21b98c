"""GPU tests of the lock-step HMC chain (pgl_hmc_* row kernels, inference/batched_hmc.py): the device chain through the C
ABI against the host mirror of the same state machine (tests/hmc_mirror.py: csrc/pglm_hmc.h built by gcc) fed by the
oracle's ll and gradient, and the driver's contract (subset = batch, local rejection, mass matrix, launch counts,
unsupported inputs).

A decision log u < H0 - H1 is a discontinuity: the cases are seeded so that in the mirror every decision keeps
|log u - (H0 - H1)| > 1e-4 (asserted), far above the difference between the oracle's and the device's ll, so no
decision can flip and the kept samples agree to rounding."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import hmc_mirror as HM

GAUSS = (0, 20.0, 1.0, 1.0, 0.0, 2.0, 0.0)                   # (kind, mu_b, sg_b, stim_sigma, mu, sigma, lam)
LASSO = (1, 20.0, 1.0, 1.0, 0.0, 2.0, 3.0)
MARGIN = 1e-4


def mirror_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, minv=None, n_warmup=0):
    """The host mirror on the oracle: ll and its gradient summed over the problems (data sequences) `probs`.
    -> (samples (n_trans, M, P), accepted (n_trans, M), margins (n_trans, M), final scalar state)."""
    def target(X):
        ll, g = 0.0, 0.0
        for p in probs:
            p.theta = p.theta.copy()
            p.theta[n_lo:n_hi] = X
            a, b = p.oracle_ll_grad(n_lo, n_hi)
            ll, g = ll + a, g + b
        return ll, g
    p0 = probs[0]
    mir = HM.Mirror(target, X0, n_lo=n_lo, prior=(prm[0], p0.N, p0.B, p0.Dstim, prm[1:]), step0=step, seed=seed, minv=minv)
    s, a, m = mir.run(n_trans, L, n_warmup)
    return s, a, m, mir.sc.copy()


def device_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, minv=None, n_warmup=0):
    """The same chain through the C ABI; the scalar state is read after every transition (a test's privilege)."""
    import torch
    p0 = probs[0]
    M, P = X0.shape
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    hs = [p.device(0) for p in probs]
    stream = torch.cuda.Stream(dev)
    try:
        for h in hs:
            h.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            h0 = hs[0]
            st = torch.zeros(h0.hmc_state_doubles(M, P), dtype=f64, device=dev)
            assert st.numel() == 4 * M * P + 10 * M
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            sc = st[4 * M * P:].view(10, M)
            Weff = torch.tensor(p0.Weff, dtype=f64, device=dev)
            mv = torch.tensor(minv, dtype=f64, device=dev) if minv is not None else None
            mvp = mv.data_ptr() if mv is not None else 0
            Xt = torch.empty((M, P), dtype=f64, device=dev)
            bufs = [torch.empty(M * (1 + P), dtype=f64, device=dev) for _ in hs]
            samples = torch.zeros((n_trans, M, P), dtype=f64, device=dev)

            def evaluate(Xe):
                for h, b in zip(hs, bufs):
                    h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), b.data_ptr(), b[M:].data_ptr(), n_lo, n_hi)
                    if b is not bufs[0]:
                        bufs[0].add_(b)
                return bufs[0][:M], bufs[0][M:]

            ll, g = evaluate(st[:M * P].view(M, P))
            h0.hmc_init_dev(st.data_ptr(), M, P, n_lo, ll.data_ptr(), g.data_ptr(), prm, step, seed)
            acc = []
            for t in range(n_trans):
                h0.hmc_begin_dev(st.data_ptr(), M, P, mvp, Xt.data_ptr())
                for i in range(L):
                    ll, g = evaluate(Xt)
                    h0.hmc_leap_dev(st.data_ptr(), M, P, mvp, ll.data_ptr(), g.data_ptr(), prm, i == L - 1, n_warmup,
                                    Xt.data_ptr(), samples[t].data_ptr() if i == L - 1 else 0)
                stream.synchronize()
                acc.append(sc[HM.SC['acc']].cpu().numpy() != 0.0)
            stream.synchronize()
            return samples.cpu().numpy(), np.array(acc), sc.cpu().numpy()
    finally:
        for h in hs:
            h.close()


def compare(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, minv=None, n_warmup=0, label=""):
    sm, am, mm, scm = mirror_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, minv, n_warmup)
    print("%s mirror: accepted %d of %d, smallest margin %.3e" % (label, am.sum(), am.size, mm.min()))
    assert mm.min() > MARGIN                                    # the condition the case was seeded for
    assert am.any()
    sd, ad, scd = device_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, minv, n_warmup)
    assert np.array_equal(ad, am)
    err = np.max(np.abs(sd - sm) / np.max(np.abs(sm), axis=2, keepdims=True))
    print("%s device against mirror: largest error relative to the row's largest entry %.3e" % (label, err))
    assert err <= 1e-9
    assert np.array_equal(scd[HM.SC['t']], scm[HM.SC['t']]) and np.array_equal(scd[HM.SC['n_accept']], scm[HM.SC['n_accept']])
    assert np.allclose(scd[HM.SC['step']], scm[HM.SC['step']], rtol=1e-15, atol=0.0)
    return sm, am, sd, ad


CASES = {  # (nlin, prior) -> (step, seed): seeded on the CPU for a mix of decisions with margins > 1e-4
    ('explinear', 'gauss'): (1.0, 1),                           # mirror: 37 of 40 accepted, smallest margin 3.8e-3
    ('explinear', 'lasso'): (1.0, 3),                           # 28 of 40, 6.9e-4
    ('exp', 'gauss'): (0.2, 1),                                 # 28 of 40, 6.8e-2
    ('exp', 'lasso'): (0.2, 1),                                 # 23 of 40, 8.2e-2
}


def _problem(N, nT, kind, seed, ibasis=None):
    ib = H.std_ibasis() if ibasis is None else ibasis
    if kind == 'exp':
        return H.Problem(N, nT, ib, kind='exp', seed=seed, bias_mu=3.0, w_scale=0.05)
    return H.Problem(N, nT, ib, kind=kind, seed=seed)


def _prior(kind, name):
    prm = GAUSS if name == 'gauss' else LASSO
    return (prm[0], 3.0 if kind == 'exp' else 20.0) + prm[2:]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
@pytest.mark.parametrize('prior', ['gauss', 'lasso'])
def test_device_chain_equals_host_mirror(kind, prior):
    """N = 5, nT = 2 000, n_leapfrog = 3, 8 transitions."""
    p = _problem(5, 2000, kind, 31)
    step, seed = CASES[(kind, prior)]
    sm, am, _, _ = compare([p], p.theta.copy(), 0, 5, _prior(kind, prior), 8, 3, step, seed, label="%s/%s" % (kind, prior))
    assert not am.all()                                         # both outcomes of the decision


@pytest.mark.gpu
def test_strided_row_loops():
    """P = 281 > the 256 threads of a row kernel's workgroup: N = 70, B = 4, nT = 512, 2 transitions."""
    p = _problem(70, 512, 'explinear', 37, ibasis=H.std_ibasis()[:, :4])
    assert p.P == 281
    compare([p], p.theta.copy(), 0, 70, _prior('explinear', 'lasso'), 2, 3, 1.0, 2, label="N=70")


@pytest.mark.gpu
def test_subset_equals_batch_and_runs_repeat():
    p = _problem(5, 2000, 'explinear', 31)
    prm = _prior('explinear', 'gauss')
    step, seed = CASES[('explinear', 'gauss')]
    full, accf, _ = device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, step, seed, n_warmup=3)
    again, acca, _ = device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, step, seed, n_warmup=3)
    assert np.array_equal(full, again) and np.array_equal(accf, acca)
    sub, accs, _ = device_chain([p], p.theta[1:4].copy(), 1, 4, prm, 6, 3, step, seed, n_warmup=3)
    assert np.array_equal(sub, full[:, 1:4]) and np.array_equal(accs, accf[:, 1:4])
    assert accf.any() and np.any(full[-1] != p.theta)


@pytest.mark.gpu
def test_two_data_sequences_sum():
    """Two recordings of the same population: their [ll | grad] blocks are summed before the row kernel sees them."""
    p1 = _problem(5, 2000, 'explinear', 31)
    p2 = _problem(5, 1008, 'explinear', 41)
    p2.theta, p2.Weff = p1.theta, p1.Weff
    compare([p1, p2], p1.theta.copy(), 0, 5, _prior('explinear', 'gauss'), 4, 3, 1.0, 3, label="two sequences")


@pytest.mark.gpu
def test_mass_matrix_equals_mirror():
    p = _problem(5, 2000, 'explinear', 31)
    minv = 0.25 + 1.5 * np.random.default_rng(43).random((5, p.P))
    compare([p], p.theta.copy(), 0, 5, _prior('explinear', 'gauss'), 4, 3, 0.7, 1, minv=minv, n_warmup=2, label="minv")


# ---- the driver --------------------------------------------------------------------------------------------------
def _population(N=4, T=6.0, seed=89):
    from tests.test_gpu_hvp import _std_population
    return _std_population(N, T, seed, nlin='exp', bias_mu=3.0)


@pytest.mark.gpu
def test_driver_laplace_mass_launch_counts_and_helpers():
    from theano_pyglm_amd.inference import batched_hmc as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        x0 = copy.deepcopy(x)
        L, n_warm, n_s, thin = 4, 6, 5, 2
        out = B.sample_glms_hmc(popn, x, n_s, n_warmup=n_warm, n_leapfrog=L, step_sz=0.05, thin=thin, mass='laplace', seed=5)
        st = popn.last_fit_stats
        print(st, out['accept_rate'], out['step_sz'])
        P = popn.glm.P
        assert out['samples'].shape == (n_s, 4, P) and np.all(np.isfinite(out['samples']))
        assert np.all(out['accept_rate'] > 0.0) and np.all(out['accept_rate'] <= 1.0)
        assert np.all(out['step_sz'] >= 1e-3) and np.all(out['step_sz'] <= 1.0)
        n_total = n_warm + n_s * thin
        assert st['transitions'] == n_total
        assert st['evaluations_per_transition'] == L and st['row_launches_per_transition'] == L + 1
        assert out['n_evals'] == 1 + n_total * L == st['ll_grad_launches']
        assert st['host_syncs_in_chain'] == 0
        # x is untouched; a draw goes back into state dicts
        assert np.array_equal(popn.theta_matrix(x), popn.theta_matrix(x0))
        glms = B.samples_to_states(popn, x, out['samples'], 3)
        xx = dict(x)
        xx['glms'] = glms
        assert np.array_equal(popn.theta_matrix(xx), out['samples'][3])
        s = B.summarize(out['samples'])
        assert s['mean'].shape == (4, P) and s['ess'].shape == (4, P)
        # a subset of the neurons: the same rows (stateless draws keyed by the neuron)
        mass = B._laplace_minv(popn, x, 0, 4, 1e-8)
        full = B.sample_glms_hmc(popn, x, 3, n_warmup=2, n_leapfrog=L, step_sz=0.05, mass=mass, seed=5)
        sub = B.sample_glms_hmc(popn, x, 3, n_warmup=2, n_leapfrog=L, step_sz=0.05, mass=mass[1:3], seed=5, n_lo=1, n_hi=3)
        assert np.array_equal(sub['samples'], full['samples'][:, 1:3])
        assert np.array_equal(sub['step_sz'], full['step_sz'][1:3])
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_rejection_is_local():
    from theano_pyglm_amd.inference import batched_hmc as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        X0 = popn.theta_matrix(x)
        step = np.full(4, 0.02)
        ref = B.sample_glms_hmc(popn, x, 6, n_warmup=0, n_leapfrog=3, step_sz=step, seed=11)
        step[2] = 1e3
        out = B.sample_glms_hmc(popn, x, 6, n_warmup=0, n_leapfrog=3, step_sz=step, seed=11)
        print(out['accept_rate'], ref['accept_rate'])
        assert out['accept_rate'][2] == 0.0 and out['step_sz'][2] == 1e3
        assert np.all(out['samples'][:, 2] == X0[2])
        others = [0, 1, 3]
        assert np.array_equal(out['samples'][:, others], ref['samples'][:, others])
        assert np.array_equal(out['accept_rate'][others], ref['accept_rate'][others])
        assert np.all(ref['accept_rate'] > 0.0)
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_unsupported_inputs_raise():
    from theano_pyglm_amd.inference import batched_hmc as B
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):     # an 'st' stimulus / Dirichlet impulses
        p2 = Population(make_model(name, N=2, dt=0.001))
        assert not B.supported(p2)
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            B.sample_glms_hmc(p2, p2.sample(np.random.RandomState(1)), 2)
    popn = _population(N=2, T=2.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                B.sample_glms_hmc(popn, x, 2)
        finally:
            popn.set_time_shard(None)
        with pytest.raises(ValueError, match="empty"):
            B.sample_glms_hmc(popn, x, 2, n_lo=1, n_hi=1)
    finally:
        popn.release_data()
