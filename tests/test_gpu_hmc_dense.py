"""GPU tests of the lock-step HMC chain with a dense mass matrix (pgl_tri_matvec_dev, pgl_hmc_dense_* and the 'laplace_dense'
/ (M, P, P) forms of inference/batched_hmc.py: mass): the batched triangular products against numpy, the device chain
through the C ABI against the host mirror of the same state machine (tests/hmc_dense_mirror.py: csrc/pglm_hmc_dense.h built
by gcc) fed by the oracle's ll and gradient, the dense chain with a diagonal factor against the diagonal device chain, and
the driver's contract.

As in tests/test_gpu_hmc.py the cases are seeded so that in the mirror every decision keeps |log u - (H0 - H1)| > 1e-4
(asserted) and both outcomes occur.  The device always gets its factors with NaN above the diagonal: a finite chain has
never read them."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import hmc_mirror as HM
from tests import hmc_dense_mirror as HD
from tests.test_gpu_hmc import MARGIN, _population, _prior, _problem, device_chain

TILE = 64                                                     # PGL_TRI_TILE: outputs per workgroup of k_tri_matvec


def _factor(M, P, seed):
    """Random well-conditioned lower-triangular factors: diagonal in [0.7, 1.3], off-diagonal entries N(0, 0.3^2 / P)."""
    rng = np.random.default_rng(seed)
    W = np.tril(rng.standard_normal((M, P, P)), -1) * (0.3 / np.sqrt(P))
    W[:, np.arange(P), np.arange(P)] = 0.7 + 0.6 * rng.random((M, P))
    return W


def _nan_above(W):
    Wn = np.array(W, dtype=float)
    iu = np.triu_indices(Wn.shape[-1], 1)
    Wn[..., iu[0], iu[1]] = np.nan
    return Wn


# ---- the products ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)
    yield h
    h.close()


def _device_product(h, W, x, trans):
    import torch
    dev = torch.device('cuda', 0)
    M, P = x.shape
    Wd = torch.tensor(W, dtype=torch.float64, device=dev)
    xd = torch.tensor(x, dtype=torch.float64, device=dev)
    yd = torch.full((M, P), np.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h.tri_matvec_dev(Wd.data_ptr(), M, P, trans, xd.data_ptr(), yd.data_ptr())
    h.sync()
    return yd.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 255, 256, 257, 281, 641])
def test_tri_matvec_against_numpy(handle, P):
    """y = W x and W^T x for M = 1 and 3 with NaN above the diagonal: within 1e-13 sum|w||x| of an extended-precision
    numpy product per output, the same bits twice, the rows of the M = 3 call equal to the M = 1 calls bit for bit, and
    the same bits from the row grid (development option 90: one workgroup per matrix walks all its tiles)."""
    assert TILE == 64                                          # (else P = TILE - 1, TILE, TILE + 1 belong to the list)
    rng = np.random.default_rng(100 + P)
    W = rng.standard_normal((3, P, P))
    x = rng.standard_normal((3, P))
    Wn = _nan_above(W)
    L = np.tril(W).astype(np.longdouble)
    xl = x.astype(np.longdouble)
    for trans in (0, 1):
        A = np.swapaxes(L, 1, 2) if trans else L
        ref = np.einsum('mij,mj->mi', A, xl)
        mag = np.einsum('mij,mj->mi', np.abs(A), np.abs(xl)).astype(float)
        y3 = _device_product(handle, Wn, x, trans)
        assert np.all(np.isfinite(y3))
        err = np.max(np.abs((y3 - ref).astype(float)) / mag)
        print("P = %d trans = %d: largest error / sum|w||x| = %.3e" % (P, trans, err))
        assert err <= 1e-13
        assert np.array_equal(y3, _device_product(handle, Wn, x, trans))
        handle.set_option(90, 1)
        try:
            assert np.array_equal(y3, _device_product(handle, Wn, x, trans))
        finally:
            handle.set_option(90, 0)
        for m in range(3):
            y1 = _device_product(handle, Wn[m:m + 1], x[m:m + 1], trans)
            assert np.array_equal(y1[0], y3[m])


# ---- the chain through the C ABI -----------------------------------------------------------------------------------
def _oracle_target(probs, n_lo, n_hi):
    def target(X):
        ll, g = 0.0, 0.0
        for p in probs:
            p.theta = p.theta.copy()
            p.theta[n_lo:n_hi] = X
            a, b = p.oracle_ll_grad(n_lo, n_hi)
            ll, g = ll + a, g + b
        return ll, g
    return target


def mirror_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, W, n_warmup=0):
    """The dense host mirror on the oracle.  -> (samples, accepted, margins, final scalar state)."""
    p0 = probs[0]
    mir = HD.DenseMirror(_oracle_target(probs, n_lo, n_hi), X0, W, n_lo=n_lo, prior=(prm[0], p0.N, p0.B, p0.Dstim, prm[1:]),
                         step0=step, seed=seed)
    s, a, m = mir.run(n_trans, L, n_warmup)
    return s, a, m, mir.sc.copy()


def dense_device_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, W, n_warmup=0, epi_f64=False):
    """The same chain through pgl_hmc_dense_*; the scalar state is read after every transition (a test's privilege).
    epi_f64: evaluate with the all-f64 rate epilogue (PGL_OPT_EPI_F64)."""
    import torch
    from theano_pyglm_amd import _lib
    p0 = probs[0]
    M, P = X0.shape
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    hs = [p.device(0) for p in probs]
    stream = torch.cuda.Stream(dev)
    try:
        for h in hs:
            h.set_stream(stream.cuda_stream)
            if epi_f64:
                h.set_option(_lib.OPT_EPI_F64, 1)
        with torch.cuda.stream(stream):
            h0 = hs[0]
            st = torch.zeros(h0.hmc_state_doubles(M, P), dtype=f64, device=dev)
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            sc = st[4 * M * P:].view(10, M)
            Weff = torch.tensor(p0.Weff, dtype=f64, device=dev)
            Wd = torch.tensor(_nan_above(W), dtype=f64, device=dev)
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
                h0.hmc_dense_begin_dev(st.data_ptr(), M, P, Wd.data_ptr(), Xt.data_ptr())
                for i in range(L):
                    ll, g = evaluate(Xt)
                    h0.hmc_dense_leap_dev(st.data_ptr(), M, P, Wd.data_ptr(), ll.data_ptr(), g.data_ptr(), prm, i == L - 1, n_warmup, Xt.data_ptr(), samples[t].data_ptr() if i == L - 1 else 0)
                stream.synchronize()
                acc.append(sc[HM.SC['acc']].cpu().numpy() != 0.0)
            stream.synchronize()
            return samples.cpu().numpy(), np.array(acc), sc.cpu().numpy()
    finally:
        for h in hs:
            h.close()


def compare(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, W, n_warmup=0, label=""):
    sm, am, mm, scm = mirror_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, W, n_warmup)
    print("%s mirror: accepted %d of %d, smallest margin %.3e" % (label, am.sum(), am.size, mm.min()))
    assert mm.min() > MARGIN                                    # the condition the case was seeded for
    assert am.any() and not am.all()                            # both outcomes of the decision
    sd, ad, scd = dense_device_chain(probs, X0, n_lo, n_hi, prm, n_trans, L, step, seed, W, n_warmup)
    assert np.array_equal(ad, am)
    err = np.max(np.abs(sd - sm) / np.max(np.abs(sm), axis=2, keepdims=True))
    print("%s device against mirror: largest error relative to the row's largest entry %.3e" % (label, err))
    assert err <= 1e-9
    assert np.array_equal(scd[HM.SC['t']], scm[HM.SC['t']]) and np.array_equal(scd[HM.SC['n_accept']], scm[HM.SC['n_accept']])
    assert np.allclose(scd[HM.SC['step']], scm[HM.SC['step']], rtol=1e-15, atol=0.0)
    return sm, am, sd, ad


CASES = {  # (nlin, prior) -> (step, seed): seeded on the CPU for a mix of decisions with margins > 1e-4
    ('explinear', 'gauss'): (1.0, 1),                           # mirror: 33 of 40 accepted, smallest margin 1.4e-1
    ('explinear', 'lasso'): (1.0, 1),                           # 29 of 40, 3.5e-2
    ('exp', 'gauss'): (0.2, 1),                                 # 23 of 40, 6.0e-2
    ('exp', 'lasso'): (0.2, 1),                                 # 18 of 40, 6.4e-2
}
WIDE = (1.0, 1)                                                 # N = 70: 68 of 140, 2.1e-2
TWO_SEQ = (1.0, 1)                                              # 16 of 20, 1.8e-1


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
@pytest.mark.parametrize('prior', ['gauss', 'lasso'])
def test_device_chain_equals_host_mirror(kind, prior):
    """N = 5, nT = 2 000, n_leapfrog = 3, 8 transitions, 2 of them warm-up."""
    p = _problem(5, 2000, kind, 31)
    step, seed = CASES[(kind, prior)]
    compare([p], p.theta.copy(), 0, 5, _prior(kind, prior), 8, 3, step, seed, _factor(5, p.P, 7), n_warmup=2,
            label="%s/%s" % (kind, prior))


@pytest.mark.gpu
def test_wide_rows():
    """P = 281: more than one tile of the products and more than the 256 threads of a row kernel.  N = 70, B = 4, nT = 512,
    2 transitions."""
    p = _problem(70, 512, 'explinear', 37, ibasis=H.std_ibasis()[:, :4])
    assert p.P == 281
    step, seed = WIDE
    compare([p], p.theta.copy(), 0, 70, _prior('explinear', 'lasso'), 2, 3, step, seed, _factor(70, 281, 9), label="N=70")


@pytest.mark.gpu
def test_diagonal_factor_equals_the_diagonal_device_chain():
    """W = diag(sqrt(minv)): the dense device chain against pgl_hmc_* with minv -- the same decisions, samples to 1e-9."""
    p = _problem(5, 2000, 'explinear', 31)
    prm = _prior('explinear', 'gauss')
    minv = 0.25 + 1.5 * np.random.default_rng(43).random((5, p.P))
    W = np.zeros((5, p.P, p.P))
    W[:, np.arange(p.P), np.arange(p.P)] = np.sqrt(minv)
    sg, ag, scg = device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, 0.7, 1, minv=minv, n_warmup=2)
    sd, ad, scd = dense_device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, 0.7, 1, W, n_warmup=2)
    assert ag.any()
    assert np.array_equal(ad, ag)
    err = np.max(np.abs(sd - sg) / np.max(np.abs(sg), axis=2, keepdims=True))
    print("dense against diagonal: largest error relative to the row's largest entry %.3e" % err)
    assert err <= 1e-9
    assert np.array_equal(scd[HM.SC['n_accept']], scg[HM.SC['n_accept']])
    assert np.allclose(scd[HM.SC['step']], scg[HM.SC['step']], rtol=1e-15, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,epi_f64', [('exp', False), ('explinear', True)])
def test_subset_equals_batch_and_runs_repeat(kind, epi_f64):
    """Neurons 1..3 against rows 1..3 of the chain over 0..4, and the chain twice, warm-up included: the same bits.
    The softplus nonlinearity runs with the all-f64 rate epilogue: by default the ll+grad kernels take exp(-x) from the
    single-precision hardware exp in waves whose currents are all > 12 (PGL_OPT_EPI_F64 in include/pyglm_hip.h, within 5e-13),
    and which neurons share a wave depends on the range of the call -- there an evaluation over a subset equals the batch
    to 5e-13, not bit for bit, whatever the sampler around it (measured here: 3.6e-15 on the samples; 0 with this option)."""
    p = _problem(5, 2000, kind, 31)
    prm = _prior(kind, 'gauss')
    step, seed = CASES[(kind, 'gauss')]
    W = _factor(5, p.P, 7)
    full, accf, _ = dense_device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, step, seed, W, n_warmup=3, epi_f64=epi_f64)
    again, acca, _ = dense_device_chain([p], p.theta.copy(), 0, 5, prm, 6, 3, step, seed, W, n_warmup=3, epi_f64=epi_f64)
    assert np.array_equal(full, again) and np.array_equal(accf, acca)
    sub, accs, _ = dense_device_chain([p], p.theta[1:4].copy(), 1, 4, prm, 6, 3, step, seed, W[1:4], n_warmup=3,
                                      epi_f64=epi_f64)
    assert np.array_equal(sub, full[:, 1:4]) and np.array_equal(accs, accf[:, 1:4])
    assert accf.any() and np.any(full[-1] != p.theta)


@pytest.mark.gpu
def test_two_data_sequences_sum():
    """Two recordings of the same population: their [ll | grad] blocks are summed before the row kernels see them."""
    p1 = _problem(5, 2000, 'explinear', 31)
    p2 = _problem(5, 1008, 'explinear', 41)
    p2.theta, p2.Weff = p1.theta, p1.Weff
    step, seed = TWO_SEQ
    compare([p1, p2], p1.theta.copy(), 0, 5, _prior('explinear', 'gauss'), 4, 3, step, seed, _factor(5, p1.P, 7),
            label="two sequences")


# ---- the driver --------------------------------------------------------------------------------------------------
def _theta_cov(popn, x, lap):
    """laplace_glms' covariances in the theta layout."""
    from theano_pyglm_amd.inference import batched_hmc as B
    pi = B._theta_positions(popn, x, 0, popn.glm.P)
    return np.array([r['cov'][np.ix_(pi, pi)] for r in lap])


@pytest.mark.gpu
def test_driver_laplace_dense():
    from theano_pyglm_amd.inference import batched_hmc as B
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        x0 = copy.deepcopy(x)
        L, n_warm, n_s, thin = 4, 6, 5, 2
        out = B.sample_glms_hmc(popn, x, n_s, n_warmup=n_warm, n_leapfrog=L, step_sz=0.05, thin=thin, mass='laplace_dense',
                                seed=5)
        st = popn.last_fit_stats
        print(st, out['accept_rate'], out['step_sz'], out['dense_rows'])
        P = popn.glm.P
        assert out['samples'].shape == (n_s, 4, P) and np.all(np.isfinite(out['samples']))
        assert np.all(out['accept_rate'] > 0.0) and np.all(out['accept_rate'] <= 1.0)
        assert np.all(out['step_sz'] >= 1e-3) and np.all(out['step_sz'] <= 1.0)
        lap = laplace_glms(popn, x)
        assert out['dense_rows'].shape == (4,) and out['dense_rows'].dtype == bool
        assert np.array_equal(out['dense_rows'], np.array([r['pd'] for r in lap]))
        n_total = n_warm + n_s * thin
        assert st['transitions'] == n_total and st['mass'] == 'dense' and st['mass_setup_s'] > 0.0
        assert st['evaluations_per_transition'] == L and st['row_launches_per_transition'] == L + 1
        assert out['n_evals'] == 1 + n_total * L == st['ll_grad_launches']
        assert st['host_syncs_in_chain'] == 0
        assert np.array_equal(popn.theta_matrix(x), popn.theta_matrix(x0))
        # the other forms of mass keep their record
        B.sample_glms_hmc(popn, x, 2, n_warmup=1, n_leapfrog=2, step_sz=0.05, mass='laplace', seed=5)
        assert popn.last_fit_stats['mass'] == 'diagonal'
        B.sample_glms_hmc(popn, x, 2, n_warmup=1, n_leapfrog=2, step_sz=0.05, seed=5)
        assert popn.last_fit_stats['mass'] == 'identity'
        assert out['dense_rows'].all()                             # (an exp nonlinearity under Gaussian priors: concave everywhere)
        # the explicit form: the Laplace covariances themselves give the same samples
        Sig = _theta_cov(popn, x, lap)
        ex = B.sample_glms_hmc(popn, x, n_s, n_warmup=n_warm, n_leapfrog=L, step_sz=0.05, thin=thin, mass=Sig, seed=5)
        assert 'dense_rows' not in ex and popn.last_fit_stats['mass'] == 'dense'
        assert np.array_equal(ex['samples'], out['samples']) and np.array_equal(ex['step_sz'], out['step_sz'])
        # a sub-range with the matching slices of Sigma: the matching rows
        sub = B.sample_glms_hmc(popn, x, n_s, n_warmup=n_warm, n_leapfrog=L, step_sz=0.05, thin=thin, mass=Sig[1:3], seed=5,
                                n_lo=1, n_hi=3)
        assert np.array_equal(sub['samples'], out['samples'][:, 1:3])
        assert np.array_equal(sub['step_sz'], out['step_sz'][1:3])
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_driver_fallback_row(monkeypatch):
    """A neuron whose Laplace result is not positive definite runs on the diagonal 'laplace' rule: its samples are those
    of the mass='laplace' chain to rounding (the dense kernels with a diagonal factor), the other rows are untouched."""
    from theano_pyglm_amd.inference import batched_hmc as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        kw = dict(n_warmup=3, n_leapfrog=3, step_sz=0.05, seed=5)
        ref = B.sample_glms_hmc(popn, x, 4, mass='laplace_dense', **kw)
        diag = B.sample_glms_hmc(popn, x, 4, mass='laplace', **kw)
        rows = B._laplace_rows

        def not_pd(population, xx, n_lo, n_hi):
            Hm, out = rows(population, xx, n_lo, n_hi)
            P = Hm.shape[1]
            return Hm, [(False, np.full((P, P), np.nan)) if n_lo + i == 2 else r for i, r in enumerate(out)]
        monkeypatch.setattr(B, '_laplace_rows', not_pd)
        out = B.sample_glms_hmc(popn, x, 4, mass='laplace_dense', **kw)
        assert np.array_equal(out['dense_rows'], [True, True, False, True])
        others = [0, 1, 3]
        assert np.array_equal(out['samples'][:, others], ref['samples'][:, others])
        assert np.all(np.isfinite(out['samples'][:, 2]))
        err = np.max(np.abs(out['samples'][:, 2] - diag['samples'][:, 2])) / np.max(np.abs(diag['samples'][:, 2]))
        print("fallback row against the diagonal chain: %.3e" % err)
        assert err <= 1e-9
        assert out['accept_rate'][2] == diag['accept_rate'][2]
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_driver_bad_masses_raise_and_rejection_is_local():
    from theano_pyglm_amd.inference import batched_hmc as B
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        X0 = popn.theta_matrix(x)
        P = popn.glm.P
        Sig = _theta_cov(popn, x, laplace_glms(popn, x))
        not_pd = Sig.copy()
        not_pd[1] = -not_pd[1]
        asym = Sig.copy()
        asym[0, 0, 1] += 1.0
        for bad in (Sig[:3], Sig[:, :P - 1, :P - 1], np.ones((4, P, P + 1)), not_pd, asym):
            with pytest.raises(ValueError):
                B.sample_glms_hmc(popn, x, 2, mass=bad)
        with pytest.raises(ValueError):
            B.sample_glms_hmc(popn, x, 2, mass='dense')
        step = np.full(4, 0.3)
        ref = B.sample_glms_hmc(popn, x, 6, n_warmup=0, n_leapfrog=3, step_sz=step, mass=Sig, seed=11)
        step[2] = 1e3
        out = B.sample_glms_hmc(popn, x, 6, n_warmup=0, n_leapfrog=3, step_sz=step, mass=Sig, seed=11)
        print(out['accept_rate'], ref['accept_rate'])
        assert out['accept_rate'][2] == 0.0 and out['step_sz'][2] == 1e3
        assert np.all(out['samples'][:, 2] == X0[2])
        others = [0, 1, 3]
        assert np.array_equal(out['samples'][:, others], ref['samples'][:, others])
        assert np.array_equal(out['accept_rate'][others], ref['accept_rate'][others])
        assert np.all(ref['accept_rate'] > 0.0)
    finally:
        popn.release_data()
