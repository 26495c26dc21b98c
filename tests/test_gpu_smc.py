"""GPU tests of adaptive sequential Monte Carlo (pgl_smc_* kernels, inference/batched_smc.py): a stage call launch by
launch against the host mirror of the same rules (tests/smc_mirror.py: csrc/pglm_smc.h built by gcc) on the same input, the
guarded moves against the pgl_ais_* kernels on the same state, and the driver's contract.

The resampling decision and the ancestors are discontinuities: the inputs are seeded on the CPU so that in the mirror no
cumulative weight lies within 1e-9 of a sampling position and no ESS within 1e-9 K of the threshold (asserted)."""
import re

import numpy as np
import pytest

from tests import smc_mirror as SM
from tests.ais_mirror import SC
from tests.test_gpu_ais import _population, _prior, _problem

NS, REC = SM.NS, SM.REC
S = 8


def _blocks(p, K, M, seed, spread, dead=None, all_dead=None, done=None, ess_min=0.5):
    """A mirror of K x M rows of problem p whose kept parts are random: q near the prior mean, gll, ll0 = -spread * U(0, 1),
    lp0, logw = normalised random weights."""
    prm = _prior('explinear')
    rng = np.random.default_rng(seed)
    mir = SM.Mirror(lambda X: (np.zeros(M), np.zeros((M, p.P))), K, M, (p.N, p.B, p.Dstim, prm[1:]), seed=seed, step0=0.2, S=S,
                    ess_min=ess_min)
    R = K * M
    mir.gll[:] = rng.standard_normal((R, p.P))
    mir.sc[SC['ll0']] = -spread * rng.random(R)
    lw = 0.3 * rng.standard_normal((K, M))
    mir.sc[SC['logw']] = (lw - np.log(np.sum(np.exp(lw), axis=0))).reshape(-1)
    mir.sc[SC['lp0']] = rng.standard_normal(R)
    mir.acc[:] = rng.integers(0, 2, R).astype(float)
    mir.ns[NS['stage']] = 1.0
    if dead is not None:
        mir.sc[SC['ll0']][dead] = np.nan
    if all_dead is not None:
        mir.sc[SC['logw']][np.arange(K) * M + all_dead] = -np.inf
    if done is not None:
        mir.ns[NS['done'], done] = 1.0
        mir.ns[NS['beta'], done] = 1.0
    return mir, prm


def _device_stage(p, mir, prm):
    import torch
    dev = torch.device('cuda', 0)
    h = p.device(0)
    try:
        st = torch.tensor(mir.st, dtype=torch.float64, device=dev)
        smc = torch.tensor(mir.smc, dtype=torch.float64, device=dev)
        h.smc_stage_dev(st.data_ptr(), smc.data_ptr(), mir.K, mir.M, mir.P, mir.S, prm, mir.n_steps, mir.rho, mir.ess_min,
                        mir.delta_min, mir.seed)
        torch.cuda.synchronize()
        out = SM.Blocks(mir.K, mir.M, mir.P, mir.S)
        out.set(st.cpu().numpy(), smc.cpu().numpy())
        return out
    finally:
        h.close()


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(same, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    return float(np.max(e)) if e.size else 0.0


def _compare_stage(p, mir, prm, label):
    before = SM.Blocks(mir.K, mir.M, mir.P, mir.S)
    before.set(mir.st, mir.smc)
    d = _device_stage(p, mir, prm)
    margins = mir.stage()
    K, M = mir.K, mir.M
    print(label, "rs", mir.ns[NS['rs']], "beta", mir.ns[NS['beta']], "ess", mir.ns[NS['ess']], "margins", margins)
    assert np.all(margins[0] > 1e-9) and np.all(margins[1] > 1e-9 * K)      # the condition the inputs were seeded for
    assert np.array_equal(d.anc, mir.anc)
    for f in ('stage', 'done', 'n_resampled', 'live', 'rs', 'acc'):
        assert np.array_equal(d.ns[NS[f]], mir.ns[NS[f]]), f
    for f in ('beta', 'log_Z', 'step', 'ess'):
        assert _rel(d.ns[NS[f]], mir.ns[NS[f]]) <= 1e-12, (f, d.ns[NS[f]], mir.ns[NS[f]])
    assert _rel(d.rec, mir.rec) <= 1e-12 and _rel(d.w, mir.w) <= 1e-12
    lw_d, lw_m = d.sc[SC['logw']], mir.sc[SC['logw']]
    assert np.array_equal(np.isneginf(lw_d), np.isneginf(lw_m))
    fin = np.isfinite(lw_m)
    assert np.max(np.abs(lw_d[fin] - lw_m[fin]) / np.maximum(1.0, np.abs(lw_m[fin])), initial=0.0) <= 1e-12
    assert d.nact[0] == mir.nact[0] and np.array_equal(d.acc, mir.acc)   # (cleared, but for a neuron done before)
    # the copied fields exactly, the new target to rounding
    assert np.array_equal(d.q, mir.q) and np.array_equal(d.gll, mir.gll)
    for f in ('ll0', 'lp0', 'seed_lo', 'seed_hi', 'particle', 't', 'neuron'):
        assert np.array_equal(d.sc[SC[f]], mir.sc[SC[f]], equal_nan=True), f
    assert _rel(d.sc[SC['step']], mir.sc[SC['step']]) <= 1e-12 and _rel(d.sc[SC['beta']], mir.sc[SC['beta']]) <= 1e-12
    gscale = np.max(np.abs(mir.g), axis=1, keepdims=True)
    assert np.max(np.abs(d.g - mir.g) / np.maximum(gscale, 1e-300)) <= 1e-13
    # U0 = -(beta ll0 + lp0) of the retemper launch, at the beta ITS input holds (the stage launch's, which agrees with the
    # mirror's to 1e-12 only), to 1e-13 of the terms' size: the sum cancels, |U0| is no scale for its rounding
    u0 = np.isfinite(mir.sc[SC['U0']])
    assert np.array_equal(np.isfinite(d.sc[SC['U0']]), u0)
    u0 = u0 & (np.tile(mir.ns[NS['live']], K) == 1.0)            # (rows the stage retempered)
    bl, lp = d.sc[SC['beta']][u0] * d.sc[SC['ll0']][u0], d.sc[SC['lp0']][u0]
    assert np.max(np.abs(d.sc[SC['U0']][u0] + (bl + lp)) / (np.abs(bl) + np.abs(lp)), initial=0.0) <= 1e-13
    # a neuron the stage did not touch keeps its bits
    for i in np.where(mir.ns[NS['live']] == 0.0)[0]:
        rows = np.arange(K) * M + i
        assert np.array_equal(d.q[rows], before.q[rows]) and np.array_equal(d.g[rows], before.g[rows])
        keep = [k for k in range(len(SC)) if k != SC['logw']]
        assert np.array_equal(d.sc[keep][:, rows], before.sc[keep][:, rows], equal_nan=True)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize('K,M', [(1, 1), (5, 3), (64, 3), (300, 1), (300, 3)])
def test_stage_launch_against_the_mirror(K, M):
    """One pgl_smc_stage_dev call (stage, gather, retemper) on a state made on the CPU: K in {1, 5, 64, 300} (300 > the 256
    threads of the workgroup), M in {1, 3}; with M = 3 neuron 0 spreads its ll0 wide (it resamples), neuron 1 narrowly (it
    does not) and neuron 2 is, in turn, all dead / done; one particle of neuron 0 is dead."""
    p = _problem(3, 600, 'explinear', 31)
    for variant in range(2 if M == 3 else 1):
        mir, prm = _blocks(p, K, M, 100 + K + variant, 1.0, dead=(M if K > 1 else None),
                           all_dead=(2 if M == 3 and variant == 0 else None), done=(2 if M == 3 and variant == 1 else None))
        R = K * M
        if K > 1:
            mir.sc[SC['ll0']][np.arange(K) * M] *= 60.0          # neuron 0: the conditional ESS bites, the ESS falls
            mir.sc[SC['logw']][np.arange(0, K, 2) * M] -= 3.0
            if M == 3:
                # neuron 1: ll0 = -5 - 1e-3 U.  (Not -1e-3 U alone: log_Z would be log of a sum within 5e-4 of 1, whose
                # rounding, K 2^-53 absolute whatever the order of the sum, is 1e-12 of such a log_Z -- a relative bound
                # says nothing there.)
                mir.sc[SC['ll0']][np.arange(K) * M + 1] = -5.0 + 1e-3 * mir.sc[SC['ll0']][np.arange(K) * M + 1]
        d = _compare_stage(p, mir, prm, "K=%d M=%d v=%d" % (K, M, variant))
        if K > 1:
            assert d.ns[NS['rs'], 0] == 1.0 and 0.0 < d.ns[NS['beta'], 0] < 1.0
            if M == 3:
                assert d.ns[NS['rs'], 1] == 0.0 and d.ns[NS['beta'], 1] == 1.0 and d.ns[NS['done'], 1] == 1.0
                assert (d.ns[NS['log_Z'], 2] == -np.inf) if variant == 0 else (d.ns[NS['live'], 2] == 0.0)
        else:
            assert d.ns[NS['beta'], 0] == 1.0 and d.ns[NS['log_Z'], 0] == mir.sc[SC['ll0']][0]


@pytest.mark.gpu
@pytest.mark.parametrize('N,nb,P', [(5, 1, 6), (70, 4, 281)])
def test_gather_and_retemper(N, nb, P):
    """The gather at P = 6 and at P = 281 > 256 (N = 70, 4 basis columns, nT = 600), K = 6, M = 2.  Through the stage call:
    the identity (no resampling), a full collapse onto one slot (one particle holds all the weight) and a generic
    resampling.  Through pgl_smc_gather_dev on prescribed ancestors: a cyclic shift, anc[k] = (k + 1 + i) mod K, in which
    every slot is read by another while it is overwritten itself, for neuron 0 alone resampled (rs = 1, 0), with new betas
    and steps per neuron."""
    import torch
    from tests import helpers as H
    p = _problem(N, 600, 'explinear', 37, ibasis=H.std_ibasis()[:, :nb])
    assert p.P == P
    K, M = 6, 2
    for name in ('identity', 'collapse', 'generic'):
        mir, prm = _blocks(p, K, M, 7, 2.0, ess_min=0.0 if name == 'identity' else 1.0)
        if name == 'collapse':
            mir.sc[SC['logw']] = -800.0
            mir.sc[SC['logw']][[3 * M, 4 * M + 1]] = 0.0
        if name == 'generic':
            mir.sc[SC['ll0']] *= 4.0
        d = _compare_stage(p, mir, prm, name)
        anc = d.anc.reshape(K, M).astype(int)
        if name == 'identity':
            assert np.array_equal(anc, np.tile(np.arange(K)[:, None], (1, M)))
        elif name == 'collapse':
            assert np.all(anc[:, 0] == 3) and np.all(anc[:, 1] == 4)
        else:
            assert any(len(set(anc[:, i])) > 1 and np.any(anc[:, i] != np.arange(K)) for i in range(M))
    for rs in ([1.0, 1.0], [1.0, 0.0]):
        mir, prm = _blocks(p, K, M, 9, 2.0)
        anc = (np.arange(K)[:, None] + 1 + np.arange(M)[None, :]) % K
        mir.anc[:] = anc.reshape(-1)
        mir.ns[NS['live']] = 1.0
        mir.ns[NS['rs']] = rs
        mir.ns[NS['beta']] = [0.3, 0.7]
        mir.ns[NS['step']] = [0.11, 0.07]
        before = SM.Blocks(K, M, P, S)
        before.set(mir.st, mir.smc)
        h = p.device(0)
        try:
            dev = torch.device('cuda', 0)
            st = torch.tensor(mir.st, dtype=torch.float64, device=dev)
            smc = torch.tensor(mir.smc, dtype=torch.float64, device=dev)
            h.smc_gather_dev(st.data_ptr(), smc.data_ptr(), K, M, P, S, prm)
            torch.cuda.synchronize()
            d = SM.Blocks(K, M, P, S)
            d.set(st.cpu().numpy(), smc.cpu().numpy())
        finally:
            h.close()
        mir.gather_retemper()
        for i in range(M):
            rows = np.arange(K) * M + i
            src = (anc[:, i] if rs[i] else np.arange(K)) * M + i
            assert np.array_equal(d.q[rows], before.q[src]) and np.array_equal(d.gll[rows], before.gll[src])
            assert np.array_equal(d.sc[SC['ll0']][rows], before.sc[SC['ll0']][src])
            assert np.array_equal(d.sc[SC['lp0']][rows], before.sc[SC['lp0']][src])
            assert np.all(d.sc[SC['step']][rows] == mir.ns[NS['step'], i]) and np.all(d.sc[SC['beta']][rows] == mir.ns[NS['beta'], i])
        assert np.array_equal(d.q, mir.q) and np.array_equal(d.gll, mir.gll)
        for f in ('ll0', 'lp0', 'seed_lo', 'seed_hi', 'particle', 't', 'neuron', 'logw', 'step', 'beta'):
            assert np.array_equal(d.sc[SC[f]], mir.sc[SC[f]]), f
            if f in ('seed_lo', 'seed_hi', 'particle', 't', 'neuron', 'logw'):
                assert np.array_equal(d.sc[SC[f]], before.sc[SC[f]]), f
        gscale = np.max(np.abs(mir.g), axis=1, keepdims=True)
        assert np.max(np.abs(d.g - mir.g) / gscale) <= 1e-13
        bl, lp = d.sc[SC['beta']] * d.sc[SC['ll0']], d.sc[SC['lp0']]
        assert np.max(np.abs(d.sc[SC['U0']] + (bl + lp)) / (np.abs(bl) + np.abs(lp))) <= 1e-13
        assert np.max(np.abs(d.sc[SC['U0']] - mir.sc[SC['U0']]) / (np.abs(bl) + np.abs(lp))) <= 1e-13
        assert d.nact[0] == M == mir.nact[0]


def _moves(p, mir, prm, dense, guarded, W=None, minv=None):
    """begin + two leaps (the second the last) on the mirror's state through pgl_smc_* (guarded) or pgl_ais_* -> Blocks, Xt."""
    import torch
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    h = p.device(0)
    try:
        K, M, P, R = mir.K, mir.M, mir.P, mir.R
        st = torch.tensor(mir.st, dtype=f64, device=dev)
        smc = torch.tensor(mir.smc, dtype=f64, device=dev)
        Xt = torch.full((R, P), -7.0, dtype=f64, device=dev)
        Weff = torch.tensor(p.Weff, dtype=f64, device=dev)
        buf = torch.empty(R * (1 + P), dtype=f64, device=dev)
        acc = torch.zeros(R, dtype=f64, device=dev)
        Wd = torch.tensor(W, dtype=f64, device=dev) if dense else None
        md = torch.tensor(minv, dtype=f64, device=dev)
        sp, mp = st.data_ptr(), smc.data_ptr()
        if guarded:
            (h.smc_dense_begin_dev(sp, mp, K, M, P, S, Wd.data_ptr(), Xt.data_ptr()) if dense else
             h.smc_begin_dev(sp, mp, K, M, P, S, md.data_ptr(), Xt.data_ptr()))
        else:
            (h.ais_dense_begin_dev(sp, K, M, P, Wd.data_ptr(), Xt.data_ptr()) if dense else
             h.ais_begin_dev(sp, K, M, P, md.data_ptr(), Xt.data_ptr()))
        torch.cuda.synchronize()                                # (the handle launches on a stream of its own)
        xts = [Xt.cpu().numpy()]
        for last in (False, True):
            for k in range(K):
                h.ll_grad_dev(Xt[k * M].data_ptr(), Weff.data_ptr(), buf[k * M:].data_ptr(), buf[R + k * M * P:].data_ptr(), 0, M)
            ll, g = buf.data_ptr(), buf[R:].data_ptr()
            if guarded and dense:
                h.smc_dense_leap_dev(sp, mp, K, M, P, S, Wd.data_ptr(), ll, g, prm, last, Xt.data_ptr())
            elif guarded:
                h.smc_leap_dev(sp, mp, K, M, P, S, md.data_ptr(), ll, g, prm, last, Xt.data_ptr())
            elif dense:
                h.ais_dense_leap_dev(sp, K, M, P, Wd.data_ptr(), ll, g, prm, last, False, Xt.data_ptr(), acc.data_ptr(), 0)
            else:
                h.ais_leap_dev(sp, K, M, P, md.data_ptr(), ll, g, prm, last, False, Xt.data_ptr(), acc.data_ptr(), 0)
            torch.cuda.synchronize()
            xts.append(Xt.cpu().numpy())
        out = SM.Blocks(K, M, P, S)
        out.set(st.cpu().numpy(), smc.cpu().numpy())
        return out, xts, acc.cpu().numpy()
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [False, True])
def test_guarded_moves(dense):
    """N = 3, nT = 600, K = 9 (two passes of 8 particles in the shared product), neuron 1 done: its rows are bitwise unchanged
    after begin and two leaps and its q is what Xt holds; the rows of neurons 0 and 2 have the bits of pgl_ais_* on the same
    state, and their decisions are counted in the block's acc."""
    p = _problem(3, 600, 'explinear', 31)
    K, M = 9, 3
    rng = np.random.default_rng(5)
    mir, prm = _blocks(p, K, M, 11, 1.0)
    mir.sc[SC['ll0']] = 0.0
    mir.gll[:] = 0.0
    mir.stage()                                                 # a consistent target (U0, g, step) for every row
    mir.acc[:] = 0.0
    mir.ns[NS['done']] = [0.0, 1.0, 0.0]
    mir.sc[SC['step']] = 0.01
    mir.sc[SC['beta']] = 1e-4                                   # (U0 and g hold for any beta: ll0 = 0, gll = 0)
    minv = 0.5 + rng.random((M, p.P))
    W = np.tril(0.05 * rng.standard_normal((M, p.P, p.P))) + np.eye(p.P)[None] * np.sqrt(minv)[:, :, None]
    g, xg, _ = _moves(p, mir, prm, dense, True, W, minv)
    a, xa, acc = _moves(p, mir, prm, dense, False, W, minv)
    done = np.arange(K) * M + 1
    act = np.array([r for r in range(K * M) if r % M != 1])
    assert np.array_equal(g.st.reshape(-1)[:SM.NVEC * mir.R * mir.P].reshape(SM.NVEC, mir.R, mir.P)[:, done],
                          mir.st[:SM.NVEC * mir.R * mir.P].reshape(SM.NVEC, mir.R, mir.P)[:, done])
    assert np.array_equal(g.sc[:, done], mir.sc[:, done], equal_nan=True)
    assert np.all(g.acc[done] == 0.0)
    for x in xg[:2]:
        assert np.array_equal(x[done], mir.q[done])
    vg = g.st[:SM.NVEC * mir.R * mir.P].reshape(SM.NVEC, mir.R, mir.P)
    va = a.st[:SM.NVEC * mir.R * mir.P].reshape(SM.NVEC, mir.R, mir.P)
    assert np.array_equal(vg[:, act], va[:, act]) and np.array_equal(g.sc[:, act], a.sc[:, act], equal_nan=True)
    for x, y in zip(xg, xa):
        assert np.array_equal(x[act], y[act])
    assert np.array_equal(g.acc[act], acc[act]) and np.all(g.sc[SC['t']][act] == mir.sc[SC['t']][act] + 1.0)
    print("accepted", acc[act].sum(), "of", act.size)


@pytest.mark.gpu
def test_whole_runs():
    """smc_glms at N = 3 ... 4 neurons, K = 8: two runs give equal bits, a neuron subset equals the matching rows of the
    full run, the 'laplace_dense' run reports its mass and finishes, and what is not served raises."""
    from theano_pyglm_amd.inference import batched_smc as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        kw = dict(n_particles=8, n_leapfrog=3, step_sz=0.05, seed=5, max_stages=400)
        out = B.smc_glms(popn, x, **kw)
        st = popn.last_fit_stats
        print(out['n_stages'], out['n_resampled'], out['log_Z'], out['idle_row_evaluations'], st)
        M, Pn = 4, out['samples'].shape[2]
        Smax = out['betas'].shape[0]
        assert out['finished'].all() and np.all(np.isfinite(out['log_Z'])) and Smax == out['n_stages'].max()
        assert out['samples'].shape == (8, M, Pn) and out['log_weights'].shape == (8, M)
        assert np.allclose(np.sum(np.exp(out['log_weights']), axis=0), 1.0, rtol=1e-12)
        for i in range(M):
            n = out['n_stages'][i]
            b = out['betas'][:n, i]
            assert b[-1] == 1.0 and np.all(np.diff(b) > 0.0) and np.all(np.isnan(out['betas'][n:, i]))
            assert np.all(out['cess'][:n - 1, i] >= 0.9 * 8 * (1.0 - 1e-9)) and np.all(np.isnan(out['accept_rate'][n - 1:, i]))
        assert st['host_reads'] == st['stages'] == Smax and st['stage_launches'] == 3 * Smax
        assert out['n_evals'] == 8 * (1 + 3 * (Smax - 1)) and 0.0 <= out['idle_row_evaluations'] < 1.0
        again = B.smc_glms(popn, x, **kw)
        for key in ('log_Z', 'betas', 'ess', 'cess', 'resampled', 'accept_rate', 'step_sz', 'log_weights', 'samples'):
            assert np.array_equal(out[key], again[key], equal_nan=True), key
        sub = B.smc_glms(popn, x, n_lo=1, n_hi=3, **kw)
        Ss = sub['betas'].shape[0]
        assert np.array_equal(sub['log_Z'], out['log_Z'][1:3]) and np.array_equal(sub['samples'], out['samples'][:, 1:3])
        assert np.array_equal(sub['betas'], out['betas'][:Ss, 1:3], equal_nan=True)
        dn = B.smc_glms(popn, x, mass='laplace_dense', **kw)
        assert dn['mass'] == 'laplace_dense' and dn['finished'].all() and popn.last_fit_stats['factorisations'] >= 1
        print("dense", dn['n_stages'], dn['log_Z'], "identity", out['log_Z'])
        with pytest.raises(ValueError, match="M, P, P"):
            B.smc_glms(popn, x, mass=np.tile(np.eye(Pn), (M, 1, 1)), **kw)
        with pytest.raises(ValueError, match="adapt"):
            B.smc_glms(popn, x, mass='adapt', **kw)
    finally:
        popn.release_data()
    lasso = _population(N=2, T=2.0, gaussian=False)
    try:
        with pytest.raises(ValueError, match="Gaussian"):
            B.smc_glms(lasso, lasso.sample(np.random.RandomState(97)), 2)
    finally:
        lasso.release_data()


class _Fed(SM.Mirror):
    """The mirror fed the device's evaluations: every call of the target is answered with the next recorded (ll, grad) of the
    device run, after the point asked for has been compared with the point the device evaluated."""

    def __init__(self, records, *a, **kw):
        self.records, self.n_fed, self.x_err = records, 0, 0.0
        SM.Mirror.__init__(self, None, *a, **kw)

    def _eval(self, X):
        Xd, ll, grad = self.records[self.n_fed]
        self.n_fed += 1
        self.n_evals += 1
        self.x_err = max(self.x_err, float(np.max(np.abs(X - Xd) / np.max(np.abs(Xd), axis=1, keepdims=True))))
        return ll.copy(), grad.copy()


@pytest.mark.gpu
@pytest.mark.parametrize('mass', [None, 'diag'])
def test_whole_run_equals_the_mirror_stage_by_stage(mass, monkeypatch):
    """smc_glms at N = 4 (neurons 1 .. 3 of 4), K = 8, n_steps = 2, n_leapfrog = 3, identity and an (M, P) mass, against the
    host mirror driven through the same sequence of calls and fed, evaluation by evaluation, the ll and gradient the DEVICE
    computed (recorded at the driver's evaluation loop), so the two runs differ by the rounding of the row kernels alone.
    The mirror's decisions keep their margins (asserted: accept 1e-7, a cumulative weight from a sampling position 1e-9, the
    ESS from its threshold 1e-9 K), so stages, resamplings, ancestors and accepts are EQUAL; every point the mirror asks to
    evaluate is the device's to 1e-10 of the row's largest entry and betas, ESS, CESS, steps, accept rates, log_Z, weights and
    samples agree to 1e-9: rounding of 1e-16 per operation through at most some 20 stages x 2 transitions x 3 leapfrog
    steps of dynamics whose step sizes are far below the curvature scale (no chaos over 6 steps), with 3 digits to spare."""
    import torch
    from theano_pyglm_amd.inference import batched_ais as BA
    from theano_pyglm_amd.inference import batched_smc as B
    from theano_pyglm_amd.inference.batched_bfgs import _Packing
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        records = []
        orig = BA.evaluate_particles

        def recording(handles, bufs, Xt, Weff, K, M, P, n_lo, n_hi, counts):
            out = orig(handles, bufs, Xt, Weff, K, M, P, n_lo, n_hi, counts)
            torch.cuda.current_stream().synchronize()
            R = K * M
            b = bufs[0].cpu().numpy()
            records.append((Xt.cpu().numpy().copy(), b[:R].copy(), b[R:].reshape(R, P).copy()))
            return out
        monkeypatch.setattr(BA, 'evaluate_particles', recording)
        n_lo, n_hi, K = 1, 4, 8
        M = n_hi - n_lo
        Pn = popn.glm.P
        minv = None if mass is None else 0.5 + np.random.default_rng(3).random((M, Pn))
        kw = dict(n_particles=K, n_steps=2, n_leapfrog=3, step_sz=0.05, seed=5, max_stages=400, n_lo=n_lo, n_hi=n_hi)
        out = B.smc_glms(popn, x, mass=minv, **kw)
        monkeypatch.undo()
        prm = _Packing(popn, None).prior_params()
        Bn = (Pn - 1) // popn.N
        mir = _Fed(records, K, M, (popn.N, Bn, 0, prm[1:]), n_lo=n_lo, step0=0.05, seed=5, minv=minv, S=400, n_steps=2,
                   n_leapfrog=3)
        assert mir.P == Pn
        worst = [np.inf, np.inf, np.inf]
        stages = 0
        while mir.nact[0] > 0.0:
            mg = mir.stage()
            stages += 1
            worst[0], worst[1] = min(worst[0], mg[0].min()), min(worst[1], mg[1].min())
            if mir.nact[0] == 0.0:
                break
            for _ in range(2):
                worst[2] = min(worst[2], mir.transition().min())
        res = mir.result()
        print("stages", res['n_stages'], "resampled", res['n_resampled'], "margins", worst, "x_err", mir.x_err)
        assert worst[0] > 1e-9 and worst[1] > 1e-9 * K and worst[2] > 1e-7
        assert mir.n_fed == len(records) and out['n_evals'] == K * len(records) and mir.x_err <= 1e-10
        assert np.array_equal(out['n_stages'], res['n_stages']) and np.array_equal(out['n_resampled'], res['n_resampled'])
        assert np.array_equal(out['resampled'], res['resampled']) and np.array_equal(out['finished'], res['finished'])
        assert res['resampled'].any() and res['n_stages'].min() < res['n_stages'].max()
        for key in ('betas', 'ess', 'cess', 'step_sz', 'accept_rate', 'log_Z'):
            assert np.array_equal(np.isnan(out[key]), np.isnan(res[key])), key
            assert _rel(out[key], res[key]) <= 1e-9, (key, _rel(out[key], res[key]))
        assert np.array_equal(out['accept_rate'] * K * 2, np.round(out['accept_rate'] * K * 2), equal_nan=True)
        assert np.nanmax(np.abs(out['accept_rate'] - res['accept_rate'])) == 0.0          # counts of decisions: equal
        assert np.max(np.abs(out['log_weights'] - res['log_weights'])) <= 1e-9
        assert np.max(np.abs(out['samples'] - res['samples']) / np.max(np.abs(res['samples']), axis=2, keepdims=True)) <= 1e-9
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_dense_factor_follows_the_device_betas(monkeypatch):
    """'laplace_dense': the factor of every move stage is built from the device's vector of betas as it stands after that
    stage -- the stage's record for a neuron that goes on, 1 for a neuron that is done -- once per stage that is followed by
    moves, and never for the last."""
    from theano_pyglm_amd.inference import batched_ais as BA
    from theano_pyglm_amd.inference import batched_smc as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        seen = []
        orig = BA.tempered_factor_rows

        def recording(G, lam, betas, *a):
            assert betas.is_cuda
            seen.append(betas.cpu().numpy().copy())
            return orig(G, lam, betas, *a)
        monkeypatch.setattr(BA, 'tempered_factor_rows', recording)
        out = B.smc_glms(popn, x, n_particles=8, n_leapfrog=3, step_sz=0.05, seed=5, max_stages=400, mass='laplace_dense')
        Smax = out['betas'].shape[0]
        assert out['finished'].all() and len(seen) == Smax - 1 == popn.last_fit_stats['factorisations']
        for s_, b in enumerate(seen):
            want = np.where(np.isnan(out['betas'][s_]), 1.0, out['betas'][s_])
            assert np.array_equal(b, want), (s_, b, want)
    finally:
        popn.release_data()


def test_symbols():
    import ctypes
    import os
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    src = open(os.path.join(SM.ROOT, 'include', 'pyglm_hip.h')).read()
    names = sorted(set(re.findall(r'\b(pgl_smc_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))))
    assert len(names) >= 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n) and n in _lib.SYMBOLS
