"""GPU tests of the NUTS chain (pgl_nuts_* row kernels, inference/batched_nuts.py): the device chain through the C ABI
against the host mirror of the same state machine (tests/nuts_mirror.py: csrc/pglm_nuts.h built by gcc) fed by the
oracle's ll and gradient, and the driver's contract.

Every decision of a transition is a discontinuity.  The mirror records the smallest margin of each kind -- a selection's
|log u - log weight ratio|, a U-turn product relative to |rho| |r|, a leaf's |H - H0 - 1000| -- and the cases are seeded
so that all of them exceed test_gpu_hmc's MARGIN = 1e-4 (asserted), far above the difference between the oracle's and the
device's ll: no decision can flip, so depths, leaf counts, stop reasons, selected leaves, done flags and divergence counts
are equal and the kept samples agree to test_gpu_hmc's 1e-9 of the row's largest entry.  The step sizes: where nothing
adapts (n_warmup = 0) to test_gpu_hmc's rtol 1e-15; where dual averaging runs they are smooth functions of exp(H0 - H)
of every leaf, which differs between the oracle and the device like the samples do, so they are held to the samples'
1e-9 (the bang-bang rule of the HMC chain has no such dependence)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import nuts_mirror as NM
from tests.test_gpu_hmc import GAUSS, LASSO, MARGIN

LOGGED = ('last_depth', 'last_nleaf', 'last_stop', 'last_sel')


def _target(probs, n_lo, n_hi):
    def target(X):
        ll, g = 0.0, 0.0
        for p in probs:
            p.theta = p.theta.copy()
            p.theta[n_lo:n_hi] = X
            a, b = p.oracle_ll_grad(n_lo, n_hi)
            ll, g = ll + a, g + b
        return ll, g
    return target


def mirror_chain(probs, X0, n_lo, n_hi, prm, n_keep, D, step, seed, n_warmup=0, thin=1, minv=None, W=None):
    """-> (the finished mirror, done (launches, M) after every launch, Xt (launches, M, P))."""
    p0 = probs[0]
    mir = NM.Mirror(_target(probs, n_lo, n_hi), X0, n_keep, n_warmup=n_warmup, thin=thin, max_depth=D, n_lo=n_lo,
                    prior=(prm[0], p0.N, p0.B, p0.Dstim, prm[1:]), step0=step, seed=seed, minv=minv, W=W)
    done, xts = [], []
    while not mir.done().all():
        mir.step()
        done.append(mir.done().copy())
        xts.append(mir.Xt.copy())
        assert len(done) < 4000
    return mir, np.array(done), np.array(xts)


def device_chain(probs, X0, n_lo, n_hi, prm, n_keep, D, step, seed, n_launch, n_warmup=0, thin=1, minv=None, W=None):
    """The same chain through the C ABI, n_launch evaluation + step launches; the scalar state and Xt are read after every
    launch (a test's privilege).  -> dict."""
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
            nst = h0.nuts_state_doubles(M, P, D)
            assert nst == (NM.NVEC + 2 * D) * M * P + len(NM.FIELDS) * M
            st = torch.zeros(nst, dtype=f64, device=dev)
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            sc = st[(NM.NVEC + 2 * D) * M * P:].view(len(NM.FIELDS), M)
            Weff = torch.tensor(p0.Weff, dtype=f64, device=dev)
            mv = torch.tensor(minv, dtype=f64, device=dev) if minv is not None else None
            Wd = torch.tensor(W, dtype=f64, device=dev) if W is not None else None
            mvp = mv.data_ptr() if mv is not None else 0
            Wp = Wd.data_ptr() if Wd is not None else 0
            step0 = torch.tensor(np.broadcast_to(np.asarray(step, dtype=float), (M,)).copy(), dtype=f64, device=dev)
            Xt = torch.empty((M, P), dtype=f64, device=dev)
            bufs = [torch.empty(M * (1 + P), dtype=f64, device=dev) for _ in hs]
            samples = torch.zeros((n_keep, M, P), dtype=f64, device=dev)
            stats = torch.zeros((n_keep, 2, M), dtype=f64, device=dev)

            def evaluate(Xe):
                for h, b in zip(hs, bufs):
                    h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), b.data_ptr(), b[M:].data_ptr(), n_lo, n_hi)
                    if b is not bufs[0]:
                        bufs[0].add_(b)
                return bufs[0][:M], bufs[0][M:]

            ll, g = evaluate(st[:M * P].view(M, P))
            h0.nuts_init_dev(st.data_ptr(), M, P, D, n_lo, ll.data_ptr(), g.data_ptr(), prm, mvp, Wp, step0.data_ptr(), seed,
                             n_warmup, thin, n_keep, Xt.data_ptr())
            log = [[] for _ in range(M)]
            done, xts, t_prev = [], [], np.zeros(M)
            for _ in range(n_launch):
                ll, g = evaluate(Xt)
                h0.nuts_step_dev(st.data_ptr(), M, P, D, ll.data_ptr(), g.data_ptr(), prm, mvp, Wp, 0.8, n_warmup, thin, n_keep,
                                 Xt.data_ptr(), samples.data_ptr(), stats.data_ptr())
                stream.synchronize()
                s = sc.cpu().numpy()
                for r in np.flatnonzero(s[NM.SC['t']] != t_prev):
                    log[r].append(tuple(int(s[NM.SC[k], r]) for k in LOGGED) + (s[NM.SC['step'], r], s[NM.SC['last_acc'], r]))
                t_prev = s[NM.SC['t']].copy()
                done.append(s[NM.SC['done']] != 0.0)
                xts.append(Xt.cpu().numpy())
            return {'samples': samples.cpu().numpy(), 'stats': stats.cpu().numpy(), 'sc': sc.cpu().numpy(), 'log': log,
                    'done': np.array(done), 'Xt': np.array(xts), 'q': st[:M * P].view(M, P).cpu().numpy()}
    finally:
        for h in hs:
            h.close()


def compare(probs, X0, n_lo, n_hi, prm, n_keep, D, step, seed, label="", **kw):
    mir, mdone, mxt = mirror_chain(probs, X0, n_lo, n_hi, prm, n_keep, D, step, seed, **kw)
    M = X0.shape[0]
    stops = np.bincount([e['stop'] for r in range(M) for e in mir.log[r]], minlength=5)
    print("%s mirror: %d launches, leapfrogs per row %s, stops (block, tree, depth, divergent) %s, smallest margins "
          "(selection, divergence, U-turn) %s" % (label, len(mdone), mir.sc[NM.SC['n_leapfrog']].astype(int), stops[1:],
                                                 mir.mg[:, :3].min(axis=0)))
    print("%s mirror: %d leaves with a non-finite H" % (label, mir.mg[:, 3].sum()))
    assert mir.mg[:, :3].min() > MARGIN                         # the condition the case was seeded for
    assert mir.mg[:, 3].sum() == 0                              # every divergence is H - H0 > 1000 with a margin: none by overflow
    d = device_chain(probs, X0, n_lo, n_hi, prm, n_keep, D, step, seed, len(mdone) + 3, **kw)
    step_err = acc_err = 0.0
    for r in range(M):
        assert [t[:4] for t in d['log'][r]] == [(e['depth'], e['n_leaf'], e['stop'], e['sel']) for e in mir.log[r]], (label, r)
        sd, sm = np.array([t[4] for t in d['log'][r]]), np.array([e['step'] for e in mir.log[r]])
        step_err = max(step_err, np.max(np.abs(sd / sm - 1.0)))
        acc_err = max(acc_err, np.max(np.abs(np.array([t[5] for t in d['log'][r]]) - np.array([e['alpha'] for e in mir.log[r]]))))
    print("%s device against mirror: largest relative step error %.3e, largest acceptance statistic error %.3e"
          % (label, step_err, acc_err))
    assert step_err <= (1e-9 if kw.get('n_warmup', 0) else 1e-15)
    assert acc_err <= 1e-9                                      # (a mean of min(1, exp(H0 - H)): the samples' tolerance)
    n = len(mdone)
    assert np.array_equal(d['done'][:n], mdone) and d['done'][n:].all()
    # idle rows: nothing of them moves, and their Xt row stays at their current point
    err = np.max(np.abs(d['Xt'][:n] - mxt) / np.max(np.abs(mxt), axis=2, keepdims=True))
    assert err <= 1e-9
    for k in range(n, n + 3):
        assert np.array_equal(d['Xt'][k], d['q'])
    for r in range(M):
        k0 = int(np.argmax(mdone[:, r]))
        assert np.all(d['Xt'][k0:, r] == d['Xt'][k0, r]) and np.array_equal(d['Xt'][k0, r], d['q'][r])
    err = np.max(np.abs(d['samples'] - mir.samples) / np.max(np.abs(mir.samples), axis=2, keepdims=True))
    print("%s device against mirror: largest error relative to the row's largest entry %.3e" % (label, err))
    assert err <= 1e-9
    assert np.array_equal(d['stats'], mir.stats)
    for k in ('t', 'n_leapfrog', 'n_div', 'done'):
        assert np.array_equal(d['sc'][NM.SC[k]], mir.sc[NM.SC[k]]), k
    return mir, d, stops


def _problem(N, nT, kind, seed, **kw):
    if kind == 'exp':
        return H.Problem(N, nT, H.std_ibasis(), kind='exp', seed=seed, bias_mu=3.0, w_scale=0.05, **kw)
    return H.Problem(N, nT, H.std_ibasis(), kind=kind, seed=seed, **kw)


def _prior(kind, name):
    prm = GAUSS if name == 'gauss' else LASSO
    return (prm[0], 3.0 if kind == 'exp' else 20.0) + prm[2:]


def _dense_factor(M, P, seed):
    """Lower-triangular factors with junk in the strict upper triangle (never read)."""
    rng = np.random.default_rng(seed)
    W = np.zeros((M, P, P))
    for m in range(M):
        L = np.tril(0.15 * rng.standard_normal((P, P)) / np.sqrt(P))
        L[np.diag_indices(P)] = 0.6 + 0.8 * rng.random(P)
        W[m] = L + np.triu(np.full((P, P), 1e30), 1)
    return W


# name -> (step, seed): seeded on the CPU so that every margin of the mirror exceeds MARGIN
SEEDS = {'explinear-gauss': (1.2, 1), 'explinear-lasso': (1.2, 2),   # smallest margin of the mirror 3.2e-3, 1.3e-3
         'exp-gauss': (0.24, 1), 'exp-lasso': (0.24, 2),             # 1.2e-3, 2.6e-3; 20 and 10 divergent transitions of 40
         'minv': (0.5, 3), 'dense': (0.7, 2), 'warm': (0.2, 1),      # 5.1e-4, 7.7e-4, 2.8e-3
         'two': (0.6, 2), 'P71': (0.6, 2), 'P261': (0.05, 1), 'M1': (0.6, 4)}     # 1.9e-3, 5.9e-3, 5.9e-2, 6.9e-2


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
@pytest.mark.parametrize('prior', ['gauss', 'lasso'])
def test_device_chain_equals_host_mirror(kind, prior):
    """N = 5 (P = 26, below one wavefront), nT = 2 000, max_depth 4, 8 transitions; rows finish at different launches."""
    p = _problem(5, 2000, kind, 31)
    step, seed = SEEDS['%s-%s' % (kind, prior)]
    mir, d, stops = compare([p], p.theta.copy(), 0, 5, _prior(kind, prior), 8, 4, step, seed, label="%s/%s" % (kind, prior))
    first = np.argmax(d['done'], axis=0)
    assert len(set(first)) > 1                                  # the rows do not finish together


@pytest.mark.gpu
def test_diagonal_mass_subset_of_neurons_and_warmup_with_thinning():
    """n_lo = 1, minv, n_warmup = 5, thin = 2: dual averaging and the kernel's own sample indexing."""
    p = _problem(5, 2000, 'explinear', 31)
    minv = 0.25 + 1.5 * np.random.default_rng(43).random((3, p.P))
    step, seed = SEEDS['minv']
    mir, d, _ = compare([p], p.theta[1:4].copy(), 1, 4, _prior('explinear', 'gauss'), 4, 4, step, seed, n_warmup=5, thin=2,
                        minv=minv, label="minv")
    assert np.all(d['sc'][NM.SC['t']] == 13) and len(set(d['sc'][NM.SC['step']])) == 3


@pytest.mark.gpu
def test_dense_mass_with_junk_above_the_diagonal():
    p = _problem(5, 2000, 'explinear', 31)
    step, seed = SEEDS['dense']
    compare([p], p.theta.copy(), 0, 5, _prior('explinear', 'lasso'), 6, 4, step, seed, W=_dense_factor(5, p.P, 3), label="dense")


@pytest.mark.gpu
def test_dense_mass_with_warmup():
    p = _problem(5, 2000, 'exp', 31)
    step, seed = SEEDS['warm']
    compare([p], p.theta.copy(), 0, 5, _prior('exp', 'gauss'), 3, 3, step, seed, n_warmup=4, thin=2, W=_dense_factor(5, p.P, 5),
            label="dense, warm-up")


@pytest.mark.gpu
def test_two_data_sequences_sum():
    p1 = _problem(5, 2000, 'explinear', 31)
    p2 = _problem(5, 1008, 'explinear', 41)
    p2.theta, p2.Weff = p1.theta, p1.Weff
    step, seed = SEEDS['two']
    compare([p1, p2], p1.theta.copy(), 0, 5, _prior('explinear', 'gauss'), 4, 4, step, seed, label="two sequences")


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [False, True])
def test_row_longer_than_a_wavefront(dense):
    """P = 71: not a multiple of 64.  N = 8, Dstim = 30, nT = 1 000."""
    p = _problem(8, 1000, 'explinear', 37, Dstim=30)
    assert p.P == 71
    step, seed = SEEDS['P71']
    compare([p], p.theta.copy(), 0, 8, _prior('explinear', 'lasso'), 3, 3, step, seed, W=_dense_factor(8, 71, 7) if dense else None,
            label="P=71")


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [False, True])
def test_strided_row_loops(dense):
    """P = 261 > the 256 threads of a row kernel's workgroup: N = 6, Dstim = 230, nT = 512, rows 2 .. 4."""
    p = _problem(6, 512, 'explinear', 37, Dstim=230)
    assert p.P == 261
    step, seed = SEEDS['P261']
    compare([p], p.theta[2:5].copy(), 2, 5, _prior('explinear', 'gauss'), 3, 3, step, seed,
            W=_dense_factor(3, 261, 9) if dense else None, label="P=261")


@pytest.mark.gpu
def test_one_row():
    p = _problem(5, 2000, 'explinear', 31)
    step, seed = SEEDS['M1']
    compare([p], p.theta[3:4].copy(), 3, 4, _prior('explinear', 'gauss'), 5, 4, step, seed, label="M=1")


# ---- the driver --------------------------------------------------------------------------------------------------
def _population(N=4, T=6.0, seed=89):
    from tests.test_gpu_hvp import _std_population
    return _std_population(N, T, seed, nlin='exp', bias_mu=3.0)


@pytest.mark.gpu
def test_driver_contract():
    from theano_pyglm_amd.inference import batched_nuts as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        X0 = popn.theta_matrix(x)
        P = popn.glm.P
        kw = dict(n_warmup=6, max_depth=4, step_sz=0.05, thin=2, seed=5)
        mass = B._laplace_minv(popn, x, 0, 4, 1e-8)
        out = B.sample_glms_nuts(popn, x, 5, mass=mass, **kw)
        st = popn.last_fit_stats
        print(st, out['accept_rate'], out['step'], out['depth'].T, out['launches'], out['idle_row_evaluations'])
        assert out['samples'].shape == (5, 4, P) and np.all(np.isfinite(out['samples']))
        assert out['depth'].shape == (5, 4) and np.all(out['depth'] >= 1) and np.all(out['depth'] <= 4)
        assert np.all(out['n_leapfrog'] >= 1) and np.all(out['n_leapfrog'] <= 2 ** out['depth'] - 1)
        assert np.all(out['step'] >= 1e-4) and np.all(out['step'] <= 10.0) and np.array_equal(out['step'], out['step_sz'])
        assert np.all(out['accept_rate'] > 0.0) and np.all(out['accept_rate'] <= 1.0) and np.all(out['divergent'] >= 0)
        # launches: the longest row's leapfrog steps, plus the flag-read slack (every POLL launches, one window late)
        longest = st['leapfrog_steps'].max()
        assert longest <= out['launches'] < longest + 2 * B.POLL and out['launches'] % B.POLL == 0
        assert out['n_evals'] == out['launches'] + 1 == st['ll_grad_launches']
        assert out['idle_row_evaluations'] == int(np.sum(out['launches'] - st['leapfrog_steps']))
        assert np.array_equal(popn.theta_matrix(x), X0)         # x is untouched
        s = B.summarize(out['samples'])
        assert s['mean'].shape == (4, P)
        xx = dict(x)
        xx['glms'] = B.samples_to_states(popn, x, out['samples'], 3)
        assert np.array_equal(popn.theta_matrix(xx), out['samples'][3])
        # two runs give the same bits; a subset of the neurons gives the matching rows
        again = B.sample_glms_nuts(popn, x, 5, mass=mass, **kw)
        sub = B.sample_glms_nuts(popn, x, 5, mass=mass[1:3], n_lo=1, n_hi=3, **kw)
        for k in ('samples', 'step', 'depth', 'n_leapfrog', 'divergent', 'accept_rate'):
            assert np.array_equal(again[k], out[k]), k
            assert np.array_equal(sub[k], out[k][1:3] if out[k].ndim == 1 else out[k][:, 1:3]), k
        # the command-line table: synth_map --nuts
        from theano_pyglm_amd.harness import synth_map
        table = synth_map.nuts_bias_table(popn, x, 6, mass='laplace', n_warmup=6, max_depth=4, seed=5).split("\n")
        print("\n".join(table))
        assert table[0].startswith("NUTS: 6 draws per neuron") and "median depth" in table[0] and "divergent" in table[0]
        assert "depth  divergent" in table[1] and len(table) == 2 + 4
        assert [int(ln.split()[0]) for ln in table[2:]] == [0, 1, 2, 3]
        # the dense mass, both routes to its factor
        for dev_factor in (False, True):
            res = B.sample_glms_nuts(popn, x, 3, n_warmup=3, max_depth=3, step_sz=0.05, mass='laplace_dense', seed=3,
                                     factor_on_device=dev_factor)
            assert res['samples'].shape == (3, 4, P) and np.all(np.isfinite(res['samples']))
            assert popn.last_fit_stats['mass'] == 'dense' and res['dense_rows'].shape == (4,)
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_unsupported_inputs_raise():
    from theano_pyglm_amd.inference import batched_nuts as B
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):     # an 'st' stimulus / Dirichlet impulses
        p2 = Population(make_model(name, N=2, dt=0.001))
        assert not B.supported(p2)
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            B.sample_glms_nuts(p2, p2.sample(np.random.RandomState(1)), 2)
    popn = _population(N=2, T=2.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                B.sample_glms_nuts(popn, x, 2)
        finally:
            popn.set_time_shard(None)
        with pytest.raises(ValueError, match="empty"):
            B.sample_glms_nuts(popn, x, 2, n_lo=1, n_hi=1)
        with pytest.raises(ValueError, match="max_depth"):
            B.sample_glms_nuts(popn, x, 2, max_depth=11)
    finally:
        popn.release_data()
