"""GPU tests of annealed importance sampling with a dense mass matrix (pgl_tri_matvec_shared_dev, pgl_ais_dense_* and the
'laplace_dense' / (M, P, P) forms of inference/batched_ais.py: mass): the shared triangular product against numpy and
against the one-row pgl_tri_matvec_dev, the device run through the C ABI against the host mirror of the same state machine
(tests/ais_dense_mirror.py: csrc/pglm_ais_dense.h built by gcc) fed by the oracle's ll and gradient, the dense run with a
diagonal factor against the diagonal device run, and the driver's contract.

As in tests/test_gpu_ais.py the cases are seeded so that in the mirror every decision keeps |log u - (H0 - H1)| > 1e-4
(asserted) and both outcomes occur.  The device always gets its factors with NaN above the diagonal: a finite run has
never read them."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import ais_mirror as AM
from tests import ais_dense_mirror as AD
from tests.test_gpu_ais import BETAS, MARGIN, _prior, _problem, _table, oracle_target

TILE = 64                                                     # PGL_TRI_TILE: outputs per workgroup of the products
CHUNK = 8                                                     # PGL_TRI_SHARED_KC: particles per pass over a part of W
KS = [1, 2, 3, 8, 11]                                         # 11 > CHUNK: a second, partial pass


def _nan_above(W):
    Wn = np.array(W, dtype=float)
    iu = np.triu_indices(Wn.shape[-1], 1)
    Wn[..., iu[0], iu[1]] = np.nan
    return Wn


def _tempered_factors(M, P, prm, NBD, betas, seed):
    """One stack of factors per temperature with moves, from a random SPD matrix per neuron standing in for minus the
    Hessian of ll: G = 40 (R R^T / P + I), W_j the lower factor of (beta_j G + Lambda)^-1 (batched_ais.tempered_factor on its
    numpy backend).  -> {j: (M, P, P)}."""
    from theano_pyglm_amd.inference import batched_ais as BA
    from theano_pyglm_amd.inference import laplace as LP
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((M, P, P))
    G = 40.0 * (np.matmul(R, np.swapaxes(R, 1, 2)) / P + np.eye(P)[None])
    lam = BA.prior_precision(prm, *NBD)
    out = {}
    for j in range(1, len(betas) - 1):
        W, info = BA.tempered_factor(G, lam, betas[j], 1e-8, LP.numpy_factor, LP.numpy_inverse, np, np.eye(P))
        assert np.all(info == 0)
        out[j] = W
    return out


# ---- the shared product ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 255, 256, 257, 281, 641])
def test_shared_product_against_numpy_and_the_one_row_product(handle, P):
    """y = W x and W^T x for K in (1, 2, 3, 8, 11) particles of M = 1 and 3 neurons with NaN above the diagonal: within
    1e-13 sum|w||x| of an extended-precision numpy product per output (the bound of tests/test_gpu_hmc_dense.py), the same
    bits twice, and row (k, i) equal to the one-row pgl_tri_matvec_dev call with W_i bit for bit."""
    import torch
    assert TILE == 64 and max(KS) > CHUNK
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    rng = np.random.default_rng(300 + P)
    Kmax = max(KS)
    W = rng.standard_normal((3, P, P))
    x = rng.standard_normal((Kmax, 3, P))
    Wd = torch.tensor(_nan_above(W), dtype=f64, device=dev)
    xd = torch.tensor(x, dtype=f64, device=dev)
    L = np.tril(W).astype(np.longdouble)
    xl = x.astype(np.longdouble)
    torch.cuda.synchronize()
    for trans in (0, 1):
        A = np.swapaxes(L, 1, 2) if trans else L
        ref = np.einsum('mij,kmj->kmi', A, xl)
        mag = np.einsum('mij,kmj->kmi', np.abs(A), np.abs(xl)).astype(float)
        one = torch.full((Kmax, 3, P), np.nan, dtype=f64, device=dev)
        torch.cuda.synchronize()                                # (the fill runs on torch's stream, the products on the handle's)
        for k in range(Kmax):
            for i in range(3):
                handle.tri_matvec_dev(Wd[i].data_ptr(), 1, P, trans, xd[k, i].data_ptr(), one[k, i].data_ptr())
        handle.sync()
        one = one.cpu().numpy()
        worst = 0.0
        for M in (1, 3):
            for K in KS:
                xs = xd[:K, :M].contiguous()
                ys = [torch.full((K * M, P), np.nan, dtype=f64, device=dev) for _ in range(2)]
                torch.cuda.synchronize()
                for y in ys:
                    handle.tri_matvec_shared_dev(Wd.data_ptr(), M, K, P, trans, xs.data_ptr(), y.data_ptr())
                handle.sync()
                y0 = ys[0].cpu().numpy().reshape(K, M, P)
                assert np.all(np.isfinite(y0))
                assert np.array_equal(y0, ys[1].cpu().numpy().reshape(K, M, P))
                assert np.array_equal(y0, one[:K, :M])
                worst = max(worst, np.max(np.abs((y0 - ref[:K, :M]).astype(float)) / mag[:K, :M]))
        print("P = %d trans = %d: largest error / sum|w||x| = %.3e" % (P, trans, worst))
        assert worst <= 1e-13


# ---- the run through the C ABI ----------------------------------------------------------------------------------------
def mirror_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, Ws, particle0=0):
    p0 = probs[0]
    mir = AD.DenseMirror(oracle_target(probs, n_lo, n_hi), K, n_hi - n_lo, (p0.N, p0.B, p0.Dstim, prm[1:]), lambda j: Ws[j],
                         n_lo=n_lo, particle0=particle0, step0=0.1, seed=seed)
    out = mir.run(betas, n_steps, L, adapt=False, step_table=table)
    out['draws'] = mir.draws
    out['ll_seen'] = np.array(mir.ll_seen)
    return out


def device_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, Ws=None, minv=None, particle0=0):
    """The run through the C ABI: pgl_ais_dense_* with the factors Ws[j] (NaN above the diagonal), or, Ws None, pgl_ais_* with
    the diagonal minv.  The decisions are read after every transition (a test's privilege).  -> dict as the mirror's."""
    import torch
    p0 = probs[0]
    M, P, R = n_hi - n_lo, p0.P, K * (n_hi - n_lo)
    J = len(betas) - 1
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    hs = [p.device(0) for p in probs]
    stream = torch.cuda.Stream(dev)
    try:
        for h in hs:
            h.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            h0 = hs[0]
            st = torch.zeros(h0.ais_state_doubles(R, P), dtype=f64, device=dev)
            sc = st[6 * R * P:].view(15, R)
            Weff = torch.tensor(p0.Weff, dtype=f64, device=dev)
            tab = torch.tensor(np.asarray(table, dtype=float).reshape(J - 1, M), dtype=f64, device=dev)
            Wd = None if Ws is None else dict((j, torch.tensor(_nan_above(w), dtype=f64, device=dev)) for j, w in Ws.items())
            md = None if minv is None else torch.tensor(minv, dtype=f64, device=dev)
            Xt = torch.empty((R, P), dtype=f64, device=dev)
            bufs = [torch.empty(R * (1 + P), dtype=f64, device=dev) for _ in hs]
            accepts = torch.zeros((J - 1, R), dtype=f64, device=dev)
            steps = torch.zeros((J - 1, R), dtype=f64, device=dev)

            def evaluate():
                for h, b in zip(hs, bufs):
                    for k in range(K):
                        h.ll_grad_dev(Xt[k * M].data_ptr(), Weff.data_ptr(), b[k * M:].data_ptr(), b[R + k * M * P:].data_ptr(),
                                      n_lo, n_hi)
                    if b is not bufs[0]:
                        bufs[0].add_(b)
                return bufs[0].data_ptr(), bufs[0][R:].data_ptr()

            sp = st.data_ptr()
            h0.ais_init_dev(sp, K, M, P, n_lo, particle0, prm, 0.1, seed, Xt.data_ptr())
            draws = Xt.cpu().numpy()
            ll, g = evaluate()
            h0.ais_start_dev(sp, K, M, P, ll, g, prm)
            accepted = []
            for j in range(1, J + 1):
                h0.ais_temper_dev(sp, K, M, P, prm, betas[j], tab[j - 1].data_ptr() if j < J else 0)
                if j == J:
                    break
                for _ in range(n_steps):
                    if Wd is not None:
                        h0.ais_dense_begin_dev(sp, K, M, P, Wd[j].data_ptr(), Xt.data_ptr())
                    else:
                        h0.ais_begin_dev(sp, K, M, P, md.data_ptr() if md is not None else 0, Xt.data_ptr())
                    for i in range(L):
                        ll, g = evaluate()
                        if Wd is not None:
                            h0.ais_dense_leap_dev(sp, K, M, P, Wd[j].data_ptr(), ll, g, prm, i == L - 1, False, Xt.data_ptr(),
                                                  accepts[j - 1].data_ptr(), steps[j - 1].data_ptr())
                        else:
                            h0.ais_leap_dev(sp, K, M, P, md.data_ptr() if md is not None else 0, ll, g, prm, i == L - 1, False,
                                            Xt.data_ptr(), accepts[j - 1].data_ptr(), steps[j - 1].data_ptr())
                    stream.synchronize()
                    accepted.append(sc[AM.SC['acc']].cpu().numpy() != 0.0)
            stream.synchronize()
            return {'log_weights': sc[AM.SC['logw']].cpu().numpy().reshape(K, M), 'samples': st[:R * P].cpu().numpy().reshape(K, M, P),
                    'accepts': accepts.cpu().numpy(), 'steps': steps.cpu().numpy(),
                    'accepted': np.array(accepted, dtype=bool).reshape(-1, R), 'draws': draws}
    finally:
        for h in hs:
            h.close()


def _close(d, m, scale, label):
    """The project's bounds: points within 1e-9 of the row's largest entry, log w within 1e-9 max(1, |ll|)."""
    err = np.max(np.abs(d['samples'] - m['samples']) / np.max(np.abs(m['samples']), axis=2, keepdims=True))
    werr = np.max(np.abs(d['log_weights'] - m['log_weights']))
    print("%s: points %.3e of the row's largest entry, log w %.3e (bound %.3e)" % (label, err, werr, 1e-9 * scale))
    assert err <= 1e-9
    assert werr <= 1e-9 * scale


def compare(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, Ws, label=""):
    m = mirror_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, Ws)
    print("%s mirror: accepted %d of %d, smallest margin %.3e" % (label, m['accepted'].sum(), m['accepted'].size, m['margins'].min()))
    assert np.all(np.isfinite(m['ll_seen'][0]))                 # ll is finite at every prior draw
    assert m['margins'].min() > MARGIN                          # the condition the case was seeded for
    assert m['accepted'].any() and not m['accepted'].all()      # both outcomes of the decision
    d = device_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, Ws)
    assert np.array_equal(d['accepted'], m['accepted'])
    assert np.array_equal(d['accepts'], m['accepts']) and np.array_equal(d['steps'], m['steps'])
    finite = m['ll_seen'][np.isfinite(m['ll_seen'])]
    _close(d, m, max(1.0, np.max(np.abs(finite))), label + " device against mirror")
    return m, d


# (kind) -> (frozen step per temperature, seed): seeded on the CPU for a mix of decisions with margins > 1e-4
CASES = {
    'explinear': ([0.9, 0.9, 0.9], 3),                          # mirror: 70 of 90 accepted, smallest margin 6.1e-3
    'exp': ([0.9, 0.9, 0.9], 2),                                # 76 of 90, 4.5e-3
}
WIDE = ([0.7], 3)                                               # N = 70: 67 of 140, 5.0e-3
TWO_SEQ = ([0.9], 3)                                            # 15 of 20, 1.9e-2


def _case_factors(p, prm, betas, seed=7, n_lo=0, n_hi=None):
    n_hi = p.N if n_hi is None else n_hi
    Ws = _tempered_factors(p.N, p.P, prm, (p.N, p.B, p.Dstim), betas, seed)
    return dict((j, np.ascontiguousarray(w[n_lo:n_hi])) for j, w in Ws.items())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
def test_device_run_equals_host_mirror(kind):
    """N = 5, nT = 2 000, K = 3, betas (0, 0.01, 0.1, 0.5, 1), n_steps = 2, n_leapfrog = 3, frozen steps, one W per
    temperature."""
    p = _problem(5, 2000, kind, 31)
    steps, seed = CASES[kind]
    prm = _prior(kind)
    compare([p], 3, 0, 5, prm, BETAS, 2, 3, _table(steps, 5), seed, _case_factors(p, prm, BETAS), label=kind)


@pytest.mark.gpu
def test_wide_rows():
    """P = 281: more than one tile of the products and more than the 256 threads of a row kernel.  N = 70, B = 4, nT = 512,
    K = 2, one transition of 3 steps."""
    p = _problem(70, 512, 'explinear', 37, ibasis=H.std_ibasis()[:, :4])
    assert p.P == 281
    steps, seed = WIDE
    prm = _prior('explinear')
    betas = [0.0, 0.5, 1.0]
    compare([p], 2, 0, 70, prm, betas, 1, 3, _table(steps, 70), seed, _case_factors(p, prm, betas, seed=9), label="N=70")


@pytest.mark.gpu
def test_diagonal_factor_equals_the_diagonal_device_run():
    """W = diag(sqrt(minv)): the dense device run against pgl_ais_* with minv -- the same decisions, accept counts and steps,
    points and weights at the bounds of the mirror comparison (not the same bits: the products sum zeros in another order
    than the diagonal kernel multiplies)."""
    p = _problem(5, 2000, 'explinear', 31)
    prm = _prior('explinear')
    minv = (0.25 + 1.5 * np.random.default_rng(43).random((5, p.P))) * 0.01
    W = np.zeros((5, p.P, p.P))
    W[:, np.arange(p.P), np.arange(p.P)] = np.sqrt(minv)
    tab = _table([0.5, 0.5, 0.5], 5)
    g = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, 2, minv=minv)
    d = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, 2, Ws={1: W, 2: W, 3: W})
    print("diagonal run: accepted %d of %d" % (g['accepted'].sum(), g['accepted'].size))
    assert g['accepted'].any()
    assert np.array_equal(d['accepted'], g['accepted'])
    assert np.array_equal(d['accepts'], g['accepts']) and np.array_equal(d['steps'], g['steps'])
    _close(d, g, max(1.0, np.max(np.abs(g['log_weights']))), "dense against diagonal")


@pytest.mark.gpu
def test_subsets_on_the_device():
    """A neuron range, a particle range and a repeat: the bits of the matching rows of the full run.  exp, for the reason
    tests/test_gpu_ais.py: test_a_row_that_cannot_move states."""
    p = _problem(5, 2000, 'exp', 31)
    prm = _prior('exp')
    steps, seed = CASES['exp']
    tab = _table(steps, 5)
    Ws = _case_factors(p, prm, BETAS)
    full = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed, Ws)
    again = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed, Ws)
    for key in ('log_weights', 'samples', 'accepted', 'draws'):
        assert np.array_equal(full[key], again[key])
    sub = device_run([p], 3, 1, 4, prm, BETAS, 2, 3, tab[:, 1:4], seed, _case_factors(p, prm, BETAS, n_lo=1, n_hi=4))
    assert np.array_equal(sub['log_weights'], full['log_weights'][:, 1:4])
    assert np.array_equal(sub['samples'], full['samples'][:, 1:4])
    part = device_run([p], 2, 0, 5, prm, BETAS, 2, 3, tab, seed, Ws, particle0=1)
    assert np.array_equal(part['log_weights'], full['log_weights'][1:3])
    assert np.array_equal(part['samples'], full['samples'][1:3])
    assert full['accepted'].any() and np.all(np.isfinite(full['log_weights']))


@pytest.mark.gpu
def test_two_data_sequences_sum():
    """Two recordings of the same population: their [ll | grad] blocks are summed before the row kernels see them."""
    p1 = _problem(5, 2000, 'explinear', 31)
    p2 = _problem(5, 1008, 'explinear', 41)
    p2.theta, p2.Weff = p1.theta, p1.Weff
    steps, seed = TWO_SEQ
    prm = _prior('explinear')
    betas = [0.0, 0.1, 1.0]
    compare([p1, p2], 2, 0, 5, prm, betas, 2, 3, _table(steps, 5), seed, _case_factors(p1, prm, betas), label="two sequences")


# ---- the driver --------------------------------------------------------------------------------------------------
def _population(N=4, T=6.0, seed=89):
    """The population of tests/test_gpu_ais.py: _population: a 4-neuron exp standard_glm with N(0, 1) impulse priors."""
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    model['nonlinearity']['type'] = 'exp'
    model['bias']['mu'] = 3.0
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    popn = Population(model)
    nT = int(round(T / 0.001))
    S = np.minimum(np.random.default_rng(seed).poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': None, 'dt_stim': 0.1})
    return popn


DRIVER = dict(n_particles=3, betas=[0.0, 0.001, 0.01, 0.1, 0.4, 1.0], n_steps=2, n_leapfrog=2, step_sz=0.3, seed=5)


@pytest.mark.gpu
def test_driver_laplace_dense():
    """mass='laplace_dense' on the parent commit raises ValueError ("mass: None, 'laplace' or an (M, P) array")."""
    from theano_pyglm_amd.inference import batched_ais as B
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        x0 = copy.deepcopy(x)
        K, L, n_steps, betas = DRIVER['n_particles'], DRIVER['n_leapfrog'], DRIVER['n_steps'], DRIVER['betas']
        J = len(betas) - 1
        out = B.ais_glms(popn, x, mass='laplace_dense', **DRIVER)
        st = popn.last_fit_stats
        print(st)
        P = popn.glm.P
        assert out['mass'] == 'laplace_dense' == st['mass']
        assert out['log_Z'].shape == out['log_Z_se'].shape == out['ess'].shape == out['log_prior_norm'].shape == (4,)
        assert out['log_weights'].shape == (K, 4) and out['samples'].shape == (K, 4, P)
        assert out['accept_rate'].shape == out['step_sz'].shape == (J - 1, 4) and np.array_equal(out['betas'], betas)
        assert out['dense_rows'].shape == (J - 1, 4) and out['dense_rows'].dtype == bool
        assert out['dense_rows'].all()                           # (an exp nonlinearity under Gaussian priors: concave everywhere)
        assert np.all(np.isfinite(out['log_weights'])) and np.all(np.isfinite(out['samples']))
        assert np.all(np.isfinite(out['log_Z'])) and np.all(np.isfinite(out['log_Z_se']))
        assert np.all(out['accept_rate'] >= 0.0) and np.all(out['accept_rate'] <= 1.0) and np.any(out['accept_rate'] > 0.0)
        n_trans = (J - 1) * n_steps
        assert out['n_evals'] == st['ll_grad_launches'] == (K + 1) * (1 + n_trans * L)
        assert st['row_launches'] == 2 * (2 + J + n_trans * (L + 1))
        assert st['factorisations'] == 2 * (J - 1)              # the pilot's and the main run's: recomputed, not kept
        assert st['product_launches'] == 2 * n_trans * (2 * L + 1)
        assert st['host_syncs_in_run'] == 0
        assert np.array_equal(popn.theta_matrix(x), popn.theta_matrix(x0))
        again = B.ais_glms(popn, x, mass='laplace_dense', **DRIVER)
        for key in ('log_weights', 'samples', 'accept_rate', 'step_sz', 'dense_rows'):
            assert np.array_equal(again[key], out[key])
        # the evidence: printed, as tests/test_gpu_ais.py: test_driver_shapes_counts_and_evidence prints it for the diagonal
        # run -- that test asserts no bound (x is a prior draw, not a mode, and K = 3), so none is asserted here
        lap = np.array([r['log_evidence'] for r in laplace_glms(popn, x)])
        for n in range(4):
            print("neuron %d: AIS log_Z + log_prior_norm %.3f +- %.3f (ess %.2f), Laplace %.3f"
                  % (n, out['log_Z'][n] + out['log_prior_norm'][n], out['log_Z_se'][n], out['ess'][n], lap[n]))
        # the diagonal forms keep their record
        B.ais_glms(popn, x, 2, betas=[0.0, 0.5, 1.0], n_leapfrog=2, step_sz=0.05, pilot=False)
        assert popn.last_fit_stats['mass'] == 'identity' and popn.last_fit_stats['product_launches'] == 0
        # a neuron range and a particle range on the frozen table, no pilot: one factorisation per temperature.  (Equal BITS
        # of a sub-range are asserted where the factors are given, test_driver_explicit_matrices_and_bad_masses: the
        # Hessian of a sub-range is not promised to the bit.)
        sub = B.ais_glms(popn, x, mass='laplace_dense', **dict(DRIVER, n_particles=2, step_sz=out['step_sz'][:, 1:3]),
                         pilot=False, particle0=1, n_lo=1, n_hi=3)
        assert sub['log_weights'].shape == (2, 2) and sub['dense_rows'].shape == (J - 1, 2) and sub['dense_rows'].all()
        assert popn.last_fit_stats['factorisations'] == J - 1
        assert np.allclose(sub['log_weights'], out['log_weights'][1:3, 1:3], rtol=0.0,
                           atol=1e-9 * max(1.0, np.max(np.abs(out['log_weights']))))
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_driver_fallback_row(monkeypatch):
    """A neuron whose beta G + Lambda does not factor runs on the diagonal rule at that temperature; the other neurons'
    bits are those of the clean run."""
    from theano_pyglm_amd.inference import batched_ais as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        ref = B.ais_glms(popn, x, mass='laplace_dense', **DRIVER)
        hessians = B._ll_hessians

        def not_pd(population, torch, dev, handles, xx, n_lo, n_hi, P):
            G = hessians(population, torch, dev, handles, xx, n_lo, n_hi, P)
            G[2 - n_lo, 0, 1] = G[2 - n_lo, 1, 0] = 1e12          # (the diagonal stays: the fallback is the 'laplace' rule's)
            return G
        monkeypatch.setattr(B, '_ll_hessians', not_pd)
        out = B.ais_glms(popn, x, mass='laplace_dense', **DRIVER)
        want = np.ones_like(ref['dense_rows'])
        want[:, 2] = False
        assert np.array_equal(out['dense_rows'], want)
        others = [0, 1, 3]
        for key in ('log_weights', 'samples', 'step_sz', 'accept_rate'):
            assert np.array_equal(out[key][..., others, :] if key == 'samples' else out[key][..., others],
                                  ref[key][..., others, :] if key == 'samples' else ref[key][..., others])
        assert np.all(np.isfinite(out['samples'][:, 2])) and np.all(np.isfinite(out['log_weights'][:, 2]))
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_driver_explicit_matrices_and_bad_masses():
    """(M, P, P) = Lambda^-1 against mass = (M, P) with the same diagonal: the same decisions, weights to rounding.  Bad
    masses raise."""
    from theano_pyglm_amd.inference import batched_ais as B
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        P = popn.glm.P
        bias, imp = popn.glm.bias_model, popn.glm.imp_model.prior
        minv = np.tile(np.concatenate(([float(bias.sig_bias) ** 2], np.full(P - 1, float(imp.sigma) ** 2))), (4, 1))
        Sig = np.zeros((4, P, P))
        Sig[:, np.arange(P), np.arange(P)] = minv
        kw = dict(DRIVER, step_sz=0.05, pilot=False)
        diag = B.ais_glms(popn, x, mass=minv, **kw)
        assert diag['mass'] == 'diagonal' and 'dense_rows' not in diag
        dense = B.ais_glms(popn, x, mass=Sig, **kw)
        assert dense['mass'] == 'dense' and 'dense_rows' not in dense and popn.last_fit_stats['factorisations'] == 0
        print(diag['accept_rate'], np.max(np.abs(dense['log_weights'] - diag['log_weights'])))
        assert np.array_equal(dense['accept_rate'], diag['accept_rate'])
        assert np.max(np.abs(dense['log_weights'] - diag['log_weights'])) <= 1e-9 * max(1.0, np.max(np.abs(diag['log_weights'])))
        err = np.max(np.abs(dense['samples'] - diag['samples']) / np.max(np.abs(diag['samples']), axis=2, keepdims=True))
        assert err <= 1e-9
        sub = B.ais_glms(popn, x, mass=Sig[1:3], n_lo=1, n_hi=3, **kw)
        assert np.array_equal(sub['log_weights'], dense['log_weights'][:, 1:3])
        not_pd, asym = -Sig, Sig.copy()
        asym[0, 0, 1] += 1.0
        for bad in (Sig[:3], Sig[:, :P - 1, :P - 1], np.ones((4, P, P + 1)), not_pd, asym, minv[:3], minv[:, :P - 1], -minv,
                    'dense'):
            with pytest.raises(ValueError):
                B.ais_glms(popn, x, mass=bad, **kw)
    finally:
        popn.release_data()
