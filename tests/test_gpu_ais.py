"""GPU tests of annealed importance sampling (pgl_ais_* row kernels, inference/batched_ais.py): the device run through the C
ABI against the host mirror of the same state machine (tests/ais_mirror.py: csrc/pglm_ais.h built by gcc) fed by the
oracle's ll and gradient, and the driver's contract (shapes, launch counts, no host synchronisation, unsupported inputs).

A decision log u < H0 - H1 is a discontinuity: the cases are seeded so that in the mirror every decision keeps
|log u - (H0 - H1)| > 1e-4 (asserted), far above the difference between the oracle's and the device's ll, so no decision
can flip and the final points and weights agree to rounding."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import ais_mirror as AM

MARGIN = 1e-4
BETAS = [0.0, 0.01, 0.1, 0.5, 1.0]


def _prior(kind):
    """(kind, mu_b, sg_b, stim_sigma, mu, sigma, lam): tight, so that ll is finite at every prior draw."""
    return (0, 3.0 if kind == 'exp' else 20.0, 0.3, 1.0, 0.0, 0.1, 0.0)


def _problem(N, nT, kind, seed, ibasis=None):
    from tests.test_gpu_hmc import _problem as hmc_problem
    return hmc_problem(N, nT, kind, seed, ibasis)


def oracle_target(probs, n_lo, n_hi):
    def target(X):
        ll, g = 0.0, 0.0
        for p in probs:
            p.theta = p.theta.copy()
            p.theta[n_lo:n_hi] = X
            a, b = p.oracle_ll_grad(n_lo, n_hi)
            ll, g = ll + a, g + b
        return ll, g
    return target


def mirror_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, particle0=0, minv=None):
    p0 = probs[0]
    mir = AM.Mirror(oracle_target(probs, n_lo, n_hi), K, n_hi - n_lo, (p0.N, p0.B, p0.Dstim, prm[1:]), n_lo=n_lo,
                    particle0=particle0, step0=0.1, seed=seed, minv=minv)
    out = mir.run(betas, n_steps, L, adapt=False, step_table=table)
    out['draws'] = mir.draws
    out['ll_seen'] = np.array(mir.ll_seen)
    return out


def device_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, particle0=0, minv=None):
    """The same run through the C ABI (minv (M, P): the neurons' inverse masses, None: 1); the decisions are read after every
    transition (a test's privilege).
    -> dict as the mirror's, plus 'draws' and 'll_draws' (the evaluation at the draws)."""
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
            assert st.numel() == 6 * R * P + 15 * R
            sc = st[6 * R * P:].view(15, R)
            Weff = torch.tensor(p0.Weff, dtype=f64, device=dev)
            tab = torch.tensor(np.asarray(table, dtype=float).reshape(J - 1, M), dtype=f64, device=dev)
            mt = None if minv is None else torch.tensor(np.asarray(minv, dtype=float).reshape(M, P), dtype=f64, device=dev)
            md = 0 if mt is None else mt.data_ptr()
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
            ll_draws = bufs[0][:R].cpu().numpy()
            h0.ais_start_dev(sp, K, M, P, ll, g, prm)
            accepted = []
            for j in range(1, J + 1):
                h0.ais_temper_dev(sp, K, M, P, prm, betas[j], tab[j - 1].data_ptr() if j < J else 0)
                if j == J:
                    break
                for _ in range(n_steps):
                    h0.ais_begin_dev(sp, K, M, P, md, Xt.data_ptr())
                    for i in range(L):
                        ll, g = evaluate()
                        h0.ais_leap_dev(sp, K, M, P, md, ll, g, prm, i == L - 1, False, Xt.data_ptr(), accepts[j - 1].data_ptr(),
                                        steps[j - 1].data_ptr())
                    stream.synchronize()
                    accepted.append(sc[AM.SC['acc']].cpu().numpy() != 0.0)
            stream.synchronize()
            return {'log_weights': sc[AM.SC['logw']].cpu().numpy().reshape(K, M), 'samples': st[:R * P].cpu().numpy().reshape(K, M, P),
                    'accepts': accepts.cpu().numpy(), 'steps': steps.cpu().numpy(),
                    'accepted': np.array(accepted, dtype=bool).reshape(-1, R), 'draws': draws, 'll_draws': ll_draws}
    finally:
        for h in hs:
            h.close()


def compare(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, label="", minv=None):
    m = mirror_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, minv=minv)
    print("%s mirror: accepted %d of %d, smallest margin %.3e" % (label, m['accepted'].sum(), m['accepted'].size, m['margins'].min()))
    assert np.all(np.isfinite(m['ll_seen'][0]))                 # ll is finite at every prior draw
    assert m['margins'].min() > MARGIN                          # the condition the case was seeded for
    assert m['accepted'].any() and not m['accepted'].all()      # both outcomes of the decision
    d = device_run(probs, K, n_lo, n_hi, prm, betas, n_steps, L, table, seed, minv=minv)
    assert np.array_equal(d['accepted'], m['accepted'])
    assert np.array_equal(d['accepts'], m['accepts']) and np.array_equal(d['steps'], m['steps'])
    err = np.max(np.abs(d['samples'] - m['samples']) / np.max(np.abs(m['samples']), axis=2, keepdims=True))
    finite = m['ll_seen'][np.isfinite(m['ll_seen'])]
    scale = max(1.0, np.max(np.abs(finite)))
    werr = np.max(np.abs(d['log_weights'] - m['log_weights']))
    print("%s device against mirror: points %.3e of the row's largest entry, log w %.3e (bound %.3e)" % (label, err, werr, 1e-9 * scale))
    assert err <= 1e-9
    assert werr <= 1e-9 * scale
    return m, d


# (kind) -> (frozen step per temperature, seed): seeded on the CPU for a mix of decisions with margins > 1e-4
CASES = {
    'explinear': ([0.1, 0.05, 0.03], 2),                        # mirror: 84 of 90 accepted, smallest margin 1.9e-2
    'exp': ([0.1, 0.05, 0.03], 2),                              # 84 of 90, 2.1e-2
}


def _table(steps, M):
    return np.repeat(np.asarray(steps, dtype=float)[:, None], M, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
def test_device_run_equals_host_mirror(kind):
    """N = 5, nT = 2 000, K = 3, betas (0, 0.01, 0.1, 0.5, 1), n_steps = 2, n_leapfrog = 3, frozen steps."""
    p = _problem(5, 2000, kind, 31)
    steps, seed = CASES[kind]
    compare([p], 3, 0, 5, _prior(kind), BETAS, 2, 3, _table(steps, 5), seed, label=kind)


@pytest.mark.gpu
def test_strided_row_loops():
    """P = 281 > the 256 threads of a row kernel's workgroup: N = 70, B = 4, nT = 512, K = 2, one transition of 3 steps."""
    p = _problem(70, 512, 'explinear', 37, ibasis=H.std_ibasis()[:, :4])
    assert p.P == 281
    compare([p], 2, 0, 70, _prior('explinear'), [0.0, 0.5, 1.0], 1, 3, _table([0.05], 70), 3, label="N=70")    # mirror: 84 of 140, 1.5e-2


@pytest.mark.gpu
def test_per_neuron_masses_shared_by_the_particles():
    """pgl_ais_begin_dev starts a transition with the chain's k_hmc_begin on the AIS state: K M = 6 rows, scalar stride 6,
    and row r on row r mod M of minv.  K = 3, neurons 1 .. 2 of N = 5 (M = 2), P = 26 (no multiple of 64), an (M, P) minv
    whose two rows differ (one constant, one random in [0.5, 4)): a wrong row of minv or a wrong stride moves the points by
    orders of magnitude more than the bound and changes decisions.  Against the host mirror at the bounds of compare():
    the decisions, accept counts and steps bit for bit, points and weights within 1e-9 -- the mirror is fed by the CPU
    oracle, whose ll and gradient agree with the device's to rounding and not to the bit, so the points cannot."""
    p = _problem(5, 2000, 'explinear', 31)
    assert p.P == 26
    minv = np.stack([np.full(p.P, 0.25), 0.5 + 3.5 * np.random.default_rng(47).random(p.P)])
    compare([p], 3, 1, 3, _prior('explinear'), BETAS, 2, 3, _table([0.12, 0.06, 0.04], 2), 3, label="minv",
            minv=minv)                                          # mirror: 26 of 36 accepted, smallest margin 4.3e-2


@pytest.mark.gpu
def test_subsets_on_the_device():
    p = _problem(5, 2000, 'explinear', 31)
    prm = _prior('explinear')
    steps, seed = CASES['explinear']
    tab = _table(steps, 5)
    full = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed)
    again = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed)
    for key in ('log_weights', 'samples', 'accepted', 'draws'):
        assert np.array_equal(full[key], again[key])
    sub = device_run([p], 3, 1, 4, prm, BETAS, 2, 3, tab[:, 1:4], seed)
    assert np.array_equal(sub['log_weights'], full['log_weights'][:, 1:4])
    assert np.array_equal(sub['samples'], full['samples'][:, 1:4])
    part = device_run([p], 2, 0, 5, prm, BETAS, 2, 3, tab, seed, particle0=1)
    assert np.array_equal(part['log_weights'], full['log_weights'][1:3])
    assert np.array_equal(part['samples'], full['samples'][1:3])
    assert full['accepted'].any() and np.all(np.isfinite(full['log_weights']))


@pytest.mark.gpu
def test_two_data_sequences_sum():
    """Two recordings of the same population: their [ll | grad] blocks are summed before the row kernel sees them."""
    p1 = _problem(5, 2000, 'explinear', 31)
    p2 = _problem(5, 1008, 'explinear', 41)
    p2.theta, p2.Weff = p1.theta, p1.Weff
    compare([p1, p2], 2, 0, 5, _prior('explinear'), [0.0, 0.1, 1.0], 2, 3, _table([0.07], 5), 3, label="two sequences")   # 13 of 20, 8.7e-3


@pytest.mark.gpu
def test_a_row_that_cannot_move():
    """Frozen step 1e3 for neuron 2.  The nonlinearity is exp, as in test_gpu_hmc.test_rejection_is_local: equal BITS of the
    other neurons need an evaluation whose arithmetic for one neuron does not depend on the currents of another, and the
    explinear epilogue of the fused kernels picks its softplus regime per wave, over lanes of several neurons
    (pgl_rate_terms_n) -- measured with explinear on an MI355X: the other neurons' log w moved in the last digits (within
    the ll tolerance), everything else of this test held."""
    p = _problem(5, 2000, 'exp', 31)
    prm = _prior('exp')
    steps, seed = CASES['exp']
    tab = _table(steps, 5)
    ref = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed)
    tab[:, 2] = 1e3
    out = device_run([p], 3, 0, 5, prm, BETAS, 2, 3, tab, seed)
    rows = np.arange(15).reshape(3, 5)
    assert np.all(out['accepts'][:, rows[:, 2]] == 0.0) and not out['accepted'][:, rows[:, 2]].any()
    assert np.array_equal(out['samples'][:, 2], out['draws'].reshape(3, 5, -1)[:, 2])
    dev = p.device(0)
    try:
        for k in range(3):                                      # the ladder telescopes to (1 - 0) ll at the draw
            th = p.theta.copy()
            th[2] = out['draws'].reshape(3, 5, -1)[k, 2]
            ll, _ = dev.ll_grad(th, p.Weff)
            rel = abs(out['log_weights'][k, 2] - ll[2]) / abs(ll[2])
            print(k, out['log_weights'][k, 2], ll[2], rel)
            assert rel <= 1e-12
    finally:
        dev.close()
    others = [0, 1, 3, 4]
    assert np.array_equal(out['log_weights'][:, others], ref['log_weights'][:, others])
    assert np.array_equal(out['samples'][:, others], ref['samples'][:, others])
    assert ref['accepted'][:, rows[:, 2]].any()


# ---- the driver --------------------------------------------------------------------------------------------------
def _population(N=4, T=6.0, seed=89, gaussian=True):
    """test_gpu_hmc._population (a 4-neuron exp standard_glm); its impulse prior is the template's group lasso unless
    gaussian, which puts N(0, 1) in its place -- the form annealed importance sampling serves."""
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    if not gaussian:
        from tests.test_gpu_hmc import _population as hmc_population
        return hmc_population(N, T, seed)
    model = make_model('standard_glm', N=N, dt=0.001)
    model['nonlinearity']['type'] = 'exp'
    model['bias']['mu'] = 3.0
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    popn = Population(model)
    nT = int(round(T / 0.001))
    S = np.minimum(np.random.default_rng(seed).poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': None, 'dt_stim': 0.1})
    return popn


@pytest.mark.gpu
@pytest.mark.parametrize('pilot', [True, False])
def test_driver_shapes_counts_and_evidence(pilot):
    from theano_pyglm_amd.inference import batched_ais as B
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    try:
        x = popn.sample(np.random.RandomState(97))
        x0 = copy.deepcopy(x)
        K, L, n_steps = 3, 2, 2
        betas = [0.0, 0.001, 0.01, 0.1, 0.4, 1.0]
        J = len(betas) - 1
        out = B.ais_glms(popn, x, n_particles=K, betas=betas, n_steps=n_steps, n_leapfrog=L, step_sz=0.05, pilot=pilot,
                         mass='laplace' if pilot else None, seed=5)
        st = popn.last_fit_stats
        print(st)
        P = popn.glm.P
        assert out['log_Z'].shape == out['log_Z_se'].shape == out['ess'].shape == out['log_prior_norm'].shape == (4,)
        assert out['log_weights'].shape == (K, 4) and out['samples'].shape == (K, 4, P)
        assert out['accept_rate'].shape == out['step_sz'].shape == (J - 1, 4) and np.array_equal(out['betas'], betas)
        assert np.all(np.isfinite(out['log_Z'])) and np.all(np.isfinite(out['log_Z_se']))
        assert np.all(out['accept_rate'] >= 0.0) and np.all(out['accept_rate'] <= 1.0)
        assert out['n_evals'] == st['ll_grad_launches'] == (K + int(pilot)) * (1 + (J - 1) * n_steps * L)
        assert st['host_syncs_in_run'] == 0
        if not pilot:
            assert np.array_equal(out['step_sz'], np.full((J - 1, 4), 0.05))
        assert np.array_equal(popn.theta_matrix(x), popn.theta_matrix(x0))
        bias, imp = popn.glm.bias_model, popn.glm.imp_model.prior
        norm = np.log(float(bias.sig_bias)) + (P - 1) * np.log(float(imp.sigma)) + 0.5 * P * np.log(2.0 * np.pi)
        assert np.allclose(out['log_prior_norm'], norm, rtol=1e-14)
        lap = np.array([r['log_evidence'] for r in laplace_glms(popn, x)])
        for n in range(4):                                      # printed, not asserted: x is a prior draw, not a mode
            print("neuron %d: AIS log_Z + log_prior_norm %.3f +- %.3f (ess %.2f), Laplace %.3f"
                  % (n, out['log_Z'][n] + out['log_prior_norm'][n], out['log_Z_se'][n], out['ess'][n], lap[n]))
        # particles 1 .. 2 of the same run, neurons 1 .. 2: the same bits (frozen steps given: no pilot)
        sub = B.ais_glms(popn, x, n_particles=2, betas=betas, n_steps=n_steps, n_leapfrog=L, step_sz=out['step_sz'][:, 1:3],
                         pilot=False, mass=None if not pilot else B._laplace_minv(popn, x, 0, 4, 1e-8)[1:3], seed=5, particle0=1,
                         n_lo=1, n_hi=3)
        assert np.array_equal(sub['log_weights'], out['log_weights'][1:3, 1:3])
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_unsupported_inputs_raise():
    from theano_pyglm_amd._lib import PglError
    from theano_pyglm_amd.inference import batched_ais as B
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):     # an 'st' stimulus / Dirichlet impulses
        p2 = Population(make_model(name, N=2, dt=0.001))
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            B.ais_glms(p2, p2.sample(np.random.RandomState(1)), 2, n_temps=5)
    lasso = _population(N=2, T=2.0, gaussian=False)
    try:
        with pytest.raises(ValueError, match="Gaussian"):
            B.ais_glms(lasso, lasso.sample(np.random.RandomState(97)), 2, n_temps=5)
    finally:
        lasso.release_data()
    popn = _population(N=2, T=2.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                B.ais_glms(popn, x, 2, n_temps=5)
        finally:
            popn.set_time_shard(None)
        with pytest.raises(ValueError, match="empty"):
            B.ais_glms(popn, x, 2, n_temps=5, n_lo=1, n_hi=1)
        for bad in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.6, 0.5, 1.0], [0.0, 0.5, 0.5, 1.0]):
            with pytest.raises(ValueError, match="ladder"):
                B.ais_glms(popn, x, 2, betas=bad)
        # the C ABI refuses the group lasso
        import torch
        popn.set_data(popn.data_sequences[0])
        h = popn._handle(popn.data_sequences[0])
        st = torch.zeros(h.ais_state_doubles(2, popn.glm.P), dtype=torch.float64, device=torch.device('cuda', popn.device))
        with pytest.raises(PglError, match="Gaussian"):
            h.ais_temper_dev(st.data_ptr(), 1, 2, popn.glm.P, (1, 3.0, 1.0, 1.0, 0.0, 1.0, 1.0), 0.5)
    finally:
        popn.release_data()
