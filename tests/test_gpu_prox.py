"""GPU tests of the lock-step proximal-gradient fit (pgl_prox_* row kernels, inference/batched_prox.py): the device fit through
the C ABI against the host mirror of the same state machine (tests/prox_mirror.py: csrc/pglm_prox.h built by gcc) fed by the
oracle's ll and gradient, and the driver's contract (KKT at the answer, launch counts, unsupported inputs, the path).

Every decision of the machine is a discontinuity, and the machine records the smallest margin of each kind it has taken
(sufficient decrease, restart, a group against its threshold, the KKT residual against gtol).  The cases run a fixed 12
iterations from a start far from the optimum -- not to convergence, where the sufficient-decrease gap shrinks into rounding --
and are seeded so that in the mirror every margin stays above 1e-7 (asserted), a thousand times the 1e-10 ll parity bound:
no decision can flip, and the rows agree to rounding."""
import copy
import os
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import prox_mirror as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-7
ITERS = 12
GTOL = 1e-5
MU, SIGMA = 0.1, 2.0
PROX_KERNELS = ['k_prox_init', 'k_prox_step']
FRACS = (0.0, 1.5, 0.3, 0.6, 0.15, 0.9, 0.45)                  # lam of row i = FRACS[i] * its lam_max: one at 0, one above

# (N, B, Ds, n_lo, n_hi, nT); per nonlinearity the problem's seed (SEEDS below): seeded on the CPU so that the mirror alone
# keeps every margin above 1e-7.
SHAPES = {
    'N1': (1, 5, 0, 0, 1, 2000),
    'N3_stim': (3, 5, 2, 0, 3, 3000),
    'N7_B3': (7, 3, 0, 0, 7, 2000),
    'N70_rows64': (70, 4, 0, 64, 70, 2000),                    # P = 281: more than one pass of the 256 threads
    'N6_one_row': (6, 5, 1, 4, 5, 5000),
}
SEEDS = {}


def _prior(kind):
    return (3.0 if kind == 'exp' else 20.0, 1.0, 1.0, MU, SIGMA)


def _problem(shape, kind, seed):
    N, B, Ds, n_lo, n_hi, nT = SHAPES[shape]
    kw = dict(bias_mu=3.0, w_scale=0.05) if kind == 'exp' else {}
    return H.Problem(N, nT, H.std_ibasis()[:, :B], kind=kind, seed=seed, Dstim=Ds, **kw)


def mirror_fit(shape, kind, seed, iters=ITERS):
    """The mirror on the oracle for `iters` iterations.  -> (problem, X0, lam, mirror, calls of the machine)."""
    N, B, Ds, n_lo, n_hi, nT = SHAPES[shape]
    p = _problem(shape, kind, seed)
    prior = _prior(kind)
    tg = PM.oracle_target([p], n_lo, n_hi)
    X0 = p.theta[n_lo:n_hi].copy()
    null = PM.Mirror(tg, X0, N, B, Ds, prior, np.inf, gtol=GTOL).run()
    gw = null.gx[:, 1 + Ds:].reshape(n_hi - n_lo, N, B)
    lam_max = SIGMA * np.max(np.sqrt(np.sum(gw * gw, axis=2)), axis=1)
    M = n_hi - n_lo
    lam = lam_max * (np.array(FRACS[:M]) if M > 1 else 0.3)
    m = PM.Mirror(tg, X0, N, B, Ds, prior, lam, gtol=GTOL, maxiter=iters)
    calls = 0
    while not m.done():
        m.step()
        calls += 1
    return p, X0, lam, m, calls


def device_fit(p, X0, n_lo, n_hi, prior, lam, maxiter, calls, max_backtrack=40, gtol=GTOL):
    """The same fit through the C ABI: init and `calls` calls of the machine.  -> (state block, Xt), host copies."""
    import torch
    M, P = X0.shape
    dev = torch.device('cuda', 0)
    f64 = torch.float64
    h = p.device(0)
    stream = torch.cuda.Stream(dev)
    try:
        h.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            st = torch.zeros(h.prox_state_doubles(M, P), dtype=f64, device=dev)
            assert st.numel() == 5 * M * P + len(PM.FIELDS) * M
            st[:M * P].view(M, P).copy_(torch.tensor(X0, dtype=f64, device=dev))
            Weff = torch.tensor(p.Weff, dtype=f64, device=dev)
            d_lam = torch.tensor(lam, dtype=f64, device=dev)
            Xt = torch.zeros((M, P), dtype=f64, device=dev)
            buf = torch.empty(M * (1 + P), dtype=f64, device=dev)
            flags = torch.zeros(M, dtype=f64).pin_memory()

            def evaluate(Xe):
                h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), n_lo, n_hi)
                return buf[:M], buf[M:]

            ll, g = evaluate(st[:M * P].view(M, P))
            h.prox_init_dev(st.data_ptr(), M, P, ll.data_ptr(), g.data_ptr(), prior, d_lam.data_ptr(), gtol, maxiter,
                            Xt.data_ptr(), flags.data_ptr())
            for _ in range(calls):
                ll, g = evaluate(Xt)
                h.prox_step_dev(st.data_ptr(), M, P, ll.data_ptr(), g.data_ptr(), prior, d_lam.data_ptr(), gtol, maxiter,
                                max_backtrack, Xt.data_ptr(), flags.data_ptr())
            stream.synchronize()
            sth = st.cpu().numpy()
            assert np.array_equal(flags.numpy(), sth[5 * M * P:].reshape(-1, M)[PM.SC['phase']])
            return sth, Xt.cpu().numpy()
    finally:
        h.close()


def _views(st, M, P):
    return st[:M * P].reshape(M, P), st[5 * M * P:].reshape(len(PM.FIELDS), M)


COUNTERS = ('iters', 'nfev', 'nbt', 'restarts', 'phase', 'status', 'y_is_x')

# (seed, iterations) and the mirror's smallest margins (m_sd, m_restart, m_zero, m_kkt) as observed on the CPU
SEEDS.update({
    ('N1', 'explinear'): (1, ITERS),                            # 1.2e-4, 7.3e-4, 9.7e-1, 9.3e+3
    ('N1', 'exp'): (1, ITERS),                                  # 8.4e-5, 1.0e-3, 7.7e-1, 4.6e+4
    ('N3_stim', 'explinear'): (1, ITERS),                       # 5.3e-6, 7.7e-7, 1.9e-3, 2.2e+2
    # seeds 1 .. 7 at 12 iterations: the row above its lam_max is all but converged and m_sd falls to 1e-12; shortened to 8
    # (a backtrack and a restart are among its decisions)
    ('N3_stim', 'exp'): (1, 8),                                 # 3.2e-7, 2.1e-5, 5.8e-3, 2.3e+3
    ('N7_B3', 'explinear'): (1, ITERS),                         # 1.2e-4, 9.3e-4, 7.9e-2, 5.6e+3
    ('N7_B3', 'exp'): (1, ITERS),                               # 8.2e-6, 9.5e-7, 3.3e-3, 1.9e+4
    ('N70_rows64', 'explinear'): (1, ITERS),                    # 1.4e-3, 3.6e-3, 1.4e-3, 1.2e+4
    ('N70_rows64', 'exp'): (3, ITERS),                          # 1.2e-4, 4.1e-5, 1.0e-3, 4.2e+4   (seeds 1, 2: m_sd below 1e-9)
    ('N6_one_row', 'explinear'): (1, ITERS),                    # 1.2e-4, 1.2e-3, 9.5e-1, 1.2e+4
    ('N6_one_row', 'exp'): (1, ITERS),                          # 8.8e-5, 8.6e-4, 6.6e-1, 1.6e+5
})


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['explinear', 'exp'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_device_fit_equals_host_mirror(shape, kind):
    N, B, Ds, n_lo, n_hi, nT = SHAPES[shape]
    seed, iters = SEEDS[(shape, kind)]
    p, X0, lam, m, calls = mirror_fit(shape, kind, seed, iters)
    M, P = X0.shape
    margins = [m.field(k).min() for k in PM.MARGINS]
    print("%s/%s mirror: %d calls, iters %s, restarts %s, smallest margins %s" % (shape, kind, calls, m.field('iters'),
                                                                                 m.field('restarts'), margins))
    assert min(margins) > MARGIN                                # the condition the case was seeded for
    assert np.all(m.field('iters') == iters) and np.all(m.field('status') == 1)
    st, Xt = device_fit(p, X0, n_lo, n_hi, _prior(kind), lam, iters, calls)
    Xd, scd = _views(st, M, P)
    for k in COUNTERS:
        assert np.array_equal(scd[PM.SC[k]], m.field(k)), k
    assert np.array_equal(Xd == MU, m.x == MU)                  # the same entries are exactly mu
    assert np.array_equal(Xt, Xd)                               # an ended row keeps x in its row of Xt
    err = np.max(np.abs(Xd - m.x) / np.max(np.abs(m.x), axis=1, keepdims=True))
    print("%s/%s device against mirror: largest error relative to the row's largest entry %.3e" % (shape, kind, err))
    assert err <= 1e-9
    assert np.allclose(scd[PM.SC['t']], m.field('t'), rtol=1e-9, atol=0.0)
    assert np.allclose(scd[PM.SC['F_x']], m.field('F_x'), rtol=1e-9, atol=0.0)
    if M > 1:
        sup = m.support()
        assert sup[0].all() and sup[1].sum() < sup[0].sum()     # lam = 0: dense; above lam_max: groups are going


@pytest.mark.gpu
def test_runs_repeat_and_row_range_equals_full_run():
    p = _problem('N7_B3', 'explinear', 3)
    prior = _prior('explinear')
    lam = np.array([0.0, 9.0, 0.2, 0.4, 0.1, 0.6, 0.3])
    full, xt = device_fit(p, p.theta.copy(), 0, 7, prior, lam, 8, 30)
    again, xt2 = device_fit(p, p.theta.copy(), 0, 7, prior, lam, 8, 30)
    assert np.array_equal(full, again) and np.array_equal(xt, xt2)
    sub, xts = device_fit(p, p.theta[2:5].copy(), 2, 5, prior, lam[2:5], 8, 30)
    Xf, scf = _views(full, 7, p.P)
    Xs, scs = _views(sub, 3, p.P)
    assert np.array_equal(Xs, Xf[2:5]) and np.array_equal(scs, scf[:, 2:5]) and np.array_equal(xts, xt[2:5])
    assert np.all(scf[PM.SC['iters']] >= 5) and np.any(scf[PM.SC['phase']] == PM.PHASE_DONE) and np.all(Xf != p.theta)


# ---- the driver --------------------------------------------------------------------------------------------------
def _population(N=4, T=4.0, seed=89):
    from tests.test_gpu_hvp import _std_population
    popn = _std_population(N, T, seed, nlin='exp', bias_mu=3.0)
    return popn


def _oracle_kkt(popn, x, lam):
    """The KKT residual of every neuron at x, recomputed in numpy from the oracle's gradient."""
    from oracle import c_oracle as CO
    glm = popn.glm
    data = popn.data_sequences[0]
    S = np.asarray(data['S']).astype(np.uint8)
    ib = np.ascontiguousarray(glm.imp_model.ibasis)
    N, B = popn.N, ib.shape[1]
    X = popn.theta_matrix(x)
    fS = CO.features(S, ib)

    def tg(Xe):
        return CO.ll_grad(S, fS, Xe, popn.W_eff(x), glm.nlin_model.kind, glm.dt)
    pr = glm.imp_model.prior
    prior = (float(glm.bias_model.mu_bias), float(glm.bias_model.sig_bias), 1.0, float(pr.mu), float(pr.sigma))
    f, G = PM.smooth_f_grad(tg, X, 0, prior)
    return PM.kkt_residual(X, G, N, B, 0, prior, lam), f + PM.h_value(X, N, B, 0, prior, lam)


@pytest.mark.gpu
def test_driver_reaches_kkt_and_counts_launches():
    from theano_pyglm_amd.inference import batched_prox as BP
    popn = _population()
    try:
        assert BP.supported(popn)
        x = popn.sample(np.random.RandomState(97))
        lmax = BP.lasso_lam_max(popn, x)
        assert lmax.shape == (4,) and np.all(lmax > 0.0)
        lam = 0.4 * lmax
        x0 = copy.deepcopy(x)
        res = BP.fit_glms_prox(popn, x, lam=lam, gtol=GTOL)
        st = popn.last_fit_stats
        print(res, st)
        assert np.all(res['status'] == 0) and np.all(res['kkt'] <= GTOL)
        r, F = _oracle_kkt(popn, x, lam)
        print("oracle KKT", r)
        assert np.all(r <= GTOL)
        assert np.allclose(F, res['objective'], rtol=1e-9, atol=0.0)
        assert np.array_equal(res['support'], np.any(popn.theta_matrix(x)[:, 1:].reshape(4, 4, -1) != 0.0, axis=2))
        assert res['support'].any() and not res['support'].all()
        # one row launch per evaluation, init included; the rows' own counts never exceed the launches
        assert st['row_launches'] == st['ll_grad_launches'] and np.all(res['nfev'] <= st['ll_grad_launches'])
        assert st['ll_grad_launches'] <= np.max(res['nfev']) + 2 * BP.POLL and st['flag_polls'] >= 1
        # rows that end in init cost one evaluation and one row launch: the flags are read behind init before anything else
        xz = copy.deepcopy(x0)
        rz = BP.fit_glms_prox(popn, xz, lam=lam, maxiter=0)
        assert np.all(rz['status'] == 1) and np.all(rz['iters'] == 0) and np.all(rz['nfev'] == 1)
        assert popn.last_fit_stats['ll_grad_launches'] == 1 and popn.last_fit_stats['row_launches'] == 1
        assert np.array_equal(popn.theta_matrix(xz), popn.theta_matrix(x0))
        # the prior's own lam; a range of neurons equals the matching rows
        xa, xb = copy.deepcopy(x0), copy.deepcopy(x0)
        ra = BP.fit_glms_prox(popn, xa, maxiter=15)
        rb = BP.fit_glms_prox(popn, xb, maxiter=15, n_lo=1, n_hi=3)
        assert np.all(ra['lam'] == popn.glm.imp_model.prior.lam)
        assert np.array_equal(popn.theta_matrix(xb)[1:3], popn.theta_matrix(xa)[1:3])
        assert np.array_equal(popn.theta_matrix(xb)[0], popn.theta_matrix(x0)[0])
        assert np.array_equal(rb['objective'], ra['objective'][1:3])
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_lasso_path():
    from theano_pyglm_amd.inference import batched_prox as BP
    from theano_pyglm_amd.utils.io import segment_data
    popn = _population(T=5.0)
    try:
        data = popn.data_sequences[0]
        held = popn.preprocess_data(segment_data(data, (3.75, 5.0)))
        x0 = popn.sample(np.random.RandomState(97))
        lmax = BP.lasso_lam_max(popn, x0)
        lams = lmax[None, :] * np.array([1.05, 0.5, 0.2])[:, None]      # per neuron: every first point is above lam_max
        x_before = copy.deepcopy(x0)
        out = BP.lasso_path(popn, x0, lams=lams, heldout=held, gtol=GTOL)
        assert np.array_equal(popn.theta_matrix(x0), popn.theta_matrix(x_before))
        P = popn.glm.P
        assert out['X'].shape == (3, 4, P) and out['support'].shape == (3, 4, 4) and out['heldout_ll'].shape == (3, 4)
        assert np.all(out['status'] == 0)
        assert not out['support'][0].any() and out['support'][2].any()
        assert np.all(out['support'].sum(axis=2)[1:] >= out['support'].sum(axis=2)[:-1])
        popn.set_data(held)
        for l in range(3):
            xx = copy.deepcopy(x0)
            BP._Packing(popn, None).unpack(xx, out['X'][l], 0, 4)
            assert np.array_equal(popn.compute_ll_vector(xx), out['heldout_ll'][l])
        assert np.array_equal(out['best'], np.argmax(out['heldout_ll'], axis=0))
        assert np.array_equal(popn.theta_matrix(out['x_best']), out['X'][out['best'], np.arange(4)])
        # the default grid: geometric, descending, from the median lam_max
        d = BP.lasso_path(popn, x0, n_lams=3, lam_ratio=0.1, maxiter=60)
        top = np.median(BP.lasso_lam_max(popn, x0, maxiter=60))       # (the fit options reach the null fit too)
        assert np.allclose(d['lams'], top * np.array([1.0, 10 ** -0.5, 0.1]), rtol=1e-12) and abs(top / np.median(lmax) - 1) < 0.05
        with pytest.raises(ValueError, match="descend"):
            BP.lasso_path(popn, x0, lams=[0.1, 0.2])
    finally:
        popn.release_data()


@pytest.mark.gpu
def test_unsupported_inputs_raise():
    from theano_pyglm_amd.inference import batched_prox as BP
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):     # an 'st' stimulus / Dirichlet impulses
        p2 = Population(make_model(name, N=2, dt=0.001))
        assert not BP.supported(p2)
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            BP.fit_glms_prox(p2, p2.sample(np.random.RandomState(1)))
    model = make_model('standard_glm', N=2, dt=0.001)
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    pg = Population(model)
    assert not BP.supported(pg)
    with pytest.raises(ValueError, match="Gaussian"):
        BP.fit_glms_prox(pg, pg.sample(np.random.RandomState(1)))
    popn = _population(N=2, T=2.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                BP.fit_glms_prox(popn, x)
            with pytest.raises(ValueError, match="time-sharded"):
                BP.lasso_path(popn, x)
        finally:
            popn.set_time_shard(None)
        with pytest.raises(ValueError, match="empty"):
            BP.fit_glms_prox(popn, x, n_lo=1, n_hi=1)
        with pytest.raises(ValueError, match="lam"):
            BP.fit_glms_prox(popn, x, lam=[1.0, 2.0, 3.0])
    finally:
        popn.release_data()


def test_prox_kernels_are_built_without_scratch():
    """(No GPU needed: the code object's metadata.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from theano_pyglm_amd import _lib
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_prox'))
    print(built)
    assert sorted(built) == sorted(PROX_KERNELS)
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0, (n, r)
    assert _lib.load().pgl_version() >= 106                  # (105: the version before the proximal-gradient entry points)
    for s in ('pgl_prox_state_doubles', 'pgl_prox_init_dev', 'pgl_prox_step_dev'):
        assert s in _lib.SYMBOLS
