"""GPU tests of the lock-step dense Newton sweep (inference/batched_newton.py on the pgl_newton_* row kernels and
pgl_chol_solve_dev): every row kernel launch of whole fits against the host mirror (tests/newton_mirror.py) on the same state
and inputs, whole fits against an independent evaluation of the log posterior, row independence, keyword handling.
N = 2 and 3, 4 000 bins, exp and explinear, with and without a basis stimulus, Gaussian impulse priors and one group lasso.

Launch by launch: before a launch the mirror takes the device's state (Mirror.load_block) and the launch's device inputs
(ll and gradient, the factor's flag and the solve's output), makes the same step on the host, and the state read back
after the launch is compared: counters, flags, status and phase exactly, everything else to 1e-10 of its scale (a vector:
the largest entry of the row, for a gradient the largest term it is the difference of; a value of the objective: |f|; a
derivative along the direction: |phi'(0)| or the terms of g . p; a step length: max(1, step)) -- the bound tests/test_newton_cg_host.py holds the Newton-CG core to against its reference, for the same reason
(the same float64 steps with sums in another order; tests/test_gpu_newton_cg.py itself has no launch-by-launch
comparison to take a bound from)."""
import copy

import numpy as np
import pytest

from tests import newton_mirror as NM

pytestmark = pytest.mark.gpu

TOL = 1e-10
GTOL = 1e-6
EXACT = ('nit', 'nfev', 'nhess', 'nfact', 'status', 'phase')
# the fields of PglLs (csrc/pglm_linesearch.h), in the order of the state's (18, M) block
LS = dict((n, i) for i, n in enumerate(('stp', 'finit', 'ginit', 'gtest', 'stx', 'fx', 'gx', 'sty', 'fy', 'gy', 'stmin', 'stmax',
                                        'width', 'width1', 'brackt', 'stage', 'nfev', 'moved')))
CASES = {'n2_exp': (2, 'exp', False, 'gaussian'), 'n3_explinear_stim': (3, 'explinear', True, 'gaussian'),
         'n3_exp_stim': (3, 'exp', True, 'gaussian'), 'n2_explinear': (2, 'explinear', False, 'gaussian'),
         'n3_exp_lasso': (3, 'exp', False, 'group_lasso')}


def _population(N, nlin, basis_stim, prior, seed=211):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    if basis_stim:
        model['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': model['bkgd']['basis']}
    model['nonlinearity']['type'] = nlin
    model['bias']['mu'] = 3.0 if nlin == 'exp' else model['bias']['mu']
    if prior == 'gaussian':
        model['impulse'] = dict(model['impulse'], prior={'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0})
    popn = Population(model)
    T = 4.0
    rng = np.random.default_rng(seed)
    S = np.minimum(rng.poisson(20.0 * 0.001, size=(4000, N)), 10).astype(np.uint8)
    data = {'S': S, 'N': N, 'dt': 0.001, 'T': T, 'stim': None, 'dt_stim': 0.1}
    if basis_stim:
        data['stim'] = rng.standard_normal((40, 2))
    popn.add_data(data)
    return popn


_POPS = {}


@pytest.fixture(scope='module')
def pops():
    def get(name):
        if name not in _POPS:
            popn = _population(*CASES[name])
            _POPS[name] = (popn, popn.sample(np.random.RandomState(97)))
        return _POPS[name]
    yield get
    for popn, _ in _POPS.values():
        popn.release_data()
    _POPS.clear()


def _compare(st_dev, mirror, M, P, what):
    got, want = NM.split_block(st_dev, M, P), NM.split_block(mirror.block(), M, P)
    for k, name in enumerate(NM.FIELDS):
        if name in EXACT:
            assert np.array_equal(got['sc'][k], want['sc'][k]), (what, name, got['sc'][k], want['sc'][k])
    worst = 0.0
    # A gradient is the difference of the likelihood's gradient and the prior's; at a stationary point the two cancel, so its
    # rounding error is relative to the terms, not to their difference: the scale of g and gb is the larger of max|g| and
    # the largest entry of the prior's gradient at the row's point.
    with np.errstate(invalid='ignore', divide='ignore'):
        gp = NM.objective(want['X'], np.zeros(M), np.zeros((M, P)), mirror.prior, *mirror.NBD)[1]
    gscale = np.maximum(np.max(np.abs(want['g']), axis=1), np.nanmax(np.abs(gp), axis=1))
    for name in NM.VECS:                                       # vectors: relative to the largest entry of the row
        a, b = got[name], want[name]
        scale = np.max(np.abs(b), axis=1, keepdims=True)
        if name in ('g', 'gb'):
            scale = np.maximum(scale, gscale[:, None])
        err = np.abs(a - b) / np.where(scale > 0, scale, 1.0)
        worst = max(worst, float(np.max(err)))
        assert np.max(err) <= TOL, (what, name, float(np.max(err)))
    # scalars, row by row: values of the objective relative to |f|, derivatives along the direction relative to |phi'(0)| or
    # to the terms of the dot product g . p (the scale of g times |p|_1) where that is larger, step lengths relative to
    # max(1, step); flags and counters of the search exactly
    sc, ls = want['sc'], want['ls']
    fscale = np.maximum(np.abs(sc[NM.SC['f']]), 1.0)
    dscale = np.maximum(np.abs(ls[LS['ginit']]), np.abs(sc[NM.SC['slope']]))
    dscale = np.maximum(dscale, gscale * np.sum(np.abs(want['p']), axis=1))
    dscale = np.where(dscale > 0, dscale, 1.0)
    groups = [('sc', [NM.SC['f'], NM.SC['fprev']], fscale), ('ls', [LS[k] for k in ('finit', 'fx', 'fy')], fscale),
              ('sc', [NM.SC['slope']], dscale), ('ls', [LS[k] for k in ('ginit', 'gtest', 'gx', 'gy')], dscale),
              ('sc', [NM.SC['alpha'], NM.SC['shift']], None),
              ('ls', [LS[k] for k in ('stp', 'stx', 'sty', 'stmin', 'stmax', 'width', 'width1')], None)]
    for blk, ks, scale in groups:
        for k in ks:
            a, b = got[blk][k], want[blk][k]
            s = np.maximum(1.0, np.abs(b)) if scale is None else scale
            err = np.abs(a - b) / s
            worst = max(worst, float(np.max(err)))
            assert np.max(err) <= TOL, (what, blk, k, a, b)
    for k in ('brackt', 'stage', 'nfev', 'moved'):
        assert np.array_equal(got['ls'][LS[k]], want['ls'][LS[k]]), (what, k)
    return worst


@pytest.mark.parametrize('name', ['n2_exp', 'n3_explinear_stim', 'n3_exp_lasso'])
def test_every_launch_against_the_host_mirror(pops, name):
    """A whole fit, driven here launch by launch: init, then per outer iteration trial (the points of the Hessian list),
    assemble (against newton_mirror.assemble on the device's Hessian), factor and solve, direction, and trial /
    search_step until no row searches."""
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import _Packing
    from theano_pyglm_amd.inference.lockstep import session
    popn, x0 = pops(name)
    M = popn.N
    with session(popn) as (torch_, dev, stream, handles):
        h = handles[0]
        pk = _Packing(popn, torch, handles, (0, M))
        P, prm = pk.Pp, pk.prior_params()
        N, B, D = popn.N, popn.glm.imp_model.B, P - 1 - popn.N * popn.glm.imp_model.B
        f64 = torch.float64
        st = torch.zeros(h.newton_state_doubles(M, P), dtype=f64, device=dev)
        X0 = pk.pack(x0, 0, M)
        st[:M * P].copy_(torch.tensor(X0, dtype=f64, device=dev).view(-1))
        Weff = torch.tensor(popn.W_eff(x0), dtype=f64, device=dev)
        mir = NM.Mirror(None, None, X0, N, B, D, prm, gtol=GTOL, maxiter=30)
        buf = torch.empty(M * (1 + P), dtype=f64, device=dev)
        Xt = [torch.empty((M, P), dtype=f64, device=dev) for _ in range(2)]
        Hd = torch.empty((M, P, P + 1), dtype=f64, device=dev)
        rows_d = torch.empty(M, dtype=torch.int32, device=dev)
        idx_d = torch.empty(M, dtype=torch.int32, device=dev)

        def state():
            stream.synchronize()
            return st.cpu().numpy()

        def lists(rows):
            rows_d[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int32))
            idx_d[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int32))

        # init
        h.ll_grad_dev(st.data_ptr(), Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), 0, M)
        stream.synchronize()
        ll, gr = buf[:M].cpu().numpy(), buf[M:].view(M, P).cpu().numpy()
        h.newton_init_dev(st.data_ptr(), M, P, buf.data_ptr(), buf[M:].data_ptr(), prm, GTOL, 30)
        mir.init(ll, gr)
        worst = {'init': _compare(state(), mir, M, P, 'init')}
        outer = 0
        while np.any(mir.field('phase') != NM.PHASE_DONE):
            outer += 1
            assert outer <= 31
            mir.load_block(state())
            rows = [int(r) for r in mir.rows_in(NM.PHASE_HESS)]
            L = len(rows)
            lists(rows)
            h.newton_trial_dev(st.data_ptr(), M, P, rows_d.data_ptr(), L, Xt[0].data_ptr())
            stream.synchronize()
            assert np.array_equal(Xt[0][:L].cpu().numpy(), mir.vec[rows, 0])           # phase 0: the points themselves
            h.hvp_prepare(Xt[0].data_ptr(), Weff.data_ptr(), d_idx=idx_d.data_ptr(), count=L)
            h.hess(Hd.data_ptr(), P + 1)
            stream.synchronize()
            Hraw = Hd[:L].clone()
            todo = list(range(L))                              # positions in Hraw
            while todo:
                cur = [rows[j] for j in todo]
                lists(cur)
                A = Hraw[todo].clone()
                Hll = A.cpu().numpy()[:, :, :P]
                rhs = torch.empty((len(cur), P), dtype=f64, device=dev)
                mir.load_block(state())
                h.newton_assemble_dev(st.data_ptr(), M, P, rows_d.data_ptr(), len(cur), A.data_ptr(), P + 1, prm, rhs.data_ptr())
                stream.synchronize()
                Ah = A.cpu().numpy()
                il = np.tril_indices(P)
                for j, r in enumerate(cur):
                    want = mir.assembled(r, Hll[j])
                    scale = np.sqrt(np.abs(np.outer(np.diag(want), np.diag(want))))
                    assert np.max(np.abs(Ah[j][:, :P][il] - want[il]) / scale[il]) <= TOL, ('assemble', r)
                    assert np.array_equal(Ah[j][:, :P][np.triu_indices(P, 1)], Hll[j][np.triu_indices(P, 1)])
                    assert np.array_equal(rhs[j].cpu().numpy(), -mir.vec[r, 1])
                scale_d, _, info = h.chol_factor(A)
                h.chol_solve(A, scale_d, info, rhs, out=rhs)
                stream.synchronize()
                info_h, sol = info.cpu().numpy(), rhs.cpu().numpy()
                h.newton_direction_dev(st.data_ptr(), M, P, rows_d.data_ptr(), len(cur), info.data_ptr(), rhs.data_ptr())
                for j, r in enumerate(cur):
                    mir.direction(r, info_h[j], sol[j])
                worst['direction'] = max(worst.get('direction', 0.0), _compare(state(), mir, M, P, 'direction %d' % outer))
                todo = [j for j in todo if mir.field('phase')[rows[j]] == NM.PHASE_REFACTOR]
            rows = [int(r) for r in mir.rows_in(NM.PHASE_SEARCH)]
            k = 0
            while rows:
                L = len(rows)
                lists(rows)
                cur, nxt = Xt[k & 1], Xt[(k + 1) & 1]
                h.newton_trial_dev(st.data_ptr(), M, P, rows_d.data_ptr(), L, cur.data_ptr())
                stream.synchronize()
                xt = cur[:L].cpu().numpy()
                for j, r in enumerate(rows):
                    want = mir.vec[r, 0] + mir.field('alpha')[r] * mir.vec[r, 2]
                    assert np.max(np.abs(xt[j] - want)) <= TOL * np.max(np.abs(want)), ('trial', r)
                b = buf[:L * (1 + P)]
                h.ll_grad_list_dev(idx_d.data_ptr(), L, cur.data_ptr(), Weff.data_ptr(), b.data_ptr(), b[L:].data_ptr())
                stream.synchronize()
                ll, gr = b[:L].cpu().numpy(), b[L:].view(L, P).cpu().numpy()
                mir.load_block(state())
                h.newton_search_step_dev(st.data_ptr(), M, P, rows_d.data_ptr(), L, cur.data_ptr(), b.data_ptr(), b[L:].data_ptr(),
                                         prm, GTOL, 30, 0, nxt.data_ptr())
                for j, r in enumerate(rows):
                    mir.feed(r, ll[j], gr[j], xt=xt[j])
                worst['search_step'] = max(worst.get('search_step', 0.0), _compare(state(), mir, M, P, 'search %d.%d' % (outer, k)))
                stream.synchronize()
                xn = nxt[:L].cpu().numpy()
                for j, r in enumerate(rows):                   # the next trial point of a row that goes on searching
                    if mir.field('phase')[r] == NM.PHASE_SEARCH:
                        assert np.max(np.abs(xn[j] - mir.vec[r, 5])) <= TOL * np.max(np.abs(mir.vec[r, 5])), ('Xt_next', r)
                rows = [r for r in rows if mir.field('phase')[r] == NM.PHASE_SEARCH]
                k += 1
        print("%s: %d outer iterations, worst relative differences %s, status %s, nit %s, shifts %s"
              % (name, outer, worst, mir.field('status'), mir.field('nit'), [len(s) for s in mir.shifts]))
        assert np.all(mir.field('status') == 0)
        assert set(worst) == {'init', 'direction', 'search_step'}


@pytest.mark.parametrize('name', sorted(CASES))
def test_whole_fit_converges_to_a_stationary_point(pops, name):
    from theano_pyglm_amd.inference import batched_newton as BN
    popn, x0 = pops(name)
    x = copy.deepcopy(x0)
    fun, nit, nfev, nhess, status = BN.fit_glms_newton_torch(popn, x, gtol=GTOL)
    stats = popn.last_fit_stats
    lp, g = popn.compute_lp_grad_packed(x)
    print("%s: nit %s nfev %s nhess %s status %s, max|g| %.3e, fun + lp %s, launches %s"
          % (name, nit, nfev, nhess, status, np.max(np.abs(g)), fun + lp, dict((k, v) for k, v in stats.items() if k != 'per_neuron')))
    assert np.all(status == 0)
    assert np.max(np.abs(g)) <= GTOL
    assert np.all(np.abs(fun + lp) <= 1e-10 * np.abs(lp))
    assert np.all(nit >= 1) and np.all(nhess == nit)
    assert stats['hess_launches'] == nit.max() and stats['hess_rows'] == nit.sum()      # a converged row costs no Hessian
    assert stats['factor_rows'] == sum(stats['per_neuron']['nfact'])


def test_rows_are_independent_and_a_converged_row_is_never_written(pops):
    from theano_pyglm_amd.inference import batched_newton as BN
    popn, x0 = pops('n3_exp_stim')
    xa = copy.deepcopy(x0)
    fa = BN.fit_glms_newton_torch(popn, xa, gtol=GTOL)
    xb = copy.deepcopy(x0)
    fb = BN.fit_glms_newton_torch(popn, xb, gtol=GTOL, n_lo=1, n_hi=3)
    for a, b in zip(fa, fb):
        assert np.array_equal(a[1:3], b)
    from theano_pyglm_amd.utils.packvec import packdict
    for n in (1, 2):
        assert np.array_equal(packdict(xa['glms'][n]['imp'])[0], packdict(xb['glms'][n]['imp'])[0])
        assert np.array_equal(xa['glms'][n]['bias']['bias'], xb['glms'][n]['bias']['bias'])
    assert np.array_equal(packdict(xb['glms'][0]['imp'])[0], packdict(x0['glms'][0]['imp'])[0])
    # row 1 starts at its optimum: it ends in init and its row of X keeps its bits while the others run
    xs = copy.deepcopy(x0)
    xs['glms'][1] = copy.deepcopy(xa['glms'][1])
    trace = []
    fun, nit, nfev, nhess, status = BN.fit_glms_newton_torch(popn, xs, gtol=GTOL, on_outer=lambda k, info: trace.append(info))
    assert np.all(status == 0) and nit[1] == 0 and nhess[1] == 0 and nfev[1] == 1
    assert len(trace) >= 2 and all(np.array_equal(t['X'][1], trace[0]['X'][1]) for t in trace)
    assert popn.last_fit_stats['hess_rows'] == nit.sum()
    for r in (0, 2):                                           # frozen from the iteration in which the row finished
        first = next(k for k, t in enumerate(trace) if t['status'][r] >= 0)
        assert all(np.array_equal(t['X'][r], trace[first]['X'][r]) for t in trace[first:])
    # maxiter = 0: status 1 everywhere, nothing moves
    x1 = copy.deepcopy(x0)
    out = BN.fit_glms_newton_torch(popn, x1, maxiter=0)
    assert np.all(out[4] == 1) and np.all(out[1] == 0)
    assert np.array_equal(packdict(x1['glms'][0]['imp'])[0], packdict(x0['glms'][0]['imp'])[0])


def test_slices_give_the_bits_of_one_list(pops):
    """A Hessian budget that holds one row per slice: the same fit, bit for bit."""
    from theano_pyglm_amd.inference import batched_newton as BN
    popn, x0 = pops('n3_exp_stim')
    xa, xb = copy.deepcopy(x0), copy.deepcopy(x0)
    fa = BN.fit_glms_newton_torch(popn, xa, gtol=GTOL)
    fb = BN.fit_glms_newton_torch(popn, xb, gtol=GTOL, hess_budget_bytes=1)
    assert popn.last_fit_stats['rows_per_slice'] == 1
    for a, b in zip(fa, fb):
        assert np.array_equal(a, b)


def test_coord_descent_newton_and_its_keywords(pops):
    from theano_pyglm_amd.inference import coord_descent as cd
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn, x0 = pops('n2_exp')
    for kw in ({'use_rop': True}, {'prox': True}):
        with pytest.raises(ValueError, match="newton=True"):
            cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, newton=True, **kw)
    x = cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, newton=True)
    assert popn.last_fit_stats['optimizer'].startswith('lock-step dense Newton')
    assert all(s == 0 for s in popn.last_fit_stats['per_neuron']['status'])
    _, g = popn.compute_lp_grad_packed(x)
    assert np.max(np.abs(g)) <= 1e-5                           # (the sweep's default gtol)
    popn.set_time_shard(0, 2)
    try:
        with pytest.raises(ValueError, match="time-sharded"):
            cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, newton=True)
    finally:
        popn.set_time_shard(None)
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):
        p2 = Population(make_model(name, N=2, dt=0.001))
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            cd.coord_descent(p2, p2.sample(np.random.RandomState(1)), maxiter=1, newton=True)
