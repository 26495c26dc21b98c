"""
Lock-step Newton-CG for all neurons with the optimiser state resident on the GPU.

The second-order counterpart of batched_bfgs.py: the reference's `use_rop` branch (parallel_coord_descent.py:62-63,
119-121; map.py:38-45) fits one neuron at a time with scipy.optimize.minimize(method='Newton-CG', jac=, hessp=);
fit_glm(use_rop=True) is that fit on device Hessian-vector products.  The N per-neuron problems are independent given
the network, and a product for ALL neurons costs what one ll+grad evaluation costs (the contraction is dense in the
post-synaptic dimension), so the sweep runs here as one lock-step optimiser: every CG iteration is ONE
pgl_hvp_apply_dev over all rows of the range, every line-search trial one pgl_ll_grad_list_dev of the rows still
searching, and the algorithm itself -- scipy's Newton-CG, restated in csrc/pglm_ncg.h -- runs as HIP row kernels
(pgl_ncg_*, one workgroup per neuron) on state that never leaves the device.  Only the per-row phase flags cross
PCIe, through pinned memory the row kernels write themselves.  PyTorch is plumbing (device memory, the stream, pinned
flags); no library kernel is on the path, except the sum over the data sequences of a population that has several.

The driver is phase-synchronous.  Per outer iteration, for the rows still running:
    pgl_hvp_prepare_dev at the current points  ->  CG iterations (apply + pgl_ncg_cg_step_dev) until no row's CG runs
    ->  line-search evaluations (ll_grad_list + pgl_ncg_search_step_dev) until no row searches.
A row whose CG has ended waits with a zero product input; a finished row is frozen (its kernels return before they write).
The product still covers finished rows (their input is zero): dropping them from an apply is not done.

Served: the packings whose per-neuron vector is the device's theta row, under the priors the row kernels know --
exactly where Glm.hvp_packing() is None (standard_glm: constant bias, no or basis stimulus, linear-basis impulses under
a Gaussian or group-lasso prior).  Time-sharded populations are not (the driver does not all-reduce).
"""
import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.lockstep import (RangeEvaluator, _check, _host_buffers, search_phase, session,  # noqa: F401
                                                 supported, wait)

PHASE_CG, PHASE_SEARCH, PHASE_DONE = 0.0, 1.0, 2.0
# rows of the scalar block of the state (PglNcg, csrc/pglm_ncg.h)
SC_F, SC_NIT, SC_NHEV, SC_NFEV, SC_STATUS, SC_PHASE = 0, 6, 7, 8, 9, 10


def fit_glms_newton_cg_torch(population, x, maxiter=225, n_lo=0, n_hi=None, verbose=False, on_outer=None):
    """In-place MAP fit of x['glms'][n_lo:n_hi] by lock-step Newton-CG; returns per-row arrays (fun, nit, nfev, nhev,
    status) with scipy's status codes (0 success, 1 maxiter, 2 precision loss, 3 CG failure).

    on_outer: optional callable(k, info) after every outer iteration k = 1, 2, ... with host copies
    info = {'X', 'status', 'nit', 'nhev', 'applies'} (a synchronising copy: for tests and traces).
    population.last_fit_stats records the launch counts."""
    _check(population)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    with session(population) as (torch, dev, stream, handles):
        out = _lockstep(population, torch, dev, stream, handles, x, int(maxiter), n_lo, n_hi, M, verbose, on_outer)
        stream.synchronize()
    return out


def _lockstep(population, torch, dev, stream, handles, x, maxiter, n_lo, n_hi, M, verbose, on_outer):
    from theano_pyglm_amd._lib import PglError
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    st = torch.zeros(h0.ncg_state_doubles(M, P), dtype=f64, device=dev)
    MP = M * P
    X = st[0:MP].view(M, P)
    sc = st[7 * MP:].view(-1, M)
    X.copy_(torch.tensor(pk.pack(x, n_lo, n_hi), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    V = torch.zeros((M, P), dtype=f64, device=dev)            # input of the next product, written by the row kernels
    whole = RangeEvaluator(torch, dev, handles, Weff, M, P, n_lo, n_hi)          # (its buffers serve the lists too)
    hvs = [torch.empty((M, P), dtype=f64, device=dev) for _ in handles]
    Xts = [torch.empty((M, P), dtype=f64, device=dev) for _ in range(2)]
    lists = torch.empty(3 * M, dtype=torch.int32, device=dev)
    flags, stage = _host_buffers(torch, dev.index, M)
    flags.fill_(PHASE_DONE)
    fl = flags.numpy()
    done = torch.cuda.Event()
    counts = {'prepare': 0, 'apply': 0, 'outer': 0, 'cg_lengths': []}

    ll0, g0 = whole(X)
    h0.ncg_init_dev(st.data_ptr(), M, P, ll0.data_ptr(), g0.data_ptr(), prm, maxiter, V.data_ptr(), flags.data_ptr())
    wait(stream, done)
    while np.any(fl != PHASE_DONE):
        counts['outer'] += 1
        # -- CG phase: one prepare at the current points, then one product over all rows per CG iteration
        ncg = 0
        if np.any(fl == PHASE_CG):
            for h in handles:
                h.hvp_prepare(X.data_ptr(), Weff.data_ptr(), n_lo, n_hi)
            counts['prepare'] += 1
            while np.any(fl == PHASE_CG):
                for h, hv in zip(handles, hvs):
                    h.hvp_apply(V.data_ptr(), hv.data_ptr())
                    if hv is not hvs[0]:
                        hvs[0].add_(hv)
                counts['apply'] += 1
                ncg += 1
                if counts['apply'] == 1:
                    try:                                       # (dev / test: only with PGL_OPT_RECORD_KERNELS on the handle)
                        counts['apply_kernels'] = h0.last_kernels()
                    except PglError:
                        counts['apply_kernels'] = None
                h0.ncg_cg_step_dev(st.data_ptr(), M, P, hvs[0].data_ptr(), prm, V.data_ptr(), flags.data_ptr())
                wait(stream, done)
        counts['cg_lengths'].append(ncg)
        # -- line-search phase: the rows still searching, one evaluation per trial step
        launch = search_phase(
            fl, PHASE_SEARCH, M, n_lo, stage, lists, Xts, whole.eval_list,
            lambda L, cur: h0.ncg_trial_dev(st.data_ptr(), M, P, lists.data_ptr(), L, cur.data_ptr()),
            lambda L, cur, ft, gt, nxt: h0.ncg_search_step_dev(
                st.data_ptr(), M, P, lists.data_ptr(), L, cur.data_ptr(), ft.data_ptr(), gt.data_ptr(), prm, maxiter, 0,
                nxt.data_ptr(), V.data_ptr(), flags.data_ptr()),
            stream, done)
        if verbose:
            print("lock-step Newton-CG outer iteration %d: %d CG iterations, %d trial launches, %d rows running"
                  % (counts['outer'], ncg, launch, int(np.sum(fl != PHASE_DONE))))
        if on_outer is not None:
            sch = sc.cpu().numpy()
            on_outer(counts['outer'], {'X': X.cpu().numpy(), 'status': sch[SC_STATUS].astype(int), 'nit': sch[SC_NIT].astype(int),
                                       'nhev': sch[SC_NHEV].astype(int), 'applies': counts['apply']})
    Xh = X.cpu().numpy()
    sch = sc.cpu().numpy()
    pk.unpack(x, Xh, n_lo, n_hi)
    fun = sch[SC_F].copy()
    nit, nfev, nhev = sch[SC_NIT].astype(int), sch[SC_NFEV].astype(int), sch[SC_NHEV].astype(int)
    status = sch[SC_STATUS].astype(int)
    population.last_fit_stats = {'optimizer': 'lock-step Newton-CG (hip row kernels)', 'outer_iterations': counts['outer'],
                                 'apply_launches': counts['apply'], 'prepare_launches': counts['prepare'],
                                 'll_grad_launches': whole.list_count + whole.count,
                                 'neuron_evaluations': whole.list_rows + M * whole.count,
                                 'cg_lengths': list(counts['cg_lengths']), 'apply_kernels': counts.get('apply_kernels'),
                                 'per_neuron': {'nit': [int(v) for v in nit], 'nhev': [int(v) for v in nhev],
                                                'nfev': [int(v) for v in nfev], 'status': [int(v) for v in status]}}
    return fun, nit, nfev, nhev, status
