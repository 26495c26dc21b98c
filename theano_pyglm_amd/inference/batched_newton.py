"""
Lock-step dense Newton for all neurons with the optimiser state resident on the GPU.

The reference's parallel driver fits every neuron with the dense Hessian of its log posterior by default
(parallel_coord_descent.py:62 use_hessian=True; map.py:38-45).  Here that route runs as one lock-step optimiser, the dense
counterpart of batched_newton_cg.py: a line-search Newton method with Hessian modification (csrc/pglm_newton.h) whose
state machines are HIP row kernels (pgl_newton_*, one workgroup per neuron) on state that never leaves the device.  Per
outer iteration, for the rows still running and nothing else:
    the list of running rows  ->  pgl_hvp_prepare_list_dev + pgl_hess_dev on every data sequence, summed  ->
    pgl_newton_assemble_dev (A = -H - H_prior, the right-hand side -g)  ->  pgl_chol_factor_dev  ->  pgl_chol_solve_dev  ->
    pgl_newton_direction_dev; rows whose factor failed or whose direction does not descend raise their shift and go
    through assemble / factor / solve / direction again, from the unshifted copy of the SAME Hessian  ->
    line-search evaluations (pgl_ll_grad_list_dev + pgl_newton_search_step_dev) until no row searches.
A row that has converged costs no Hessian any more: the work goes by row list.  Only the per-row phase flags cross PCIe,
through pinned memory the row kernels write themselves.  PyTorch is plumbing (device memory, copies, the stream, pinned
flags); no library kernel is on the path, except the sum over the data sequences of a population that has several.

The Hessians of a list live in two buffers of L * P * ld doubles (the work copy that the factor overwrites and the
unshifted one); a list whose buffers would exceed `hess_budget_bytes` (default 4 GB) runs in slices.

Served: exactly what batched_newton_cg serves (lockstep._check): theta-row packings under a Gaussian or group-lasso prior, no
time shard.
"""
import time

import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.lockstep import (RangeEvaluator, _check, _host_buffers, search_phase, send_list,  # noqa: F401
                                                 session, supported, wait)

PHASE_HESS, PHASE_SEARCH, PHASE_DONE, PHASE_REFACTOR = 0.0, 1.0, 2.0, 3.0
# rows of the scalar block of the state (PglNewton, csrc/pglm_newton.h)
SC_F, SC_SHIFT, SC_NIT, SC_NFEV, SC_NHESS, SC_NFACT, SC_STATUS, SC_PHASE = 0, 4, 5, 6, 7, 8, 9, 10
NVEC = 5
HESS_BUDGET_BYTES = 4 << 30


def fit_glms_newton_torch(population, x, maxiter=50, gtol=1e-5, n_lo=0, n_hi=None, verbose=False, on_outer=None,
                          hess_budget_bytes=HESS_BUDGET_BYTES, timings=None):
    """In-place MAP fit of x['glms'][n_lo:n_hi] by lock-step dense Newton; returns per-row arrays (fun, nit, nfev, nhess,
    status): status 0 converged (max|g| <= gtol), 1 maxiter, 2 the line search found no acceptable point, 3 no descent
    direction.

    on_outer: optional callable(k, info) after every outer iteration k = 1, 2, ... with host copies
    info = {'X', 'status', 'nit', 'nhess', 'shift'} (a synchronising copy: for tests and traces).
    timings: optional dict; receives the seconds spent in 'hess', 'factor', 'solve', 'eval' (each phase is then
    synchronised: for benchmarks).  population.last_fit_stats records the launch counts."""
    _check(population)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    with session(population) as (torch, dev, stream, handles):
        out = _lockstep(population, torch, dev, stream, handles, x, int(maxiter), float(gtol), n_lo, n_hi, M, verbose,
                        on_outer, int(hess_budget_bytes), timings)
        stream.synchronize()
    return out


def _lockstep(population, torch, dev, stream, handles, x, maxiter, gtol, n_lo, n_hi, M, verbose, on_outer, budget, timings):
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    ld = P
    prm = pk.prior_params()
    f64 = torch.float64
    st = torch.zeros(h0.newton_state_doubles(M, P), dtype=f64, device=dev)
    MP = M * P
    X = st[0:MP].view(M, P)
    sc = st[NVEC * MP:].view(-1, M)
    X.copy_(torch.tensor(pk.pack(x, n_lo, n_hi), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    whole = RangeEvaluator(torch, dev, handles, Weff, M, P, n_lo, n_hi)          # (its buffers serve the lists too)
    Xts = [torch.empty((M, P), dtype=f64, device=dev) for _ in range(2)]
    rhs = torch.empty((M, P), dtype=f64, device=dev)
    lists = torch.empty(3 * M, dtype=torch.int32, device=dev)
    flags, stage = _host_buffers(torch, dev.index, M)
    flags.fill_(PHASE_DONE)
    fl = flags.numpy()
    done = torch.cuda.Event()
    per = max(1, min(M, budget // (2 * P * ld * 8)))          # rows per slice: two buffers of `per` matrices
    Hraw = torch.empty((per, P, ld), dtype=f64, device=dev)
    Awork = torch.empty((per, P, ld), dtype=f64, device=dev)
    counts = {'hess': 0, 'hess_rows': 0, 'factor': 0, 'factor_rows': 0, 'solve': 0, 'outer': 0, 'refactor_rows': 0}
    tm = {'hess': 0.0, 'factor': 0.0, 'solve': 0.0, 'eval': 0.0}

    def timed(key, t0):
        if timings is not None:
            stream.synchronize()
            tm[key] += time.perf_counter() - t0

    def send(rows):
        return send_list(stage, lists, rows, n_lo, M)

    def evaluate(Xt, idx32, L):
        t0 = time.perf_counter()
        out = whole.eval_list(Xt, idx32, L)
        timed('eval', t0)
        return out

    def factor_solve_direction(L):
        """assemble, factor, solve and direction of the L listed rows: Awork[:L] holds the Hessians of ll"""
        A = Awork[:L]
        b = rhs[:L]
        t0 = time.perf_counter()
        h0.newton_assemble_dev(st.data_ptr(), M, P, lists.data_ptr(), L, A.data_ptr(), ld, prm, b.data_ptr())
        scale, _, info = h0.chol_factor(A)
        counts['factor'] += 1
        counts['factor_rows'] += L
        timed('factor', t0)
        t0 = time.perf_counter()
        h0.chol_solve(A, scale, info, b, out=b)
        counts['solve'] += 1
        timed('solve', t0)
        h0.newton_direction_dev(st.data_ptr(), M, P, lists.data_ptr(), L, info.data_ptr(), b.data_ptr(), flags.data_ptr())
        wait(stream, done)

    ll0, g0 = whole(X)
    h0.newton_init_dev(st.data_ptr(), M, P, ll0.data_ptr(), g0.data_ptr(), prm, gtol, maxiter, flags.data_ptr())
    wait(stream, done)
    while np.any(fl != PHASE_DONE):
        counts['outer'] += 1
        # -- Newton directions of the rows that need a Hessian, a slice at a time
        running = np.nonzero(fl == PHASE_HESS)[0].astype(np.int32)
        for s0 in range(0, running.size, per):
            rows = running[s0:s0 + per]
            L = send(rows)
            t0 = time.perf_counter()
            h0.newton_trial_dev(st.data_ptr(), M, P, lists.data_ptr(), L, Xts[0].data_ptr())     # (phase 0: the points)
            for h in handles:
                dst = Hraw if h is h0 else Awork
                h.hvp_prepare(Xts[0].data_ptr(), Weff.data_ptr(), d_idx=lists[M:].data_ptr(), count=L)
                h.hess(dst.data_ptr(), ld)
                if h is not h0:
                    Hraw[:L].add_(Awork[:L])
            counts['hess'] += 1
            counts['hess_rows'] += L
            timed('hess', t0)
            Awork[:L].copy_(Hraw[:L])
            factor_solve_direction(L)
            pos = rows                                         # pos[j]: the row at position j of Hraw
            again = np.nonzero(fl[pos] == PHASE_REFACTOR)[0]
            while again.size:
                # the flagged rows alone, from the unshifted copy: their Hessians move to the front of both buffers
                for j, src in enumerate(again):
                    if j != src:
                        Hraw[j].copy_(Hraw[src])
                pos = pos[again]
                L = send(pos)
                Awork[:L].copy_(Hraw[:L])
                counts['refactor_rows'] += L
                factor_solve_direction(L)
                again = np.nonzero(fl[pos] == PHASE_REFACTOR)[0]
        # -- line-search phase: the rows still searching, one evaluation per trial step
        launch = search_phase(
            fl, PHASE_SEARCH, M, n_lo, stage, lists, Xts, evaluate,
            lambda L, cur: h0.newton_trial_dev(st.data_ptr(), M, P, lists.data_ptr(), L, cur.data_ptr()),
            lambda L, cur, ft, gt, nxt: h0.newton_search_step_dev(
                st.data_ptr(), M, P, lists.data_ptr(), L, cur.data_ptr(), ft.data_ptr(), gt.data_ptr(), prm, gtol, maxiter, 0,
                nxt.data_ptr(), flags.data_ptr()),
            stream, done)
        if verbose:
            print("lock-step Newton outer iteration %d: %d Hessians, %d trial launches, %d rows running"
                  % (counts['outer'], int(running.size), launch, int(np.sum(fl != PHASE_DONE))))
        if on_outer is not None:
            sch = sc.cpu().numpy()
            on_outer(counts['outer'], {'X': X.cpu().numpy(), 'status': sch[SC_STATUS].astype(int), 'nit': sch[SC_NIT].astype(int),
                                       'nhess': sch[SC_NHESS].astype(int), 'shift': sch[SC_SHIFT].copy()})
    Xh = X.cpu().numpy()
    sch = sc.cpu().numpy()
    pk.unpack(x, Xh, n_lo, n_hi)
    fun = sch[SC_F].copy()
    nit, nfev, nhess = sch[SC_NIT].astype(int), sch[SC_NFEV].astype(int), sch[SC_NHESS].astype(int)
    nfact, status = sch[SC_NFACT].astype(int), sch[SC_STATUS].astype(int)
    if timings is not None:
        timings.update(tm)
    population.last_fit_stats = {'optimizer': 'lock-step dense Newton (hip row kernels)', 'outer_iterations': counts['outer'],
                                 'hess_launches': counts['hess'], 'hess_rows': counts['hess_rows'],
                                 'factor_launches': counts['factor'], 'factor_rows': counts['factor_rows'],
                                 'solve_launches': counts['solve'], 'refactor_rows': counts['refactor_rows'],
                                 'll_grad_launches': whole.list_count + whole.count,
                                 'neuron_evaluations': whole.list_rows + M * whole.count,
                                 'rows_per_slice': int(per),
                                 'per_neuron': {'nit': [int(v) for v in nit], 'nhess': [int(v) for v in nhess],
                                                'nfact': [int(v) for v in nfact], 'nfev': [int(v) for v in nfev],
                                                'status': [int(v) for v in status]}}
    return fun, nit, nfev, nhess, status
