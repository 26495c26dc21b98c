"""
Group-lasso MAP by lock-step accelerated proximal gradient, with a warm-started regularisation path.

The group-lasso prior on the impulse weights (one group per presynaptic neuron) is how standard_glm gets a sparse network
without the Gibbs sampler.  Its objective is not smooth: a quasi-Newton fit (batched_bfgs.py serves the prior through
pgl_bfgs_objective_dev kind 1) never puts a group at exactly zero, so a network can only be read off it by thresholding.
Here the per-neuron problems F = f + h -- f the smooth part (minus ll, bias and stimulus priors), h = (lam / sigma) sum_g
|w_g - mu| -- are solved by FISTA with backtracking and function restart (csrc/pglm_prox.h states the machine once, for
hipcc and gcc): the group soft-threshold gives EXACT zeros, and the KKT residual is a stopping rule that means something.
Given the network the neurons are independent and ONE pgl_ll_grad_dev evaluates all of them, so the M fits advance in lock
step: every call of the machine is one evaluation over all rows plus one row launch (pgl_prox_*, one workgroup per
neuron) on state that never leaves the device.  lam is a per-row device array: every neuron may have its own.  Only the
rows' phase flags cross PCIe, through pinned memory the row kernels write themselves; the driver reads them behind an
event every POLL launches and never waits per iteration (a finished row is frozen, so the launches in flight are harmless).
PyTorch is plumbing (device memory, the stream, pinned flags); no library kernel is on the path, except the sum over the
data sequences of a population that has several.

Served: populations whose per-neuron vector is the device's theta row (_Packing.identity) with a GroupLasso impulse prior.
Gaussian impulse priors, the 'st' and Dirichlet packings and time-sharded populations raise ValueError before any device work.
"""
import copy

import numpy as np

from theano_pyglm_amd.components.priors import GroupLasso
from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.lockstep import RangeEvaluator, _host_buffers, session

PHASE_Y, PHASE_TRIAL, PHASE_DONE = 0.0, 1.0, 2.0
# rows of the scalar block of the state (PglProx, csrc/pglm_prox.h)
FIELDS = ('f_x', 'F_x', 'f_y', 't', 'tk', 'iters', 'nfev', 'nbt', 'restarts', 'phase', 'status', 'kkt', 'y_is_x', 'm_sd',
          'm_restart', 'm_zero', 'm_kkt')
SC = dict((n, i) for i, n in enumerate(FIELDS))
NVEC = 5
POLL = 4                                                       # launches between two looks at the flags

def supported(population):
    return population.glm.hvp_packing() is None and isinstance(population.glm.imp_model.prior, GroupLasso)


def _check(population):
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("lock-step proximal gradient: the row kernels are not implemented for the %s packing" % bad)
    if not isinstance(population.glm.imp_model.prior, GroupLasso):
        raise ValueError("lock-step proximal gradient solves the group-lasso MAP: the impulse prior is %s (a smooth prior is "
                         "fitted by lock-step BFGS or Newton-CG)" % type(population.glm.imp_model.prior).__name__)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("lock-step proximal gradient does not run on a time-sharded population (set_time_shard): "
                         "evaluations are not all-reduced")


def _row_lams(population, lam, M):
    if lam is None:
        lam = float(population.glm.imp_model.prior.lam)
    lam = np.asarray(lam, dtype=float)
    if lam.ndim > 1 or (lam.ndim == 1 and lam.shape != (M,)):
        raise ValueError("lam: None, a number or an (M,) = (%d,) array" % M)
    lam = np.ascontiguousarray(np.broadcast_to(lam, (M,)))
    if np.any(np.isnan(lam)) or np.any(lam < 0.0):
        raise ValueError("lam must not be negative (+inf is allowed: the null model)")
    return lam


def fit_glms_prox(population, x, lam=None, maxiter=500, gtol=1e-5, max_backtrack=40, n_lo=0, n_hi=None, verbose=False):
    """In-place group-lasso MAP fit of x['glms'][n_lo:n_hi] given the rest of x.  lam: None (the prior's), a number or one
    per neuron (M,).  Returns per-neuron arrays {'status' (0 converged: KKT residual <= gtol, 1 maxiter, 2 max_backtrack
    failed trials in one iteration), 'iters', 'nfev', 'kkt', 'objective' (F = minus compute_log_p's per-neuron term),
    'support' (M, N) bool: the presynaptic groups that are not exactly mu, 'lam'}.
    population.last_fit_stats records the launch counts, the looks at the flags and 'loop_s', the wall time from behind
    the init launch to the end of the last launch (no packing, upload or copy back)."""
    res, _, _ = _fit(population, x, lam, maxiter, gtol, max_backtrack, n_lo, n_hi, verbose, write=True)
    return res


def _fit(population, x, lam, maxiter, gtol, max_backtrack, n_lo, n_hi, verbose, write):
    _check(population)
    maxiter, max_backtrack, gtol = int(maxiter), int(max_backtrack), float(gtol)
    if max_backtrack <= 0 or not gtol > 0.0:
        raise ValueError("max_backtrack and gtol must be positive")
    N = population.N
    n_hi = N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    lam = _row_lams(population, lam, M)
    with session(population) as (torch, dev, stream, handles):
        return _lockstep(population, torch, dev, stream, handles, x, lam, maxiter, gtol, max_backtrack, n_lo, n_hi, M, verbose, write)


def _lockstep(population, torch, dev, stream, handles, x, lam, maxiter, gtol, max_backtrack, n_lo, n_hi, M, verbose, write):
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    if not pk.identity:
        raise ValueError("lock-step proximal gradient: the per-neuron vector of this population is not the device's theta row")
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    MP = M * P
    st = torch.zeros(h0.prox_state_doubles(M, P), dtype=f64, device=dev)
    X = st[0:MP].view(M, P)
    Gx = st[3 * MP:4 * MP].view(M, P)
    sc = st[NVEC * MP:].view(len(FIELDS), M)
    X.copy_(torch.tensor(pk.pack(x, n_lo, n_hi), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    d_lam = torch.tensor(lam, dtype=f64, device=dev)
    Xt = torch.empty((M, P), dtype=f64, device=dev)
    evaluate = RangeEvaluator(torch, dev, handles, Weff, M, P, n_lo, n_hi)
    flags = _host_buffers(torch, dev.index, M)[0]
    flags.fill_(PHASE_TRIAL)
    fl = flags.numpy()
    counts = {'row': 0, 'polls': 0}

    ll0, g0 = evaluate(X)
    h0.prox_init_dev(st.data_ptr(), M, P, ll0.data_ptr(), g0.data_ptr(), prm, d_lam.data_ptr(), gtol, maxiter, Xt.data_ptr(),
                     flags.data_ptr())
    counts['row'] += 1
    import time
    t_loop = time.perf_counter()
    # rows that end in init (already at their optimum, or maxiter <= 0) cost no further launch: one look behind init's event
    ev0 = torch.cuda.Event()
    ev0.record(stream)
    ev0.synchronize()
    counts['polls'] += 1
    all_done = bool(np.all(fl == PHASE_DONE))
    # every row ends: an iteration is at most 2 + max_backtrack calls (a restart does not reset the count of failed trials)
    cap = 2 + max(maxiter, 0) * (max_backtrack + 2)
    events = []
    k = 0
    while not all_done:
        if k % POLL == 0:
            ev = torch.cuda.Event()
            ev.record(stream)
            events.append(ev)
            if len(events) > 1:                               # the look lags one window behind: the queue never runs dry
                events.pop(0).synchronize()
                counts['polls'] += 1
                if np.all(fl == PHASE_DONE):
                    break
                if verbose:
                    print("lock-step proximal gradient: %d launches, %d rows running" % (k, int(np.sum(fl != PHASE_DONE))))
        if k >= cap:
            stream.synchronize()
            if np.all(fl == PHASE_DONE):
                break
            raise RuntimeError("lock-step proximal gradient: rows still running after %d launches" % k)
        llt, gt = evaluate(Xt)
        h0.prox_step_dev(st.data_ptr(), M, P, llt.data_ptr(), gt.data_ptr(), prm, d_lam.data_ptr(), gtol, maxiter, max_backtrack,
                         Xt.data_ptr(), flags.data_ptr())
        counts['row'] += 1
        k += 1
    stream.synchronize()
    loop_s = time.perf_counter() - t_loop
    Xh = X.cpu().numpy()
    sch = sc.cpu().numpy()
    gxh = Gx.cpu().numpy()
    if write:
        pk.unpack(x, Xh, n_lo, n_hi)
    o = 1 + pk.nbk
    res = {'status': sch[SC['status']].astype(int), 'iters': sch[SC['iters']].astype(int), 'nfev': sch[SC['nfev']].astype(int),
           'kkt': sch[SC['kkt']].copy(), 'objective': sch[SC['F_x']].copy(),
           'support': np.any(Xh[:, o:].reshape(M, pk.N, pk.B) != prm[4], axis=2), 'lam': lam.copy()}
    population.last_fit_stats = {'optimizer': 'lock-step proximal gradient (hip row kernels)', 'll_grad_launches': evaluate.count,
                                 'row_launches': counts['row'], 'flag_polls': counts['polls'], 'loop_s': loop_s,
                                 'restarts': [int(v) for v in sch[SC['restarts']]],
                                 'per_neuron': {'iters': [int(v) for v in res['iters']], 'nfev': [int(v) for v in res['nfev']],
                                                'status': [int(v) for v in res['status']]}}
    return res, Xh, gxh


def lasso_lam_max(population, x, n_lo=0, n_hi=None, **fit):
    """The smallest lam per neuron (M,) at which every group is zero: sigma max_g |d ll / d w_g|_2 at the null model, which
    is fitted by the solver itself with lam = +inf (the prox then sends every group to mu; bias and stimulus weights are
    fitted), from x.  The gradient is the one evaluation the solver made at its last point.  x is not changed.
    RESTRICTION: 'every group is zero' holds for lam > lam_max, not at lam = lam_max itself.  There the last group's KKT
    condition holds with EQUALITY, F is flat to first order along that group, and a fit that stops at a KKT residual <= gtol
    may stop with the group O(gtol / curvature) away from mu (measured on the host tests' problem: up to 9e-4 at gtol 1e-5,
    however tightly the null model itself is fitted).  The returned number also carries the null fit's own gtol.  A grid
    that must start at an empty support starts a little above: the tests use 1.001 lam_max, and that is what they assert."""
    _check(population)
    n_hi = population.N if n_hi is None else n_hi
    res, Xh, G = _fit(population, x, np.inf, fit.get('maxiter', 500), fit.get('gtol', 1e-5), fit.get('max_backtrack', 40), n_lo,
                      n_hi, fit.get('verbose', False), write=False)
    if res['support'].any():
        raise RuntimeError("lasso_lam_max: the null fit left a group away from mu")
    pr = population.glm.imp_model.prior
    M, P = Xh.shape
    B = population.glm.imp_model.B
    gw = G[:, P - population.N * B:].reshape(M, population.N, B)
    return float(pr.sigma) * np.max(np.sqrt(np.sum(gw * gw, axis=2)), axis=1)


def lasso_path(population, x0, lams=None, n_lams=10, lam_ratio=1e-2, heldout=None, n_lo=0, n_hi=None, **fit):
    """The fits along a descending grid of lam, each warm-started from the last (the first from x0).

    lams: (L,) -- one lam for all neurons per point -- or (L, M), one per neuron; None: n_lams points, geometric from the
    median lasso_lam_max over the neurons down to lam_ratio times it.  heldout: a preprocessed data set; every point is
    scored on it by compute_ll_vector.  fit: maxiter, gtol, max_backtrack, verbose of fit_glms_prox.
    Returns {'lams' (L,) or (L, M), 'X' (L, M, P) rows in the theta layout, 'support' (L, M, N), 'objective' (L, M),
    'status' (L, M), 'iters' (L, M)} and, with heldout, 'heldout_ll' (L, M), 'best' (M,) the index of every neuron's best
    point (the first of equals: the sparser one) and 'x_best', a state dict assembled row by row from each neuron's best point.
    x0 is not changed."""
    _check(population)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    if lams is None:
        top = float(np.median(lasso_lam_max(population, x0, n_lo, n_hi, **fit)))
        lams = top * np.geomspace(1.0, float(lam_ratio), int(n_lams))
    lams = np.asarray(lams, dtype=float)
    if lams.ndim not in (1, 2) or lams.shape[0] == 0 or (lams.ndim == 2 and lams.shape[1] != M):
        raise ValueError("lams: an (L,) or (L, M) array")
    if np.any(np.diff(lams, axis=0) > 0.0):
        raise ValueError("lams must descend")
    x = copy.deepcopy(x0)
    pk = _Packing(population, None)
    out = {'lams': lams.copy(), 'X': [], 'support': [], 'objective': [], 'status': [], 'iters': []}
    held = []
    current = population._current
    for lam in lams:
        res = fit_glms_prox(population, x, lam=lam, n_lo=n_lo, n_hi=n_hi, **fit)
        out['X'].append(pk.pack(x, n_lo, n_hi))
        for k in ('support', 'objective', 'status', 'iters'):
            out[k].append(res[k])
        if heldout is not None:
            population.set_data(heldout)
            held.append(np.array(population.compute_ll_vector(x, n_lo, n_hi)))
    for k in ('X', 'support', 'objective', 'status', 'iters'):
        out[k] = np.array(out[k])
    if heldout is not None:
        if current is not None:
            population.set_data(current)
        out['heldout_ll'] = np.array(held)
        out['best'] = np.argmax(out['heldout_ll'], axis=0)
        xb = copy.deepcopy(x0)
        pk.unpack(xb, out['X'][out['best'], np.arange(M)], n_lo, n_hi)
        out['x_best'] = xb
    return out
