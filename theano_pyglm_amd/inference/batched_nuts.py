"""
The No-U-Turn sampler for the per-neuron GLM posteriors with the chain state resident on the GPU.

The setting is batched_hmc's: given the network the neurons' parameter rows have independent posteriors, and ONE
pgl_ll_grad_dev evaluates all of them for the price of one.  What changes is the transition: multinomial NUTS (Hoffman &
Gelman 2014; Betancourt 2017) as inference/nuts.py states it and csrc/pglm_nuts.h restates it in O(max_depth) storage --
no trajectory length to guess -- with a step size per row from dual averaging towards target_accept during the warm-up,
frozen afterwards.  It runs as HIP row kernels (pgl_nuts_*, one workgroup per neuron) on state that never leaves the
device.  Trees differ in size from row to row and from transition to transition, so the rows do not wait for each other:
every launch is one leapfrog step of every row that still has transitions to run, a row that ends a transition starts
its next one in the same launch, counts its own t and writes its kept points itself; a row that has finished idles (its
evaluation is wasted: 'idle_row_evaluations').  The host only enqueues evaluation + step launches and looks at the rows'
done flags behind an event every POLL launches, one window late, so the queue never runs dry.

The mass matrix is batched_hmc's: None, 'laplace', an (M, P) array, 'laplace_dense' or an (M, P, P) array
(factor_inverse_mass; factor_on_device=True builds the Laplace factor on the device).  All of them are one code path: the
chain runs in the whitened momentum r = W^T p, a diagonal W inside the row kernel, a dense one through two
pgl_tri_matvec_dev products per leapfrog step.

Served: the populations batched_hmc serves, with the same errors for the others.
"""
import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.batched_hmc import _check, _check_chains, chain_starts, per_row, resolve_mass, split_chains
from theano_pyglm_amd.inference.batched_hmc import (_laplace_minv, factor_inverse_mass, samples_to_states,  # noqa: F401
                                                    summarize, supported)                                   # (the same here)
from theano_pyglm_amd.inference.lockstep import RangeEvaluator, session

# rows of the scalar block of the state (PglNuts, csrc/pglm_nuts.h)
SC_STEP, SC_T, SC_DONE, SC_NLEAP, SC_NDIV, SC_ACC = 2, 3, 7, 21, 22, 23
NSCAL, NVEC = 30, 17
POLL = 8                                                      # launches between two looks at the done flags


def sample_glms_nuts(population, x, n_samples, n_warmup=200, max_depth=8, step_sz=0.1, target_accept=0.8, thin=1, mass=None,
                     seed=0, n_lo=0, n_hi=None, factor_on_device=False, mass_floor=1e-8, n_chains=1, init_jitter=0.0, diagnostics=False,
                     filters=False):
    """Posterior samples of the parameter rows of neurons [n_lo, n_hi) given the rest of x, started at x.

    n_warmup transitions adapt every row's step size (dual averaging towards target_accept) and are dropped; then
    n_samples * thin transitions, every thin-th kept.  max_depth: at most that many doublings per transition (1 .. 10).
    step_sz: the starting step, a number or one per row.  mass, factor_on_device, mass_floor, n_chains, init_jitter: as
    sample_glms_hmc.  mass='adapt' runs inside the step kernel (rows are asynchronous: every row switches at its own
    transition boundary, csrc/pglm_nuts.hip.h) and restarts the row's dual averaging at every window's end; the result
    gains 'minv' and 'adapt_windows'.  With n_chains > 1 every per-row result gains a leading chain axis.
    Returns sample_glms_hmc's dict -- 'samples' (n_samples, M, P), 'accept_rate' (M,) (here the mean acceptance statistic
    after warm-up), 'step_sz' (M,) the frozen steps, 'n_evals', with 'laplace_dense' 'dense_rows' -- and 'depth',
    'n_leapfrog' (n_samples, M) of the kept transitions, 'divergent' (M,) divergent transitions after warm-up, 'step'
    (= 'step_sz'), 'launches' (evaluation + step launches: the largest number of leapfrog steps of any row, plus fewer
    than 2 POLL because the done flags are read every POLL launches and one window late) and 'idle_row_evaluations' (the
    sum over rows of launches - the row's leapfrog steps).  x is not changed.
    diagnostics=True: as sample_glms_hmc -- 'summary', from k_diag_column on the device tensor of the draws.
    filters=True (or a level): as sample_glms_hmc -- 'filters', from k_filter_bands on the same tensor."""
    _check(population)
    n_samples, n_warmup, max_depth, thin = int(n_samples), int(n_warmup), int(max_depth), int(thin)
    if n_samples <= 0 or n_warmup < 0 or thin <= 0:
        raise ValueError("n_samples and thin must be positive, n_warmup not negative")
    if not 1 <= max_depth <= 10:
        raise ValueError("max_depth: 1 .. 10")
    if not 0.0 < float(target_accept) < 1.0:
        raise ValueError("target_accept: in (0, 1)")
    n_chains, init_jitter = _check_chains(n_chains, init_jitter)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    mass, factor, dense_rows, setup_s = resolve_mass(population, x, mass, n_lo, n_hi, mass_floor, factor_on_device)
    step_sz = np.ascontiguousarray(np.broadcast_to(np.asarray(step_sz, dtype=float), (M,)))
    if not np.all(step_sz > 0.0):
        raise ValueError("step_sz must be positive")
    with session(population) as (torch, dev, stream, handles):
        out = _chain(population, torch, dev, stream, handles, x, n_samples, n_warmup, max_depth, step_sz,
                     float(target_accept), thin, mass, int(seed), n_lo, n_hi, M, factor, n_chains, init_jitter,
                     bool(diagnostics), filters)
    if dense_rows is not None:
        out['dense_rows'] = dense_rows
    population.last_fit_stats['mass_setup_s'] = setup_s
    return out


def _chain(population, torch, dev, stream, handles, x, n_keep, n_warmup, D, step_sz, delta, thin, mass, seed, n_lo, n_hi, M,
           factor, n_chains=1, init_jitter=0.0, diagnostics=False, filters=False):
    from theano_pyglm_amd.inference.mass_adapt import adapt_windows, schedule_ints
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    C, R = n_chains, n_chains * M                             # rows: chain c of neuron n_lo + m is row c M + m
    RP = R * P
    st = torch.zeros(h0.nuts_state_doubles(R, P, D), dtype=f64, device=dev)
    sc = st[(NVEC + 2 * D) * RP:].view(NSCAL, R)
    st[0:RP].view(R, P).copy_(torch.tensor(chain_starts(pk, x, n_lo, n_hi, C, seed, init_jitter), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    minv = Wd = None
    assert P == population.glm.P                              # (mass and step_sz were checked against it by the caller)
    adapt = isinstance(mass, str) and mass == 'adapt'
    windows, ad, sched = [], None, None
    if adapt:                                                 # ones: the identity chain until a row's first window ends
        minv = torch.ones((R, P), dtype=f64, device=dev)
        windows = adapt_windows(n_warmup)
        if windows:
            ad = torch.zeros(h0.adapt_state_doubles(R, P), dtype=f64, device=dev)
            sched = torch.tensor(schedule_ints(windows), dtype=torch.int32, device=dev)
    elif mass is not None:
        minv = per_row(torch.tensor(mass, dtype=f64, device=dev), M, C)
    if factor is not None:                                    # (M, P, P) lower-triangular factors: uploaded once
        assert tuple(factor.shape) == (M, P, P)
        Wd = per_row(factor if torch.is_tensor(factor) else torch.tensor(factor, dtype=f64, device=dev), M, C)
    step0 = torch.tensor(np.tile(step_sz, C), dtype=f64, device=dev)
    minv_ptr = minv.data_ptr() if minv is not None else 0
    W_ptr = Wd.data_ptr() if Wd is not None else 0
    Xt = torch.empty((R, P), dtype=f64, device=dev)
    evaluate = RangeEvaluator(torch, dev, handles, Weff, M, P, n_lo, n_hi, C)
    samples = torch.zeros((n_keep, R, P), dtype=f64, device=dev)
    stats = torch.zeros((n_keep, 2, R), dtype=f64, device=dev)
    flags = [torch.zeros(R, dtype=f64).pin_memory() for _ in range(2)]
    counts = {'polls': 0}

    ll0, g0 = evaluate(st[0:RP].view(R, P))
    h0.nuts_init_dev(st.data_ptr(), M, P, D, n_lo, ll0.data_ptr(), g0.data_ptr(), prm, minv_ptr, W_ptr, step0.data_ptr(),
                     seed, n_warmup, thin, n_keep, Xt.data_ptr(), n_chains=C)
    launches, events, all_done = 0, [], False
    while not all_done:
        llt, gt = evaluate(Xt)
        if windows:
            h0.nuts_adapt_step_dev(st.data_ptr(), R, P, D, llt.data_ptr(), gt.data_ptr(), prm, minv_ptr, ad.data_ptr(),
                                   sched.data_ptr(), delta, n_warmup, thin, n_keep, Xt.data_ptr(), samples.data_ptr(),
                                   stats.data_ptr())
        else:
            h0.nuts_step_dev(st.data_ptr(), R, P, D, llt.data_ptr(), gt.data_ptr(), prm, minv_ptr, W_ptr, delta, n_warmup, thin,
                             n_keep, Xt.data_ptr(), samples.data_ptr(), stats.data_ptr())
        launches += 1
        if launches % POLL == 0:
            fl = flags[(launches // POLL) % 2]
            fl.copy_(sc[SC_DONE], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            events.append((ev, fl))
            if len(events) > 1:                               # the look lags one window behind: the queue never runs dry
                ev, fl = events.pop(0)
                ev.synchronize()
                counts['polls'] += 1
                all_done = bool(np.all(fl.numpy() != 0.0))
    if diagnostics:                                           # (every row is done: the draws are complete on the device)
        from theano_pyglm_amd.inference.diagnostics import queue_summary, finish_summary
        diag_rows = queue_summary(h0, samples, C)
    if filters:
        from theano_pyglm_amd.inference.filters import queue_bands, finish_bands, filters_level
        bands = queue_bands(population, h0, torch, samples, C, filters_level(filters))
    stream.synchronize()
    sch = sc.cpu().numpy()
    sth = stats.cpu().numpy()
    nleap = sch[SC_NLEAP]
    step = split_chains(sch[SC_STEP].copy(), M, C, 0)
    out = {'samples': split_chains(samples.cpu().numpy(), M, C, 1),
           'accept_rate': split_chains(sch[SC_ACC] / float(n_keep * thin), M, C, 0), 'step_sz': step,
           'n_evals': evaluate.count, 'depth': split_chains(sth[:, 0].astype(int), M, C, 1),
           'n_leapfrog': split_chains(sth[:, 1].astype(int), M, C, 1),
           'divergent': split_chains(sch[SC_NDIV].astype(int), M, C, 0), 'step': step.copy(), 'launches': launches,
           'idle_row_evaluations': int(np.sum(launches - nleap))}
    if adapt:
        out['minv'] = split_chains(minv.cpu().numpy(), M, C, 0)
        out['adapt_windows'] = windows
    if diagnostics:
        out['summary'] = finish_summary(diag_rows, out['samples'], C)
    if filters:
        out['filters'] = finish_bands(population, bands, samples, C, filters_level(filters))
    assert np.all(sch[SC_DONE] != 0.0) and np.all(sch[SC_T] == n_warmup + n_keep * thin)
    population.last_fit_stats = {'sampler': 'NUTS (hip row kernels)', 'transitions': n_warmup + n_keep * thin,
                                 'mass': 'dense' if Wd is not None else ('adapted diagonal' if adapt else
                                                                         ('diagonal' if minv is not None else 'identity')),
                                 'll_grad_launches': evaluate.count, 'step_launches': launches,
                                 'leapfrog_steps': nleap.astype(int), 'flag_reads': counts['polls'],
                                 'idle_share': float(np.sum(launches - nleap)) / float(launches * R)}
    if C > 1:
        population.last_fit_stats['n_chains'] = C
    return out
