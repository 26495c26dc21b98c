"""
Lock-step Hamiltonian Monte Carlo for the per-neuron GLM posteriors with the chain state resident on the GPU.

Given the network, the posteriors of the neurons' parameter rows (bias, w_stim, w_ir) are independent, and ONE
pgl_ll_grad_dev evaluates all of them for the price of one.  So the N chains advance in lock step: every leapfrog step
is one evaluation over all rows of the range, and the algorithm itself -- Neal (2011) fig. 2 as inference/hmc.py states
it, restated in csrc/pglm_hmc.h -- runs as HIP row kernels (pgl_hmc_*, one workgroup per neuron) on state that never
leaves the device: momentum draw, leapfrog, accept step and step-size rule.  All rows take the same number of steps, so
there are no lists and no flags: the whole run of n_transitions x (2 n_leapfrog + 1) launches is enqueued without one
host synchronisation, and the kept samples are written by the kernel into one device tensor that is copied once at the end.
PyTorch is plumbing (device memory, the stream); no library kernel is on the path, except the sum over the data sequences
of a population that has several.

What differs from the HMC block updates of gibbs_sample (inference/gibbs.py: Hmc*Update over hmc_lockstep), which keep
their behaviour: the whole row is sampled jointly instead of one component at a time; every row has a step size of its
own, adapted during the first n_warmup transitions only (adapt_step_size of inference/hmc.py) and frozen afterwards, so
the kept chain is a valid Markov chain; the random numbers are stateless functions of (seed, neuron, transition,
component), documented in include/pyglm_hip.h, so a chain over a range of neurons equals the matching rows of a chain over
all of them.

The mass matrix is diagonal (mass=None, 'laplace' or an (M, P) array) or dense: mass='laplace_dense' or an (M, P, P)
array of inverse mass matrices Sigma, factored on the host as Sigma = W W^T (factor_inverse_mass) and uploaded once (or, for
'laplace_dense' with factor_on_device=True, built on the device).  The
dense chain (csrc/pglm_hmc_dense.h) runs in the whitened momentum r = W^T p: a leapfrog step is the same evaluation plus
two batched triangular matrix-vector products (pgl_hmc_dense_*), the draws, decisions and step-size rule unchanged.

Served: exactly the populations of batched_newton_cg.supported (the packings whose per-neuron vector is the device's
theta row, under the priors the row kernels know).  Time-sharded populations are not (nothing is all-reduced).
"""
import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.batched_newton_cg import supported  # noqa: F401  (the served populations are the same)
from theano_pyglm_amd.inference.lockstep import RangeEvaluator, session

# rows of the scalar block of the state (PglHmc, csrc/pglm_hmc.h)
SC_U0, SC_H0, SC_STEP, SC_AVG, SC_NACC, SC_T, SC_ACC = 0, 1, 2, 3, 4, 5, 6
NSCAL = 10


def _check(population):
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("lock-step HMC: the row kernels are not implemented for the %s packing" % bad)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("lock-step HMC does not run on a time-sharded population (set_time_shard): "
                         "evaluations are not all-reduced")


def _theta_positions(population, x, n_lo, P):
    """Packed position of every theta column (the per-neuron packed vector and the theta row hold the same numbers)."""
    from theano_pyglm_amd.inference.laplace import theta_positions
    pi, _ = theta_positions(population, x, n_lo)
    assert pi.size == P
    return pi


def _minv_from_hessian(H, pi, floor):
    d = -np.diagonal(H, axis1=1, axis2=2)[:, pi]
    d = np.where(np.isfinite(d), d, floor)
    return 1.0 / np.maximum(d, floor)


def _laplace_minv(population, x, n_lo, n_hi, floor):
    """1 / max(diag A, floor) in the theta layout, A = minus the Hessian of the log posterior at x."""
    H = population.compute_hessian_packed(x, n_lo, n_hi)
    return _minv_from_hessian(H, _theta_positions(population, x, n_lo, H.shape[1]), floor)


def factor_inverse_mass(Sigma, sym_tol=1e-8):
    """Lower-triangular W with W W^T = Sigma for inverse mass matrices Sigma (P, P) or (M, P, P).  Sigma must be finite,
    symmetric -- |S_ij - S_ji| <= sym_tol sqrt(S_ii S_jj): the rounding of a computed inverse passes, a matrix that was
    never meant to be symmetric does not -- and positive definite, else ValueError.  The factorisation is equilibrated
    like laplace_from_hessian's: W = D^1/2 chol(D^-1/2 Sigma D^-1/2), D = diag Sigma, so parameters on scales many orders
    of magnitude apart cost it no digits."""
    S = np.asarray(Sigma, dtype=float)
    if S.ndim not in (2, 3) or S.shape[-1] != S.shape[-2] or S.shape[-1] == 0:
        raise ValueError("inverse mass matrices: a (P, P) or (M, P, P) array, got shape %s" % (S.shape,))
    if not np.all(np.isfinite(S)):
        raise ValueError("inverse mass matrix with a NaN or infinite entry")
    d = np.diagonal(S, axis1=-2, axis2=-1)
    if not np.all(d > 0.0):
        raise ValueError("inverse mass matrix is not positive definite (a diagonal entry <= 0)")
    sd = np.sqrt(d)
    St = np.swapaxes(S, -1, -2)
    if np.any(np.abs(S - St) > sym_tol * sd[..., :, None] * sd[..., None, :]):
        raise ValueError("inverse mass matrix is not symmetric")
    C = 0.5 * (S + St) / (sd[..., :, None] * sd[..., None, :])
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        raise ValueError("inverse mass matrix is not positive definite")
    return np.ascontiguousarray(sd[..., :, None] * L)


def _laplace_rows(population, x, n_lo, n_hi):
    """-> (H (M, P, P) packed Hessians of the log posterior at x, [(pd, cov)] per neuron: laplace_glms' 'pd' and 'cov',
    the same algebra on the same Hessian).  The one place mass='laplace_dense' gets its covariances from."""
    from theano_pyglm_amd.inference.laplace import laplace_from_hessian
    H = population.compute_hessian_packed(x, n_lo, n_hi)
    rows = []
    for i in range(H.shape[0]):
        res = laplace_from_hessian(-0.5 * (H[i] + H[i].T), 0.0)
        rows.append((bool(res['pd']), res['cov']))
    return H, rows


def _laplace_dense_factor(population, x, n_lo, n_hi, floor):
    """W (M, P, P) for mass='laplace_dense' in the theta layout and dense_rows (M,): Sigma = the Laplace covariance where
    the Laplace result is positive definite (and factors), else W = diag(sqrt(minv)) with the 'laplace' rule's minv."""
    H, rows = _laplace_rows(population, x, n_lo, n_hi)
    M, P = H.shape[0], H.shape[1]
    pi = _theta_positions(population, x, n_lo, P)
    minv = _minv_from_hessian(H, pi, floor)
    W = np.zeros((M, P, P))
    dense = np.zeros(M, dtype=bool)
    for i, (pd, cov) in enumerate(rows):
        if pd:
            try:
                W[i] = factor_inverse_mass(np.asarray(cov)[np.ix_(pi, pi)])
                dense[i] = True
                continue
            except ValueError:
                pass
        W[i][np.diag_indices(P)] = np.sqrt(minv[i])
    return W, dense


def _laplace_dense_factor_device(population, x, n_lo, n_hi, floor):
    """_laplace_dense_factor with the factorisation on the device (laplace.laplace_on_device: one batched Cholesky and one
    triangular inverse give W directly, no covariance and no second factorisation): W stays there, a torch tensor (M, P, P)
    in the theta layout, and only dense_rows (M,) comes back.  Rows that are not positive definite get the 'laplace' rule."""
    import torch
    from theano_pyglm_amd.inference.laplace import laplace_on_device
    res, A, _, _ = laplace_on_device(population, x, n_lo, n_hi)
    W = res['W']
    dense = res['pd'] & torch.isfinite(W).all(dim=2).all(dim=1)
    d = torch.diagonal(A, dim1=1, dim2=2)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, floor))
    dense_h = dense.cpu().numpy()
    for m in np.flatnonzero(~dense_h):                         # (rare: the stack is touched only where a row failed)
        W[m] = torch.diag(torch.sqrt(1.0 / torch.clamp(d[m], min=floor)))
    return W, dense_h


def resolve_mass(population, x, mass, n_lo, n_hi, mass_floor, factor_on_device=False, dense='laplace'):
    """The mass= argument of the samplers for the rows [n_lo, n_hi) -> (minv, factor, dense_rows, setup_s): minv (M, P)
    positive inverse masses on the host or None; factor (M, P, P) lower-triangular W with W W^T = the inverse mass matrix
    (host array, or a device tensor with factor_on_device) or None; dense_rows (M,) bool with 'laplace_dense', else None;
    setup_s: the seconds spent on Hessians and factorisations.  dense='tempered' (annealed importance sampling, which
    builds one factor per temperature itself): 'laplace_dense' gives factor = 'tempered' and computes nothing.
    mass='adapt' (the chain learns a diagonal mass during its warm-up) gives minv = 'adapt' and setup_s = 0."""
    import time
    t0 = time.perf_counter()
    M, P = n_hi - n_lo, population.glm.P
    minv = factor = dense_rows = None
    if isinstance(mass, str):
        if mass == 'adapt':
            # learned by the chain itself during its warm-up (csrc/pglm_adapt.h): nothing to compute here
            if dense == 'tempered':
                raise ValueError("mass='adapt' is not available in annealed importance sampling: a mass that depends on "
                                 "the particles' states would invalidate the weights")
            if factor_on_device:
                raise ValueError("mass='adapt' builds no factor: factor_on_device does not apply")
            return 'adapt', None, None, 0
        elif mass == 'laplace':
            minv = _laplace_minv(population, x, n_lo, n_hi, float(mass_floor))
        elif mass == 'laplace_dense' and dense == 'tempered':
            factor = 'tempered'
        elif mass == 'laplace_dense':
            build = _laplace_dense_factor_device if factor_on_device else _laplace_dense_factor
            factor, dense_rows = build(population, x, n_lo, n_hi, float(mass_floor))
        else:
            raise ValueError("mass: None, 'laplace', 'laplace_dense', an (M, P) or an (M, P, P) array, or 'adapt'")
    elif mass is not None and np.ndim(mass) == 3:
        if np.shape(mass) != (M, P, P):
            raise ValueError("mass: an (M, P, P) = (%d, %d, %d) array of inverse mass matrices" % (M, P, P))
        factor = factor_inverse_mass(mass)
    else:
        minv = mass
    setup_s = time.perf_counter() - t0
    if minv is not None:
        minv = np.ascontiguousarray(minv, dtype=float)
        if minv.shape != (M, P) or not np.all(np.isfinite(minv)) or not np.all(minv > 0.0):
            raise ValueError("mass: an (M, P) = (%d, %d) array of positive inverse masses" % (M, P))
    return minv, factor, dense_rows, setup_s


def chain_starts(pk, x, n_lo, n_hi, n_chains, seed, init_jitter):
    """The starting points (n_chains M, P) of the chains, chain-major: x's rows, plus init_jitter * z with z the stateless
    normals of mass_adapt.start_jitter under the chain's seed."""
    from theano_pyglm_amd.inference.mass_adapt import chain_seed, start_jitter
    X0 = np.asarray(pk.pack(x, n_lo, n_hi), dtype=float)
    M, P = X0.shape
    X = np.tile(X0, (n_chains, 1))
    if init_jitter != 0.0:
        for c in range(n_chains):
            for m in range(M):
                X[c * M + m] += init_jitter * start_jitter(chain_seed(seed, c), n_lo + m, P)
    return X


def _check_chains(n_chains, init_jitter):
    n_chains, init_jitter = int(n_chains), float(init_jitter)
    if n_chains <= 0:
        raise ValueError("n_chains must be positive")
    if not np.isfinite(init_jitter) or init_jitter < 0.0:
        raise ValueError("init_jitter must be a finite number, not negative")
    return n_chains, init_jitter


def per_row(a, M, n_chains):
    """An (M, ...) array a neuron's chains share -> (n_chains M, ...), chain-major."""
    return a if n_chains == 1 else a.repeat(*([n_chains] + [1] * (a.dim() - 1)))


def split_chains(a, M, n_chains, axis):
    """The rows axis (n_chains M) of a result -> (n_chains, M) with the chain axis in front; n_chains = 1: unchanged."""
    if n_chains == 1:
        return a
    a = np.asarray(a)
    b = a.reshape(a.shape[:axis] + (n_chains, M) + a.shape[axis + 1:])
    return np.ascontiguousarray(np.moveaxis(b, axis, 0))


def sample_glms_hmc(population, x, n_samples, n_warmup=200, n_leapfrog=10, step_sz=0.1, thin=1, mass=None, seed=0,
                    n_lo=0, n_hi=None, mass_floor=1e-8, factor_on_device=False, n_chains=1, init_jitter=0.0, diagnostics=False,
                    filters=False):
    """Posterior samples of the parameter rows of neurons [n_lo, n_hi) given the rest of x, started at x.

    n_warmup transitions adapt every row's step size and are dropped; then n_samples * thin transitions, every thin-th
    kept.  step_sz: the starting step size, a number or one per row.  mass: None (identity), 'laplace' (minv = 1 /
    max(diag A, mass_floor), A = minus the Hessian of the log posterior at x: Population.compute_hessian_packed), an
    (M, P) array of inverse masses in the theta layout, an (M, P, P) array of inverse mass MATRICES Sigma in the theta
    layout (finite, symmetric, positive definite: factor_inverse_mass) or 'laplace_dense' (Sigma = the Laplace covariance
    A^-1 of every neuron, laplace_glms' 'cov'; a neuron whose A is not positive definite runs on the 'laplace' rule).
    mass='adapt': a diagonal mass learned by every row from its own warm-up draws in Stan's windows (mass_adapt.
    adapt_windows; the estimate, on the device, is csrc/pglm_adapt.h) -- no Hessian, no mode, one more small row launch per
    transition of the windows and no host synchronisation; with n_warmup < 20 there is no window and the chain is the
    mass=None chain.
    factor_on_device: with 'laplace_dense', the factor W of the Laplace covariance is built on the device
    (pgl_chol_factor_dev, pgl_tri_inverse_dev) and handed to the chain without a host copy; the default keeps the host
    factorisation, and with it the draws of earlier versions (the two W agree to rounding, not to the bit).
    n_chains = C > 1: C chains per neuron in the same launches (the state has C M rows; an evaluation is C pgl_ll_grad_dev,
    one per chain).  Chain c runs on the seed mass_adapt.chain_seed(seed, c) and equals the single-chain run with that
    seed; arrays given per neuron (step_sz, an (M, P) or (M, P, P) mass) are shared by a neuron's chains, 'adapt' learns
    one mass per chain.  All chains start at x, plus init_jitter * z (mass_adapt.start_jitter) when init_jitter > 0.
    Returns {'samples': (n_samples, M, P) rows in the theta layout [bias, w_stim, w_ir], 'accept_rate': (M,) after
    warm-up, 'step_sz': (M,) the frozen step sizes, 'n_evals': ll+grad launches} and, with 'laplace_dense', 'dense_rows':
    (M,) bool, the rows that run on the full covariance; with 'adapt', 'minv' (M, P) the learned inverse masses and
    'adapt_windows'.  With n_chains > 1 'samples', 'accept_rate', 'step_sz' and 'minv' gain a leading chain axis
    (summarize(samples, chains=True) takes them).  x is not changed.
    diagnostics=True (n_samples >= 8): the result gains 'summary', the convergence diagnostics of every parameter -- arrays
    (M, P) under the keys of diagnostics.chain_diagnostics plus 'route' -- computed by k_diag_column on the device tensor of
    the draws before it is copied (inference/diagnostics.py); the draws themselves are the same bits either way.
    filters=True (or a level in (0, 1); True: 0.95): the result gains 'filters', the posterior bands of the impulse responses
    and stimulus filters (inference/filters.py: filter_bands' dict), queued the same way (k_filter_bands).
    population.last_fit_stats records the launch counts, the host synchronisations inside the chain, 'mass' ('identity',
    'diagonal', 'adapted diagonal' or 'dense') and 'mass_setup_s' (the Hessian and the host factorisation; 0 for 'adapt')."""
    _check(population)
    n_samples, n_warmup, n_leapfrog, thin = int(n_samples), int(n_warmup), int(n_leapfrog), int(thin)
    if n_samples <= 0 or n_warmup < 0 or n_leapfrog <= 0 or thin <= 0:
        raise ValueError("n_samples, n_leapfrog and thin must be positive, n_warmup not negative")
    n_chains, init_jitter = _check_chains(n_chains, init_jitter)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    minv, factor, dense_rows, setup_s = resolve_mass(population, x, mass, n_lo, n_hi, mass_floor, factor_on_device)
    with session(population) as (torch, dev, stream, handles):
        out = _chain(population, torch, dev, stream, handles, x, n_samples, n_warmup, n_leapfrog, step_sz, thin, minv,
                     int(seed), n_lo, n_hi, M, factor, n_chains, init_jitter, bool(diagnostics), filters)
    if dense_rows is not None:
        out['dense_rows'] = dense_rows
    population.last_fit_stats['mass_setup_s'] = setup_s
    return out


def _chain(population, torch, dev, stream, handles, x, n_samples, n_warmup, n_leapfrog, step_sz, thin, mass, seed, n_lo, n_hi,
           M, factor=None, n_chains=1, init_jitter=0.0, diagnostics=False, filters=False):
    from theano_pyglm_amd.inference.mass_adapt import adapt_windows, schedule_ints
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    C, R = n_chains, n_chains * M                             # rows: chain c of neuron n_lo + m is row c M + m
    RP = R * P
    st = torch.zeros(h0.hmc_state_doubles(R, P), dtype=f64, device=dev)
    q = st[0:RP].view(R, P)
    sc = st[4 * RP:].view(NSCAL, R)
    q.copy_(torch.tensor(chain_starts(pk, x, n_lo, n_hi, C, seed, init_jitter), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    assert P == population.glm.P                              # (resolve_mass checked mass against it)
    adapt = isinstance(mass, str) and mass == 'adapt'
    windows, ad, sched = [], None, None
    if adapt:                                                 # ones: the identity chain until the first window ends
        minv = torch.ones((R, P), dtype=f64, device=dev)
        windows = adapt_windows(n_warmup)
        if windows:
            ad = torch.zeros(h0.adapt_state_doubles(R, P), dtype=f64, device=dev)
            sched = torch.tensor(schedule_ints(windows), dtype=torch.int32, device=dev)
    else:
        minv = per_row(torch.tensor(mass, dtype=f64, device=dev), M, C) if mass is not None else None
    step = np.ascontiguousarray(np.broadcast_to(np.asarray(step_sz, dtype=float), (M,)))
    if not np.all(step > 0.0):
        raise ValueError("step_sz must be positive")
    minv_ptr = minv.data_ptr() if minv is not None else 0
    Wd = None
    if factor is not None:                                    # (M, P, P) lower-triangular factors: uploaded once
        assert tuple(factor.shape) == (M, P, P)
        Wd = per_row(factor if torch.is_tensor(factor) else torch.tensor(factor, dtype=f64, device=dev), M, C)
    Xt = torch.empty((R, P), dtype=f64, device=dev)
    evaluate = RangeEvaluator(torch, dev, handles, Weff, M, P, n_lo, n_hi, C)
    samples = torch.empty((n_samples, R, P), dtype=f64, device=dev)
    counts = {'row': 0, 'adapt': 0, 'syncs': 0}

    def wait():
        counts['syncs'] += 1
        stream.synchronize()

    ll0, g0 = evaluate(q)
    h0.hmc_init_dev(st.data_ptr(), M, P, n_lo, ll0.data_ptr(), g0.data_ptr(), prm, float(step[0]), seed, n_chains=C)
    if np.any(step != step[0]):
        sc[SC_STEP].copy_(torch.tensor(np.tile(step, C), dtype=f64, device=dev))
    n_total = n_warmup + n_samples * thin
    syncs_before_chain = counts['syncs']
    evals_before_chain = evaluate.count
    for t in range(n_total):
        if Wd is not None:
            h0.hmc_dense_begin_dev(st.data_ptr(), R, P, Wd.data_ptr(), Xt.data_ptr())
        else:
            h0.hmc_begin_dev(st.data_ptr(), R, P, minv_ptr, Xt.data_ptr())
        counts['row'] += 1
        k = t - n_warmup
        keep = k >= 0 and (k + 1) % thin == 0
        for i in range(n_leapfrog):
            llt, gt = evaluate(Xt)
            last = i == n_leapfrog - 1
            out_ptr = samples[k // thin].data_ptr() if (last and keep) else 0
            if Wd is not None:
                h0.hmc_dense_leap_dev(st.data_ptr(), R, P, Wd.data_ptr(), llt.data_ptr(), gt.data_ptr(), prm, last,
                                      n_warmup, Xt.data_ptr(), out_ptr)
            else:
                h0.hmc_leap_dev(st.data_ptr(), R, P, minv_ptr, llt.data_ptr(), gt.data_ptr(), prm, last, n_warmup,
                                Xt.data_ptr(), out_ptr)
            counts['row'] += 1
        if windows and windows[0][0] <= t < windows[-1][1]:   # (the rows' window state is on the device; the host only
            h0.mass_adapt_dev(st.data_ptr(), R, P, ad.data_ptr(), sched.data_ptr(), minv_ptr)   # knows when none is open)
            counts['adapt'] += 1
    syncs_in_chain = counts['syncs'] - syncs_before_chain
    if diagnostics:                                           # on the draws where they lie, behind the last transition
        from theano_pyglm_amd.inference.diagnostics import queue_summary, finish_summary
        diag_rows = queue_summary(h0, samples, C)
    if filters:
        from theano_pyglm_amd.inference.filters import queue_bands, finish_bands, filters_level
        bands = queue_bands(population, h0, torch, samples, C, filters_level(filters))
    wait()
    sch = sc.cpu().numpy()
    out = {'samples': split_chains(samples.cpu().numpy(), M, C, 1),
           'accept_rate': split_chains(sch[SC_NACC] / float(n_samples * thin), M, C, 0),
           'step_sz': split_chains(sch[SC_STEP].copy(), M, C, 0), 'n_evals': evaluate.count}
    if adapt:
        out['minv'] = split_chains(minv.cpu().numpy(), M, C, 0)
        out['adapt_windows'] = windows
    if diagnostics:
        out['summary'] = finish_summary(diag_rows, out['samples'], C)
    if filters:
        out['filters'] = finish_bands(population, bands, samples, C, filters_level(filters))
    # ('row' counts the begin / leap CALLS of the C ABI; a dense call is three small launches, a diagonal one is one)
    population.last_fit_stats = {'sampler': 'lock-step HMC (hip row kernels)', 'transitions': n_total,
                                 'mass': 'dense' if Wd is not None else ('adapted diagonal' if adapt else
                                                                         ('diagonal' if minv is not None else 'identity')),
                                 'll_grad_launches': evaluate.count, 'row_launches': counts['row'],
                                 'evaluations_per_transition': (evaluate.count - evals_before_chain) / float(n_total),
                                 'row_launches_per_transition': counts['row'] / float(n_total),
                                 'host_syncs_in_chain': syncs_in_chain, 'host_syncs': counts['syncs']}
    if adapt:
        population.last_fit_stats['adapt_launches'] = counts['adapt']
    if C > 1:
        population.last_fit_stats['n_chains'] = C
    return out


# -- host-only helpers ---------------------------------------------------------------------------------------
def effective_sample_size(x):
    """Effective sample size of a scalar chain x (n,) by Geyer's initial positive sequence (Geyer 1992, "Practical Markov
    chain Monte Carlo", section 3.3): n / (-1 + 2 sum_k Gamma_k), Gamma_k = rho_{2k} + rho_{2k+1}, summed while positive.
    A constant chain has none: 0."""
    x = np.asarray(x, dtype=float)
    n = x.size
    xc = x - x.mean()
    var = xc.dot(xc) / n
    if n < 4 or not var > 0.0:
        return 0.0
    nfft = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(xc, nfft)
    rho = np.fft.irfft(f * np.conj(f), nfft)[:n] / (n * var)
    tau = -1.0
    for k in range(0, n - 1, 2):
        gam = rho[k] + rho[k + 1]
        if not gam > 0.0:
            break
        tau += 2.0 * gam
    return float(n / max(tau, 1.0 / n))


def summarize(samples, chains=False):
    """Per-parameter summary of samples (n, ...): dict of arrays shaped like one draw -- 'mean', 'sd' (n - 1), 'q025',
    'q975' and 'ess' (effective_sample_size).  chains=True: samples (n_chains, n, ...) as the samplers return them with
    n_chains > 1 -- the moments and quantiles of the pooled draws, 'ess' the sum of the chains' effective sample sizes, and
    'rhat' (mass_adapt.rhat: split-R-hat)."""
    s = np.asarray(samples, dtype=float)
    if chains:
        from theano_pyglm_amd.inference.mass_adapt import rhat
        if s.ndim < 2:
            raise ValueError("summarize(chains=True): samples (n_chains, n, ...)")
        out = summarize(s.reshape((s.shape[0] * s.shape[1],) + s.shape[2:]))
        out['ess'] = sum(summarize(c)['ess'] for c in s)
        out['rhat'] = rhat(s)
        return out
    n = s.shape[0]
    flat = s.reshape(n, -1)
    ess = np.array([effective_sample_size(flat[:, j]) for j in range(flat.shape[1])]).reshape(s.shape[1:])
    lo, hi = np.percentile(s, [2.5, 97.5], axis=0)
    return {'mean': s.mean(axis=0), 'sd': s.std(axis=0, ddof=1) if n > 1 else np.zeros(s.shape[1:]), 'q025': lo, 'q975': hi,
            'ess': ess}


def samples_to_states(population, x, samples, i, n_lo=0):
    """The x['glms'] list (deep copies) with the rows of draw i (samples (n, M, P), neurons n_lo ..) written in."""
    import copy
    s = np.asarray(samples, dtype=float)
    glms = copy.deepcopy(x['glms'])
    pk = _Packing(population, None)
    pk.unpack({'glms': glms}, s[i], n_lo, n_lo + s.shape[1])
    return glms
