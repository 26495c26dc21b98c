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

Served: exactly the populations of batched_newton_cg.supported (the packings whose per-neuron vector is the device's
theta row, under the priors the row kernels know).  Time-sharded populations are not (nothing is all-reduced).
"""
import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.batched_newton_cg import supported  # noqa: F401  (the served populations are the same)

# rows of the scalar block of the state (PglHmc, csrc/pglm_hmc.h)
SC_U0, SC_H0, SC_STEP, SC_AVG, SC_NACC, SC_T, SC_ACC = 0, 1, 2, 3, 4, 5, 6
NSCAL = 10

_STREAMS = {}


def _check(population):
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("lock-step HMC: the row kernels are not implemented for the %s packing" % bad)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("lock-step HMC does not run on a time-sharded population (set_time_shard): "
                         "evaluations are not all-reduced")


def _laplace_minv(population, x, n_lo, n_hi, floor):
    """1 / max(diag A, floor) in the theta layout, A = minus the Hessian of the log posterior at x."""
    from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars
    H = population.compute_hessian_packed(x, n_lo, n_hi)
    _, shapes = packdict(get_vars(population.glm_syms(), x['glms'][n_lo]))
    P = H.shape[1]
    pi = np.rint(population.glm.theta_row(unpackdict(np.arange(P, dtype=float), shapes))).astype(int)   # packed position of theta column
    d = -np.diagonal(H, axis1=1, axis2=2)[:, pi]
    d = np.where(np.isfinite(d), d, floor)
    return 1.0 / np.maximum(d, floor)


def sample_glms_hmc(population, x, n_samples, n_warmup=200, n_leapfrog=10, step_sz=0.1, thin=1, mass=None, seed=0,
                    n_lo=0, n_hi=None, mass_floor=1e-8):
    """Posterior samples of the parameter rows of neurons [n_lo, n_hi) given the rest of x, started at x.

    n_warmup transitions adapt every row's step size and are dropped; then n_samples * thin transitions, every thin-th
    kept.  step_sz: the starting step size, a number or one per row.  mass: None (identity), 'laplace' (minv = 1 /
    max(diag A, mass_floor), A = minus the Hessian of the log posterior at x: Population.compute_hessian_packed) or an
    (M, P) array of inverse masses in the theta layout.
    Returns {'samples': (n_samples, M, P) rows in the theta layout [bias, w_stim, w_ir], 'accept_rate': (M,) after
    warm-up, 'step_sz': (M,) the frozen step sizes, 'n_evals': ll+grad launches}.  x is not changed.
    population.last_fit_stats records the launch counts and the host synchronisations inside the chain."""
    _check(population)
    n_samples, n_warmup, n_leapfrog, thin = int(n_samples), int(n_warmup), int(n_leapfrog), int(thin)
    if n_samples <= 0 or n_warmup < 0 or n_leapfrog <= 0 or thin <= 0:
        raise ValueError("n_samples, n_leapfrog and thin must be positive, n_warmup not negative")
    import torch
    N = population.N
    n_hi = N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    if isinstance(mass, str):
        if mass != 'laplace':
            raise ValueError("mass: None, 'laplace' or an (M, P) array")
        mass = _laplace_minv(population, x, n_lo, n_hi, float(mass_floor))
    dev = torch.device('cuda', population.device)
    handles = []
    for data in population.data_sequences:
        population.set_data(data)
        handles.append(population._handle(data))
    stream = _STREAMS.get(dev.index)
    if stream is None:
        stream = _STREAMS[dev.index] = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for h in handles:
        h.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            out = _chain(population, torch, dev, stream, handles, x, n_samples, n_warmup, n_leapfrog, step_sz, thin, mass,
                         int(seed), n_lo, n_hi, M)
    finally:
        try:
            stream.synchronize()
        except Exception:
            pass
        for h in handles:
            h.set_stream(None)
    return out


def _chain(population, torch, dev, stream, handles, x, n_samples, n_warmup, n_leapfrog, step_sz, thin, mass, seed, n_lo, n_hi,
           M):
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    MP = M * P
    st = torch.zeros(h0.hmc_state_doubles(M, P), dtype=f64, device=dev)
    q = st[0:MP].view(M, P)
    sc = st[4 * MP:].view(NSCAL, M)
    q.copy_(torch.tensor(pk.pack(x, n_lo, n_hi), dtype=f64, device=dev))
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    minv = None
    if mass is not None:
        mh = np.ascontiguousarray(mass, dtype=float)
        if mh.shape != (M, P) or not np.all(np.isfinite(mh)) or not np.all(mh > 0.0):
            raise ValueError("mass: an (M, P) = (%d, %d) array of positive inverse masses" % (M, P))
        minv = torch.tensor(mh, dtype=f64, device=dev)
    step = np.ascontiguousarray(np.broadcast_to(np.asarray(step_sz, dtype=float), (M,)))
    if not np.all(step > 0.0):
        raise ValueError("step_sz must be positive")
    minv_ptr = minv.data_ptr() if minv is not None else 0
    Xt = torch.empty((M, P), dtype=f64, device=dev)
    bufs = [torch.empty(M * (1 + P), dtype=f64, device=dev) for _ in handles]     # [ll | grad] per data sequence
    samples = torch.empty((n_samples, M, P), dtype=f64, device=dev)
    counts = {'ll_grad': 0, 'row': 0, 'syncs': 0}

    def wait():
        counts['syncs'] += 1
        stream.synchronize()

    def evaluate(Xe):
        tot = None
        for h, buf in zip(handles, bufs):
            h.ll_grad_dev(Xe.data_ptr(), Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), n_lo, n_hi)
            tot = buf if tot is None else tot.add_(buf)
        counts['ll_grad'] += 1
        return tot[:M], tot[M:]

    ll0, g0 = evaluate(q)
    h0.hmc_init_dev(st.data_ptr(), M, P, n_lo, ll0.data_ptr(), g0.data_ptr(), prm, float(step[0]), seed)
    if np.any(step != step[0]):
        sc[SC_STEP].copy_(torch.tensor(step, dtype=f64, device=dev))
    n_total = n_warmup + n_samples * thin
    syncs_before_chain = counts['syncs']
    evals_before_chain = counts['ll_grad']
    for t in range(n_total):
        h0.hmc_begin_dev(st.data_ptr(), M, P, minv_ptr, Xt.data_ptr())
        counts['row'] += 1
        k = t - n_warmup
        keep = k >= 0 and (k + 1) % thin == 0
        for i in range(n_leapfrog):
            llt, gt = evaluate(Xt)
            last = i == n_leapfrog - 1
            h0.hmc_leap_dev(st.data_ptr(), M, P, minv_ptr, llt.data_ptr(), gt.data_ptr(), prm, last, n_warmup, Xt.data_ptr(),
                            samples[k // thin].data_ptr() if (last and keep) else 0)
            counts['row'] += 1
    syncs_in_chain = counts['syncs'] - syncs_before_chain
    wait()
    sch = sc.cpu().numpy()
    out = {'samples': samples.cpu().numpy(), 'accept_rate': sch[SC_NACC] / float(n_samples * thin), 'step_sz': sch[SC_STEP].copy(),
           'n_evals': counts['ll_grad']}
    population.last_fit_stats = {'sampler': 'lock-step HMC (hip row kernels)', 'transitions': n_total,
                                 'll_grad_launches': counts['ll_grad'], 'row_launches': counts['row'],
                                 'evaluations_per_transition': (counts['ll_grad'] - evals_before_chain) / float(n_total),
                                 'row_launches_per_transition': counts['row'] / float(n_total),
                                 'host_syncs_in_chain': syncs_in_chain, 'host_syncs': counts['syncs']}
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


def summarize(samples):
    """Per-parameter summary of samples (n, ...): dict of arrays shaped like one draw -- 'mean', 'sd' (n - 1), 'q025',
    'q975' and 'ess' (effective_sample_size)."""
    s = np.asarray(samples, dtype=float)
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
