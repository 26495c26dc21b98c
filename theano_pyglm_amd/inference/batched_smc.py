"""
Per-neuron marginal likelihood by an adaptive sequential Monte Carlo sampler (Del Moral, Doucet & Jasra 2006; the ladder
rule of Jasra et al. 2011 / Zhou, Johansen & Aston 2016) on the tempered path of inference/batched_ais.py, with the
particles resident on the GPU.

Annealed importance sampling walks a ladder guessed in advance and shared by all neurons, never removes a dead particle and
needs a pilot run for its step sizes.  Here every neuron chooses its next temperature from its own K particles -- the
largest step that keeps the conditional effective sample size at cess K (bisection on the device) -- so the weights
degrade by a set amount per stage; a particle set whose ESS falls below ess_min K is resampled (systematic, on the
device); and one step size per neuron is adapted from the acceptances of the neuron's whole population, stage by stage.
The rows, the kept parts (ll0, lp0, grad ll), the moves and the random numbers are those of annealed importance sampling
(csrc/pglm_ais.h); what couples the particles of a neuron is csrc/pglm_smc.h, run as HIP kernels (pgl_smc_*): one
workgroup per neuron for the stage, one per row for the gather and the change of target.  The moves are the AIS kernels'
bodies with a guard: a neuron that has reached beta = 1 is done and its rows are passed by, while the others go on.  The
host reads ONE number per stage, the count of unfinished neurons.

The estimate of Z from an adaptive SMC sampler is CONSISTENT (it converges as K grows), not unbiased as Neal's AIS
estimate is: the ladder and the resampling times depend on the particles.  No standard error comes from a single run --
variance estimation for adaptive-resampling SMC is not attempted here: repeat the run with other seeds and look at the
spread.

Served: the populations of ais_glms under the same Gaussian-prior condition.
"""
import numpy as np

from theano_pyglm_amd.inference import batched_ais as BA
from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.batched_hmc import _check, resolve_mass
from theano_pyglm_amd.inference.lockstep import session

# the per-neuron block (include/pyglm_hip.h): NSCAL (M) arrays, then NREC (S, M) records, then (R) anc, w, acc, (1) n_active
NSCAL, NREC = 10, 6
NS_BETA, NS_LOGZ, NS_STEP, NS_STAGE, NS_DONE, NS_NRES = 0, 1, 2, 3, 4, 5
REC_BETA, REC_ESS, REC_CESS, REC_RS, REC_ACC, REC_STEP = 0, 1, 2, 3, 4, 5


def smc_glms(population, x, n_particles=64, cess=0.9, ess_min=0.5, n_steps=1, n_leapfrog=10, step_sz=0.1, mass=None,
             max_stages=2000, delta_min=1e-6, seed=0, n_lo=0, n_hi=None, mass_floor=1e-8):
    """log Z_n of every neuron of [n_lo, n_hi) given the network of x, under the NORMALISED Gaussian priors, by adaptive
    sequential Monte Carlo with n_particles particles per neuron.

    cess: the conditional ESS, as a share of K, that every change of temperature keeps (closer to 1: more, smaller stages).
    ess_min: resampling when the ESS falls below ess_min K.  After every stage but a neuron's last, n_steps HMC transitions
    of n_leapfrog steps under the new target; step_sz is every neuron's first step, adapted afterwards from the accept
    rate of the neuron's particles towards 0.9.  delta_min: the smallest change of temperature (progress is guaranteed).
    mass: None, 'laplace' (evaluated at x), an (M, P) array of inverse masses, or 'laplace_dense', the tempered dense mass
    rebuilt after every stage from the neurons' OWN temperatures on the device: the lower factor of (beta_i G_i + Lambda)^-1
    (batched_ais.tempered_factor_rows).  An (M, P, P) array and 'adapt' raise ValueError.  The run stops when every neuron is
    done or after max_stages stages; a neuron that is not done by then has log_Z = NaN and finished = False.

    Returns a dict: 'log_Z', 'log_prior_norm', 'finished', 'n_stages', 'n_resampled' (M,); 'betas', 'ess' (before the
    stage's resampling), 'cess', 'resampled', 'accept_rate' (of the moves after the stage), 'step_sz' (they ran on), each
    (S, M), S the longest ladder, NaN (False) after a neuron's last stage; 'log_weights' (K, M), final and normalised over
    the particles; 'samples' (K, M, P), with the weights a weighted posterior sample; 'n_evals' (ll+grad launches);
    'idle_row_evaluations', the share of row evaluations spent on rows of done neurons; 'mass'.  The number comparable with
    laplace_glms' 'log_evidence' is log_Z + log_prior_norm.  No standard error: the estimate is consistent, not unbiased,
    and the variance of an adaptive-resampling sampler is not estimated from one run -- repeat with other seeds.
    population.last_fit_stats records the launches and the host reads (one per stage)."""
    _check(population)
    if isinstance(mass, str) and mass == 'adapt':
        raise ValueError("mass='adapt' is not available in sequential Monte Carlo: the step size is what adapts here")
    if mass is not None and not isinstance(mass, str) and np.ndim(mass) == 3:
        raise ValueError("sequential Monte Carlo takes no fixed (M, P, P) mass: 'laplace_dense' follows each neuron's "
                         "temperature")
    K, n_steps, n_leapfrog, max_stages = int(n_particles), int(n_steps), int(n_leapfrog), int(max_stages)
    if K <= 0 or n_steps <= 0 or n_leapfrog <= 0 or max_stages <= 0:
        raise ValueError("n_particles, n_steps, n_leapfrog and max_stages must be positive")
    cess, ess_min, delta_min, step_sz = float(cess), float(ess_min), float(delta_min), float(step_sz)
    if not (0.0 < cess < 1.0) or not (0.0 <= ess_min <= 1.0) or not (0.0 < delta_min <= 1.0) or not step_sz > 0.0:
        raise ValueError("cess in (0, 1), ess_min in [0, 1], delta_min in (0, 1], step_sz positive")
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    if _Packing(population, None).prior_params()[0] != 0:
        raise ValueError("sequential Monte Carlo starts from an exact prior draw: Gaussian impulse priors only "
                         "(group lasso is not served)")
    minv, factor, _, _ = resolve_mass(population, x, mass, n_lo, n_hi, mass_floor, dense='tempered')
    with session(population) as (torch, dev, stream, handles):
        return _run(population, torch, dev, stream, handles, x, K, cess, ess_min, n_steps, n_leapfrog, step_sz, minv,
                    factor is not None, max_stages, delta_min, int(seed), n_lo, n_hi, M, float(mass_floor))


def _run(population, torch, dev, stream, handles, x, K, cess, ess_min, n_steps, n_leapfrog, step0, mass, dense, S, delta_min,
         seed, n_lo, n_hi, M, mass_floor):
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    R = K * M
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    minv = torch.tensor(mass, dtype=f64, device=dev) if mass is not None else None
    minv_ptr = minv.data_ptr() if minv is not None else 0
    counts = {'ll_grad': 0, 'stage': 0, 'row': 0, 'syncs': 0, 'factor': 0, 'product': 0}
    st = torch.zeros(h0.ais_state_doubles(R, P), dtype=f64, device=dev)
    smc = torch.zeros(h0.smc_state_doubles(K, M, P, S), dtype=f64, device=dev)
    # (the layout this module reads the block by is the header's: the sizes must agree, or the library is another version's)
    if smc.numel() != NSCAL * M + NREC * S * M + 3 * R + 1 + 2 * R * P + 2 * R:
        raise RuntimeError("pgl_smc_state_doubles does not match the layout inference/batched_smc.py reads")
    Xt = torch.empty((R, P), dtype=f64, device=dev)
    bufs = [torch.empty(R * (1 + P), dtype=f64, device=dev) for _ in handles]
    sp, mp = st.data_ptr(), smc.data_ptr()
    n_active = smc[NSCAL * M + NREC * S * M + 3 * R:][:1]
    betas_dev = smc[NS_BETA * M:(NS_BETA + 1) * M]

    def evaluate():
        return BA.evaluate_particles(handles, bufs, Xt, Weff, K, M, P, n_lo, n_hi, counts)

    factor_now = None
    if dense:
        G = BA._ll_hessians(population, torch, dev, handles, x, n_lo, n_hi, P)
        lam = torch.tensor(BA.prior_precision(prm, population.N, pk.B, pk.nbk), dtype=f64, device=dev)
        eye = torch.eye(P, dtype=f64, device=dev)

        def chol(Ar):
            Ar = Ar.contiguous()
            return (Ar,) + h0.chol_factor(Ar)

        def tri_inv(Ls, info):
            h0.tri_inverse(Ls, info)
            return Ls

        def factor_now():
            W, _ = BA.tempered_factor_rows(G, lam, betas_dev, mass_floor, chol, tri_inv, torch, eye)
            counts['factor'] += 1
            return W.contiguous()

    h0.smc_init_dev(sp, mp, K, M, P, S, n_lo, prm, step0, seed, Xt.data_ptr())
    ll, g = evaluate()
    h0.ais_start_dev(sp, K, M, P, ll, g, prm)
    counts['row'] += 2
    idle_rows = 0
    stages = 0
    while stages < S:
        h0.smc_stage_dev(sp, mp, K, M, P, S, prm, n_steps, cess, ess_min, delta_min, seed)
        stages += 1
        counts['stage'] += 1
        counts['syncs'] += 1
        left = int(n_active.item())                           # the one host read of the stage
        if left == 0:
            break
        W = factor_now() if dense else None
        for _ in range(n_steps):
            if W is not None:
                h0.smc_dense_begin_dev(sp, mp, K, M, P, S, W.data_ptr(), Xt.data_ptr())
            else:
                h0.smc_begin_dev(sp, mp, K, M, P, S, minv_ptr, Xt.data_ptr())
            for i in range(n_leapfrog):
                ll, g = evaluate()
                if W is not None:
                    h0.smc_dense_leap_dev(sp, mp, K, M, P, S, W.data_ptr(), ll, g, prm, i == n_leapfrog - 1, Xt.data_ptr())
                else:
                    h0.smc_leap_dev(sp, mp, K, M, P, S, minv_ptr, ll, g, prm, i == n_leapfrog - 1, Xt.data_ptr())
            counts['row'] += 1 + n_leapfrog
            idle_rows += n_leapfrog * K * (M - left)
            if W is not None:
                counts['product'] += 2 * n_leapfrog + 1
    counts['syncs'] += 1
    stream.synchronize()
    sm = smc.cpu().numpy()
    ns = sm[:NSCAL * M].reshape(NSCAL, M)
    rec = sm[NSCAL * M:NSCAL * M + NREC * S * M].reshape(NREC, S, M)
    sch = st[BA.NVEC * R * P:].view(BA.NSCAL, R).cpu().numpy()
    fin = ns[NS_DONE] != 0.0
    n_st = ns[NS_STAGE].astype(int)
    Smax = int(n_st.max())
    lw = sch[BA.SC_LOGW].reshape(K, M).copy()
    top = np.max(lw, axis=0)
    ok = np.isfinite(top)
    with np.errstate(invalid='ignore', divide='ignore'):
        lw = lw - np.where(ok, top + np.log(np.sum(np.exp(lw - np.where(ok, top, 0.0)), axis=0)), 0.0)
    out = {'log_Z': np.where(fin, ns[NS_LOGZ], np.nan), 'finished': fin, 'n_stages': n_st,
           'n_resampled': ns[NS_NRES].astype(int),
           'log_prior_norm': np.full(M, BA.log_prior_norm(prm, population.N, pk.B, pk.nbk)),
           'betas': rec[REC_BETA, :Smax].copy(), 'ess': rec[REC_ESS, :Smax].copy(), 'cess': rec[REC_CESS, :Smax].copy(),
           'resampled': rec[REC_RS, :Smax] == 1.0, 'accept_rate': rec[REC_ACC, :Smax].copy(),
           'step_sz': rec[REC_STEP, :Smax].copy(), 'log_weights': lw,
           'samples': st[:R * P].view(K, M, P).cpu().numpy(), 'n_evals': counts['ll_grad'],
           'idle_row_evaluations': idle_rows / float(max(counts['ll_grad'] * M, 1)),
           'mass': 'laplace_dense' if dense else ('diagonal' if minv is not None else 'identity')}
    population.last_fit_stats = {'sampler': 'adaptive sequential Monte Carlo (hip row kernels)', 'particles': K,
                                 'stages': stages, 'll_grad_launches': counts['ll_grad'], 'stage_launches': 3 * counts['stage'],
                                 'row_launches': counts['row'], 'mass': out['mass'], 'factorisations': counts['factor'],
                                 'product_launches': counts['product'], 'host_reads': stages,
                                 'host_syncs': counts['syncs'], 'idle_row_evaluations': out['idle_row_evaluations']}
    return out
