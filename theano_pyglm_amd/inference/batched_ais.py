"""
Per-neuron marginal likelihood by annealed importance sampling (AIS; Neal 2001) with the particles resident on the GPU.

Given the network (A, W) the evidence of the model factorises over neurons, so the result is one log Z_n per neuron,
conditional on the network, exactly as the Laplace evidence of inference/laplace.py is.  K particles of every neuron of a
range start at an exact draw from the (Gaussian) prior and walk a ladder 0 = beta_0 < ... < beta_J = 1 of tempered targets
prior x L^beta.  ONE pgl_ll_grad_dev evaluates a particle of all neurons for the price of one, so all chains advance in
lock step: a leapfrog step is K evaluations (one per particle block) and one row launch over all K M rows.  The
algorithm runs as HIP row kernels (pgl_ais_*, csrc/pglm_ais.h over csrc/pglm_hmc.h; one workgroup per row) on state that
never leaves the device; the whole run is enqueued without one host synchronisation.  PyTorch is plumbing (device memory,
the stream); no library kernel is on the path, except the sum over the data sequences of a population that has several.

Order of the weight update.  Neal's estimator weighs the point that was sampled under beta_{j-1} with
L^(beta_j - beta_{j-1}) and THEN moves it under beta_j; that is what runs here.  The reference
(pyglm/inference/parallel_ais.py) moves x under beta_j first and then weighs f_j(x) / f_{j-1}(x) at the moved point, which
is not Neal's estimator and is biased.

Step sizes.  AIS weights are valid only if every transition kernel is fixed in advance; a step size adapted from the
particle's own history is not.  So one pilot particle (a random stream of its own; its weights are discarded) runs the
ladder with the adapting rule of pgl_hmc_decide and its step after each temperature's moves is recorded per (temperature,
neuron); the K particles then run frozen on that table, which moves device to device.

The mass matrix of the moves is diagonal (mass=None, 'laplace' or an (M, P) array) or dense: an (M, P, P) array of fixed
inverse mass matrices, or 'laplace_dense', the TEMPERED dense mass.  The target changes along the ladder -- the prior at
beta = 0, the posterior at beta = 1 -- and a mass fitted to the posterior is far too narrow for the first temperatures.  The
priors are Gaussian, so their precision Lambda is a known diagonal; with G = minus the Hessian of ll at x the Gaussian
approximation of the target at beta has precision A_beta = beta G + Lambda, and every temperature runs on the lower factor
W of A_beta^-1 (tempered_factor: one batched Cholesky factorisation and one triangular inverse on the device per
temperature).  The dense transition (csrc/pglm_ais_dense.h) runs in the whitened momentum r = W^T p; its two triangular
products per leapfrog step read a neuron's W once for all of the neuron's particles (pgl_tri_matvec_shared_dev).  A mass
that depends on beta but not on the particle's state keeps every transition valid for its target: the weights stay valid.

Served: the populations of batched_newton_cg.supported with Gaussian impulse priors (the start is an exact draw from the
normalised prior, which only the Gaussian form gives in closed form).  Not served: group lasso, the 'st' and Dirichlet
packings, time-sharded populations.
"""
import numpy as np

from theano_pyglm_amd.inference.batched_bfgs import _Packing
from theano_pyglm_amd.inference.batched_hmc import _check, _laplace_minv, resolve_mass  # noqa: F401  (_laplace_minv: what
#                                                                        mass='laplace' computes, for callers that freeze it)
from theano_pyglm_amd.inference.lockstep import session
from theano_pyglm_amd.inference.batched_newton_cg import supported  # noqa: F401  (the served populations: these, Gaussian)

# the state block (include/pyglm_hip.h): NVEC (R, P) arrays, then the rows of the scalar block (PglAis, csrc/pglm_ais.h)
NVEC, NSCAL = 6, 15
SC_STEP, SC_LOGW = 2, 13


def reference_ladder(n_temps):
    """The reference's ladder at n_temps points (parallel_ais.py:112): linspace(0, 0.01, n_temps/5) joined to
    logspace(-2, 0, 4 n_temps/5), duplicates removed."""
    n_temps = int(n_temps)
    if n_temps < 5:
        raise ValueError("n_temps must be at least 5")
    return np.unique(np.concatenate((np.linspace(0.0, 0.01, n_temps // 5), np.logspace(-2.0, 0.0, 4 * n_temps // 5))))


def check_ladder(betas):
    b = np.array(betas, dtype=float).reshape(-1)
    if b.size < 2 or b[0] != 0.0 or b[-1] != 1.0 or not np.all(np.diff(b) > 0.0):
        raise ValueError("betas: a ladder that starts at 0, ends at 1 and increases")
    return b


def weights_summary(log_weights):
    """log_weights (K, M) -> (log_Z (M,) = logsumexp_k - log K, log_Z_se (M,) = sd(w) / (mean(w) sqrt K), the delta-method
    standard error, ess (M,) = (sum w)^2 / sum w^2).  A dead particle (log w = -inf) counts in K with weight 0; a neuron
    whose particles are all dead has log_Z = -inf, se NaN, ess 0."""
    lw = np.asarray(log_weights, dtype=float)
    K = lw.shape[0]
    top = np.max(lw, axis=0)
    alive = np.isfinite(top)
    w = np.exp(lw - np.where(alive, top, 0.0))
    mean = w.mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        log_Z = np.where(alive, top + np.log(mean), -np.inf)
        se = np.where(alive, (w.std(axis=0, ddof=1) if K > 1 else np.full(mean.shape, np.nan)) / (mean * np.sqrt(K)), np.nan)
        ess = np.where(alive, w.sum(axis=0) ** 2 / np.sum(w * w, axis=0), 0.0)
    return log_Z, se, ess


def log_prior_norm(prm, N, B, Dstim):
    """sum_j log(sigma_j sqrt(2 pi)) over a row [bias, w_stim (Dstim), w_ir (N, B)]: the normalising constant the host
    priors drop.  prm: _Packing.prior_params()."""
    _, _, sg_b, stim_sigma, _, sigma, _ = prm
    return (np.log(sg_b) + (Dstim * np.log(stim_sigma) if Dstim else 0.0) + N * B * np.log(sigma) +
            0.5 * (1 + Dstim + N * B) * np.log(2.0 * np.pi))


def prior_precision(prm, N, B, Dstim):
    """The diagonal of Lambda, the precision of the Gaussian priors, over a row [bias, w_stim (Dstim), w_ir (N, B)]: (P,).
    prm: _Packing.prior_params()."""
    _, _, sg_b, stim_sigma, _, sigma, _ = prm
    sd = np.concatenate(([sg_b], np.full(Dstim, stim_sigma), np.full(N * B, sigma))).astype(float)
    return 1.0 / (sd * sd)


def tempered_factor(G, lam, beta, floor, factor, inverse, xp, eye):
    """The factor of the tempered mass on any backend.  G (M, P, P): minus the Hessians of ll in the theta layout, lam (P,)
    the diagonal of Lambda, eye the (P, P) identity (xp arrays: numpy, or torch tensors on the device); factor, inverse:
    laplace_from_factor's.  A = beta G + Lambda; W (M, P, P) lower triangular with W W^T = A^-1 by the route of
    laplace.laplace_from_factor (the index reversal, ONE factorisation, ONE triangular inverse, the scales put back).  A row
    whose A does not factor (info != 0) gets W = diag(1 / sqrt(max(diag A, floor))), a non-finite diagonal entry counting as
    floor: the 'laplace' rule.  Nothing is read back: the choice is made where the arrays live.  At beta = 0 A is the
    diagonal Lambda and W = Lambda^-1/2 exactly: nothing is factored.
    Returns (W, info (M,): 0 where A factored); the strict upper triangle of W is 0."""
    from theano_pyglm_amd.inference.laplace import laplace_from_factor
    if beta == 0.0:
        return xp.zeros_like(G) + (1.0 / xp.sqrt(lam))[None, :, None] * eye[None], xp.zeros_like(lam[:1]).repeat(G.shape[0])
    A = beta * G + lam[None, :, None] * eye[None]
    res = laplace_from_factor(A, factor, inverse, xp)
    d = beta * xp.diagonal(G, 0, 1, 2) + lam[None]
    d = xp.where(xp.isfinite(d), d, xp.full_like(d, floor))
    fb = 1.0 / xp.sqrt(xp.where(d > floor, d, xp.full_like(d, floor)))
    bad = res['info'] != 0
    return xp.where(bad[:, None, None], fb[:, :, None] * eye[None], res['W']), res['info']


def _ll_hessians(population, torch, dev, handles, x, n_lo, n_hi, P):
    """G (M, P, P) = minus the sum over the data sequences of the Hessian of ll at x, rows [n_lo, n_hi), on the device in
    the theta layout -- computed as laplace.laplace_on_device computes it (hvp_prepare + hess per sequence, summed where
    pgl_hess_dev leaves them).  Queued on the current stream; nothing is read back."""
    f64 = torch.float64
    M = n_hi - n_lo
    theta = torch.tensor(population.theta_matrix(x, n_lo, n_hi), dtype=f64, device=dev)
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    G = torch.zeros((M, P, P), dtype=f64, device=dev)
    buf = torch.empty((M, P, P), dtype=f64, device=dev)
    for h in handles:
        h.hvp_prepare(theta.data_ptr(), Weff.data_ptr(), n_lo, n_hi)
        h.hess(buf.data_ptr(), P)
        G.sub_(buf)
    return G


def tempered_factor_rows(G, lam, betas, floor, factor, inverse, xp, eye):
    """tempered_factor with one temperature per ROW: betas (M,) on G's backend (a device vector is never read back).
    A_i = betas_i G_i + Lambda, W_i W_i^T = A_i^-1 by the same route, the same fall-back for a row that does not factor.  A
    row at beta = 0 goes through the factorisation of the diagonal Lambda like any other (W = Lambda^-1/2 within 2 ulp).
    Returns (W, info (M,))."""
    from theano_pyglm_amd.inference.laplace import laplace_from_factor
    b = betas[:, None, None]
    A = b * G + lam[None, :, None] * eye[None]
    res = laplace_from_factor(A, factor, inverse, xp)
    d = betas[:, None] * xp.diagonal(G, 0, 1, 2) + lam[None]
    d = xp.where(xp.isfinite(d), d, xp.full_like(d, floor))
    fb = 1.0 / xp.sqrt(xp.where(d > floor, d, xp.full_like(d, floor)))
    bad = res['info'] != 0
    return xp.where(bad[:, None, None], fb[:, :, None] * eye[None], res['W']), res['info']


def evaluate_particles(handles, bufs, Xt, Weff, K, M, P, n_lo, n_hi, counts):
    """ll and its gradient of all K M rows of Xt (particle-major): one pgl_ll_grad_dev per particle block -- the (M, P) block
    of rows k M .. -- and data sequence into that sequence's [ll (R) | grad (R, P)] buffer, summed into the first.
    counts['ll_grad'] += K.  -> (pointer to ll, pointer to grad).  The loop annealed importance sampling and sequential
    Monte Carlo share."""
    R = K * M
    for h, buf in zip(handles, bufs):
        for k in range(K):
            h.ll_grad_dev(Xt[k * M].data_ptr(), Weff.data_ptr(), buf[k * M:].data_ptr(),
                          buf[R + k * M * P:].data_ptr(), n_lo, n_hi)
        if buf is not bufs[0]:
            bufs[0].add_(buf)
    counts['ll_grad'] += K
    return bufs[0].data_ptr(), bufs[0][R:].data_ptr()


def ais_glms(population, x, n_particles=16, betas=None, n_temps=200, n_steps=1, n_leapfrog=10, step_sz=0.1, pilot=True,
             mass=None, seed=0, particle0=0, n_lo=0, n_hi=None, mass_floor=1e-8):
    """log Z_n = log of the integral of L_n(theta) prior(theta) over the parameter row (bias, w_stim, w_ir) of every neuron
    of [n_lo, n_hi), given the network of x, under the NORMALISED Gaussian priors.

    betas: the ladder (starts at 0, ends at 1, increases); None: reference_ladder(n_temps).  At every temperature but the
    last, n_steps HMC transitions of n_leapfrog steps.  mass: as sample_glms_hmc -- None, 'laplace' (evaluated at x), an
    (M, P) array of inverse masses, an (M, P, P) array of inverse mass MATRICES Sigma in the theta layout (finite, symmetric,
    positive definite: factor_inverse_mass; the same at every temperature) or 'laplace_dense', the tempered dense mass:
    at temperature beta_j the lower factor W_j of (beta_j G + Lambda)^-1, G = minus the Hessian of ll at x, Lambda the
    priors' precision (tempered_factor).  A row whose matrix does not factor at a temperature runs there on the 'laplace'
    rule, diag(1 / sqrt(max(diag, mass_floor))).  All particles of a neuron share the mass; the pilot uses the same W_j.
    The W_j are RECOMPUTED for the main run, not kept from the pilot's: kept they are (J-1) M P^2 8 bytes (20 GB at N = 128,
    P = 641 with 49 temperatures), recomputed they cost one factorisation and one inverse per temperature (about 15 ms
    there, beside about a second of evaluations), and the same inputs give the same bits both times.  pilot: find the (J-1, M) step table with one
    adapting pilot particle started at step_sz (a number); False: step_sz, a number or a (J-1, M) table, is the table.
    Particles are numbered particle0 .. particle0 + n_particles - 1: runs with different ranges and the same seed are
    independent particles of one larger run.  x supplies the network (and the point of the Hessian for mass='laplace'); it
    is not changed.  mass='adapt' (the samplers' warm-up adaptation) raises ValueError: a mass that depends on the states
    of the particles would invalidate the weights.

    Returns a dict: 'log_Z' (M,), 'log_Z_se' (M,), 'ess' (M,) (weights_summary), 'log_weights' (K, M), 'samples'
    (K, M, P) the final points, 'accept_rate' (J-1, M), 'step_sz' (J-1, M), 'betas', 'log_prior_norm' (M,), 'n_evals'
    (ll+grad launches), 'mass' (the form used: 'identity', 'diagonal', 'dense' or 'laplace_dense') and, with
    'laplace_dense', 'dense_rows' (J-1, M) bool: the rows that ran on the full factor at each temperature.  The host priors -- and with them laplace_glms -- drop the priors' normalising constants: the number
    comparable with laplace_glms' 'log_evidence' is log_Z + log_prior_norm.
    population.last_fit_stats records the launch counts -- with a dense mass also 'factorisations' (tempered_factor calls)
    and 'product_launches' (pgl_tri_matvec_shared launches) -- and the host synchronisations inside the run (none)."""
    _check(population)
    if isinstance(mass, str) and mass == 'adapt':
        raise ValueError("mass='adapt' is not available in annealed importance sampling: a mass that depends on the "
                         "particles' states would invalidate the weights")
    K, n_steps, n_leapfrog = int(n_particles), int(n_steps), int(n_leapfrog)
    if K <= 0 or n_steps <= 0 or n_leapfrog <= 0 or int(particle0) < 0:
        raise ValueError("n_particles, n_steps and n_leapfrog must be positive, particle0 not negative")
    betas = reference_ladder(n_temps) if betas is None else check_ladder(betas)
    n_hi = population.N if n_hi is None else n_hi
    M = n_hi - n_lo
    if M <= 0:
        raise ValueError("empty neuron range")
    if _Packing(population, None).prior_params()[0] != 0:
        raise ValueError("annealed importance sampling starts from an exact prior draw: Gaussian impulse priors only "
                         "(group lasso is not served)")
    minv, factor, _, _ = resolve_mass(population, x, mass, n_lo, n_hi, mass_floor, dense='tempered')
    with session(population) as (torch, dev, stream, handles):
        return _run(population, torch, dev, stream, handles, x, K, betas, n_steps, n_leapfrog, step_sz, bool(pilot), minv,
                    int(seed), int(particle0), n_lo, n_hi, M, factor, float(mass_floor))


def _run(population, torch, dev, stream, handles, x, K, betas, n_steps, n_leapfrog, step_sz, pilot, mass, seed, particle0,
         n_lo, n_hi, M, factor=None, mass_floor=1e-8):
    pk = _Packing(population, torch, handles, (n_lo, n_hi))
    assert pk.identity                                        # (hvp_packing() is None: the row IS the theta row)
    h0 = handles[0]
    P = pk.Pp
    prm = pk.prior_params()
    f64 = torch.float64
    J = betas.size - 1
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
    assert P == population.glm.P                              # (resolve_mass checked mass against it)
    minv = torch.tensor(mass, dtype=f64, device=dev) if mass is not None else None
    minv_ptr = minv.data_ptr() if minv is not None else 0
    if pilot:
        step0 = float(step_sz)
        table = None
    else:
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(step_sz, dtype=float), (J - 1, M)))
        step0 = float(th.flat[0]) if th.size else 0.1
        table = torch.tensor(th, dtype=f64, device=dev)
    if not step0 > 0.0 or (table is not None and not bool(np.all(th > 0.0))):
        raise ValueError("step_sz must be positive")
    counts = {'ll_grad': 0, 'row': 0, 'syncs': 0, 'factor': 0, 'product': 0}

    def wait():
        counts['syncs'] += 1
        stream.synchronize()

    # the dense forms: factor_at(j) -> W (M, P, P) on the device for the moves at betas[j] (None: the diagonal forms)
    factor_at = dense_rows = None
    if isinstance(factor, str):                               # 'laplace_dense': one factor per temperature, recomputed per run
        G = _ll_hessians(population, torch, dev, handles, x, n_lo, n_hi, P)
        lam = torch.tensor(prior_precision(prm, population.N, pk.B, pk.nbk), dtype=f64, device=dev)
        eye = torch.eye(P, dtype=f64, device=dev)
        dense_rows = torch.zeros((max(J - 1, 1), M), dtype=torch.bool, device=dev)

        def chol(Ar):
            Ar = Ar.contiguous()
            return (Ar,) + h0.chol_factor(Ar)

        def tri_inv(Ls, info):
            h0.tri_inverse(Ls, info)
            return Ls

        def factor_at(j):
            W, info = tempered_factor(G, lam, float(betas[j]), mass_floor, chol, tri_inv, torch, eye)
            dense_rows[j - 1] = info == 0
            counts['factor'] += 1
            return W.contiguous()
    elif factor is not None:                                  # (M, P, P) lower-triangular factors: uploaded once
        assert tuple(factor.shape) == (M, P, P)
        Wfix = torch.tensor(factor, dtype=f64, device=dev)

        def factor_at(j):
            return Wfix

    def ladder(Kr, part0, adapt, table):
        """One run of Kr particles over the whole ladder -> (state block, accept counts (J-1, R), steps (J-1, R) or None)."""
        R = Kr * M
        st = torch.zeros(h0.ais_state_doubles(R, P), dtype=f64, device=dev)
        Xt = torch.empty((R, P), dtype=f64, device=dev)
        bufs = [torch.empty(R * (1 + P), dtype=f64, device=dev) for _ in handles]     # [ll | grad] per data sequence
        acc = torch.zeros((max(J - 1, 1), R), dtype=f64, device=dev)
        steps = torch.zeros((max(J - 1, 1), R), dtype=f64, device=dev) if adapt else None
        sp = st.data_ptr()

        def evaluate():
            return evaluate_particles(handles, bufs, Xt, Weff, Kr, M, P, n_lo, n_hi, counts)

        h0.ais_init_dev(sp, Kr, M, P, n_lo, part0, prm, step0, seed, Xt.data_ptr())
        ll, g = evaluate()
        h0.ais_start_dev(sp, Kr, M, P, ll, g, prm)
        counts['row'] += 2
        for j in range(1, J + 1):
            h0.ais_temper_dev(sp, Kr, M, P, prm, betas[j], table[j - 1].data_ptr() if (table is not None and j < J) else 0)
            counts['row'] += 1
            if j == J:
                break
            Wj = factor_at(j) if factor_at is not None else None
            for _ in range(n_steps):
                if Wj is not None:
                    h0.ais_dense_begin_dev(sp, Kr, M, P, Wj.data_ptr(), Xt.data_ptr())
                else:
                    h0.ais_begin_dev(sp, Kr, M, P, minv_ptr, Xt.data_ptr())
                for i in range(n_leapfrog):
                    ll, g = evaluate()
                    if Wj is not None:
                        h0.ais_dense_leap_dev(sp, Kr, M, P, Wj.data_ptr(), ll, g, prm, i == n_leapfrog - 1, adapt,
                                              Xt.data_ptr(), acc[j - 1].data_ptr(), steps[j - 1].data_ptr() if adapt else 0)
                    else:
                        h0.ais_leap_dev(sp, Kr, M, P, minv_ptr, ll, g, prm, i == n_leapfrog - 1, adapt, Xt.data_ptr(),
                                        acc[j - 1].data_ptr(), steps[j - 1].data_ptr() if adapt else 0)
                # ('row' counts the begin / leap CALLS of the C ABI; a dense call is three small launches, two of them
                # products but for the last leap's one; a diagonal call is one launch)
                counts['row'] += 1 + n_leapfrog
                if Wj is not None:
                    counts['product'] += 2 * n_leapfrog + 1
        return st, acc, steps

    if pilot and J > 1:
        _, _, table = ladder(1, -1, True, None)               # (J-1, M): stays on the device
    st, acc, _ = ladder(K, particle0, False, table if J > 1 else None)
    syncs_in_run = counts['syncs']
    wait()
    R = K * M
    sch = st[NVEC * R * P:].view(NSCAL, R).cpu().numpy()
    lw = sch[SC_LOGW].reshape(K, M).copy()
    log_Z, se, ess = weights_summary(lw)
    Dstim = pk.nbk
    out = {'log_Z': log_Z, 'log_Z_se': se, 'ess': ess, 'log_weights': lw,
           'samples': st[:R * P].view(K, M, P).cpu().numpy(),
           'accept_rate': acc[:J - 1].view(J - 1, K, M).sum(dim=1).cpu().numpy() / float(K * n_steps),
           'step_sz': table.cpu().numpy() if J > 1 else np.zeros((0, M)), 'betas': betas,
           'log_prior_norm': np.full(M, log_prior_norm(prm, population.N, pk.B, Dstim)), 'n_evals': counts['ll_grad'],
           'mass': ('laplace_dense' if isinstance(factor, str) else 'dense') if factor is not None else
                   ('diagonal' if minv is not None else 'identity')}
    if dense_rows is not None:
        out['dense_rows'] = dense_rows[:J - 1].cpu().numpy()
    population.last_fit_stats = {'sampler': 'annealed importance sampling (hip row kernels)', 'particles': K, 'pilot': int(pilot and J > 1),
                                 'temperatures': J, 'll_grad_launches': counts['ll_grad'], 'row_launches': counts['row'],
                                 'mass': out['mass'], 'factorisations': counts['factor'], 'product_launches': counts['product'],
                                 'host_syncs_in_run': syncs_in_run, 'host_syncs': counts['syncs']}
    return out
