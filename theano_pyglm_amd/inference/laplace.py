"""
Laplace approximation of the per-neuron posterior at a MAP estimate.

Given the other neurons' parameters and the network, the log posterior of neuron n's packed GLM parameters theta_n is
log_prior_n + sum_data ll_n (what fit_glm maximises, coord_descent.py:161-204).  Around its mode theta_hat

    log p(theta) ~ log p(theta_hat) - 1/2 (theta - theta_hat)^T A (theta - theta_hat),   A = -Hessian at theta_hat

so the posterior is approximately N(theta_hat, A^-1): standard errors sqrt(diag A^-1) and the evidence

    log Z_n ~ log p(theta_hat) + (P / 2) log 2 pi - 1/2 log det A

which compares models (e.g. values of the group-lasso `lam`) without held-out data.  The dense Hessian comes from the
device (Population.compute_hessian_packed: one Gram contraction per data sequence), the P x P factorisation runs on the
host (P <= 1 221 at the shapes the library serves) or, with laplace_glms(device=True), on the device as well: a batched
equilibrated Cholesky factorisation and a triangular inverse (pgl_chol_factor_dev, pgl_tri_inverse_dev), one workgroup
per neuron, from which every output follows without a covariance or a second factorisation (laplace_from_factor).  The reference builds the same matrix with hessian_wrt_list
(pyglm/utils/grads.py:30-66) for its Newton fit and has no Laplace step of its own.
"""
import numpy as np

from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars


def laplace_from_hessian(A, log_post):
    """The Laplace algebra for one mode: A (P, P) = minus the Hessian of the log posterior there, log_post its value.
    Returns a dict: 'A'; 'pd' (A is positive definite: its Cholesky factorisation exists); 'chol' (lower factor), 'cov' =
    A^-1, 'stderr_vec' = sqrt(diag cov), 'log_evidence'.  Where A is not positive definite (not a mode, or a flat
    direction) the factor, covariance, standard errors and evidence are NaN."""
    A = np.asarray(A, dtype=float)
    P = A.shape[0]
    out = {'A': A, 'pd': False, 'chol': np.full((P, P), np.nan), 'cov': np.full((P, P), np.nan),
           'stderr_vec': np.full(P, np.nan), 'log_evidence': np.nan}
    if not np.all(np.isfinite(A)) or not np.all(np.diag(A) > 0.0):
        return out
    # the factorisation runs on the equilibrated matrix D^-1/2 A D^-1/2, D = diag A: at a group-lasso optimum the groups
    # shrunk to (almost) zero carry curvatures ~ 1 / |w_g| many orders of magnitude above the rest, a scaling that costs
    # an unscaled factorisation all of its digits and this one none
    s = 1.0 / np.sqrt(np.diag(A))
    try:
        Ls = np.linalg.cholesky(A * s[:, None] * s[None, :])
    except np.linalg.LinAlgError:
        return out
    sign, logdet = np.linalg.slogdet(A)
    if not (sign > 0 and np.isfinite(logdet)):
        return out
    Linv = np.linalg.solve(Ls, np.eye(P)) * s[None, :]        # (D^1/2 Ls)^-1
    cov = Linv.T.dot(Linv)
    out.update(pd=True, chol=Ls / s[:, None], cov=cov, stderr_vec=np.sqrt(np.diag(cov)),
               log_evidence=float(log_post) + 0.5 * P * np.log(2.0 * np.pi) - 0.5 * logdet)
    return out


# -- the same posterior from ONE factorisation and ONE triangular inverse ------------------------------------------------
# With A_t = A in the theta layout (the device's) and J the index reversal, factor the reversed matrix, J A_t J = F F^T, F lower
# triangular.  Then W = J F^-T J is lower triangular with a positive diagonal and W W^T = A_t^-1: by uniqueness of the
# Cholesky factor W is batched_hmc.factor_inverse_mass of the Laplace covariance in the theta layout -- the factor of the
# inverse mass matrix the dense-mass chain runs on -- the standard errors are the row norms of W and log det A = 2 sum log
# F_ii.  No covariance is formed and nothing is factored twice.  F comes equilibrated, F = D^1/2 Ls with D = diag(J A_t J),
# so W = J D^-1/2 Ls^-T J.
def laplace_from_factor(A_theta, factor, inverse, xp, cov=False):
    """The Laplace algebra for a stack of modes on any backend.  A_theta (M, P, P): minus the Hessians in the theta layout
    (xp arrays: numpy, or torch tensors on the device).  factor(Ar) -> (Ls, scale, logdet, info) for a fresh contiguous stack
    Ar (it may work in place): the lower triangle of Ls[m] is the Cholesky factor of Ar[m] scaled to a unit diagonal, scale
    (M, P) = sqrt(diag Ar), logdet (M,) = log det Ar[m], info (M,) = 0 or the first failing column + 1 (then the row's Ls,
    scale and logdet are NaN).  inverse(Ls, info) -> X, the lower triangle of X[m] = Ls[m]^-1, rows with info != 0 left NaN.
    Returns a dict of xp arrays: 'W' (M, P, P) lower triangular with W W^T = A_theta^-1 (strict upper triangle exactly 0),
    'stderr' (M, P) = sqrt(diag A_theta^-1) in the theta layout, 'logdet', 'info', 'pd' (M,) = (info == 0) and, with cov,
    'cov' = W W^T.  Failed rows are NaN."""
    Ls, scale, logdet, info = factor(xp.flip(A_theta, (1, 2)))
    X = inverse(Ls, info)
    W = xp.flip(xp.swapaxes(xp.tril(X), 1, 2) / scale[:, :, None], (1, 2))
    out = {'W': W, 'stderr': xp.sqrt((W * W).sum(2)), 'logdet': logdet, 'info': info, 'pd': info == 0}
    if cov:
        out['cov'] = xp.matmul(W, xp.swapaxes(W, 1, 2))
    return out


def _first_failing_minor(C):
    """k + 1 for the first column k at which the Cholesky factorisation of C stops."""
    for k in range(1, C.shape[0] + 1):
        try:
            if not np.all(np.isfinite(np.linalg.cholesky(C[:k, :k]))):
                return k
        except np.linalg.LinAlgError:
            return k
    return C.shape[0]


def numpy_factor(Ar):
    """laplace_from_factor's `factor` on the host: np.linalg.cholesky of the equilibrated matrix, lower triangle read only."""
    Ar = np.array(Ar, dtype=float)
    M, P = Ar.shape[0], Ar.shape[1]
    scale, logdet, info = np.full((M, P), np.nan), np.full(M, np.nan), np.zeros(M, dtype=np.int32)
    for m in range(M):
        low = np.tril(Ar[m])
        d = np.diag(low).copy()
        bad = ~(np.isfinite(low).all(axis=1) & (d > 0.0))
        if np.any(bad):
            info[m] = int(np.argmax(bad)) + 1
        else:
            s = 1.0 / np.sqrt(d)
            C = (low + np.tril(low, -1).T) * s[:, None] * s[None, :]
            try:
                L = np.linalg.cholesky(C)
            except np.linalg.LinAlgError:
                L = None
            if L is None or not np.all(np.isfinite(L)):
                info[m] = _first_failing_minor(C)
            else:
                Ar[m][np.tril_indices(P)] = L[np.tril_indices(P)]
                scale[m] = np.sqrt(d)
                logdet[m] = 2.0 * np.sum(np.log(np.diag(L))) + np.sum(np.log(d))
        if info[m] != 0:
            Ar[m][np.tril_indices(P)] = np.nan
    return Ar, scale, logdet, info


def numpy_inverse(Ls, info):
    """laplace_from_factor's `inverse` on the host: forward substitution against the identity."""
    from scipy.linalg import solve_triangular
    P = Ls.shape[1]
    for m in range(Ls.shape[0]):
        if info[m] == 0:
            Ls[m][np.tril_indices(P)] = solve_triangular(Ls[m], np.eye(P), lower=True)[np.tril_indices(P)]
    return Ls


def theta_positions(population, x, n_lo):
    """(pi, shapes): the packed position of every theta column (Population.compute_hessian_packed's check) and the shapes
    that unpack a packed vector."""
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("Hessian-vector products are not implemented for the %s packing" % bad)
    w0, shapes = packdict(get_vars(population.glm_syms(), x['glms'][n_lo]))
    P = w0.size
    pi = np.rint(population.glm.theta_row(unpackdict(np.arange(P, dtype=float), shapes))).astype(int)
    if P != population.glm.P or not np.array_equal(np.sort(pi), np.arange(P)):
        raise ValueError("the packed vector is not a permutation of the theta row")
    return pi, shapes


_STREAMS = {}


def laplace_on_device(population, x, n_lo=0, n_hi=None, cov=False, timings=None):
    """laplace_from_factor on the device for the neurons [n_lo, n_hi) at x: the Hessians of ll of every data sequence are
    summed where pgl_hess_dev leaves them, the priors' Hessians (glm.hess_log_prior, host) are permuted to the theta layout
    and added, pgl_chol_factor_dev and pgl_tri_inverse_dev run on the reversed stack.  Returns (res, A, pi, shapes): res =
    laplace_from_factor's dict of device tensors, A (M, P, P) the device stack of minus the Hessians in the theta layout.
    timings: a dict that receives the seconds of the stages 'hessian', 'factor', 'inverse' (each behind a synchronisation;
    without it the stages are queued back to back)."""
    import time
    import torch
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("laplace_glms does not run on a time-sharded population (set_time_shard): "
                         "the Hessians are not all-reduced")
    n_hi = population.N if n_hi is None else n_hi
    if n_hi <= n_lo:
        raise ValueError("empty neuron range")
    pi, shapes = theta_positions(population, x, n_lo)
    M, P = n_hi - n_lo, pi.size
    dev = torch.device('cuda', population.device)
    f64 = torch.float64
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
    def lap(name, t0):
        # (a stage time needs a synchronisation: only where the caller asked for timings)
        if timings is None:
            return t0
        stream.synchronize()
        timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    try:
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            theta = torch.tensor(population.theta_matrix(x, n_lo, n_hi), dtype=f64, device=dev)
            Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)
            pid = torch.tensor(pi, dtype=torch.long, device=dev)
            # the priors: packed on the host, H_theta[a, b] = H_packed[pi[a], pi[b]]
            Hp = np.stack([population.glm.hess_log_prior(x['glms'][n]) for n in range(n_lo, n_hi)])
            A = torch.tensor(Hp, dtype=f64, device=dev)[:, pid[:, None], pid[None, :]].contiguous()
            buf = torch.empty((M, P, P), dtype=f64, device=dev)
            for h in handles:
                h.hvp_prepare(theta.data_ptr(), Weff.data_ptr(), n_lo, n_hi)
                h.hess(buf.data_ptr(), P)
                A.add_(buf)
            A.neg_()
            t0 = lap('hessian', t0)
            h0 = handles[0]

            def factor(Ar):
                Ar = Ar.contiguous()
                return (Ar,) + h0.chol_factor(Ar)

            def inverse(Ls, info):
                lap('factor', t0)
                t1 = time.perf_counter()
                h0.tri_inverse(Ls, info)
                lap('inverse', t1)
                return Ls

            res = laplace_from_factor(A, factor, inverse, torch, cov=cov)
            stream.synchronize()
    finally:
        try:
            stream.synchronize()
        except Exception:
            pass
        for h in handles:
            h.set_stream(None)
    return res, A, pi, shapes


def _failed(P, cov, extras):
    out = {'pd': False, 'stderr_vec': np.full(P, np.nan), 'log_evidence': np.nan}
    if cov:
        out['cov'] = np.full((P, P), np.nan)
    if 'chol' in extras:
        out['chol'] = np.full((P, P), np.nan)
    return out


def laplace_glms(population, x, n_lo=0, n_hi=None, device=False, cov=False, extras=()):
    """Laplace approximation of every neuron n in [n_lo, n_hi) at the state x (a MAP estimate, e.g. coord_descent's).
    Returns one dict per neuron: laplace_from_hessian's entries plus 'log_post' (log_prior_n + sum_data ll_n at x) and
    'stderr' (the standard errors unpacked into the shapes of the neuron's differentiable variables).

    device=True: the Hessians stay on the device and are factored and inverted there (laplace_on_device); only 'pd',
    'stderr_vec' / 'stderr', 'log_evidence', 'log_post' and 'info' (0, or the failing column + 1 of the reversed theta
    layout) come back, with cov=True also 'cov' (packed order, as on the host route), and the entries named in extras:
    'A' (packed order) and 'chol' (the lower factor of the packed A: one more device factorisation).  Rows that are not
    positive definite give pd = False and NaNs, as on the host route.  cov and extras have no effect with device=False,
    which returns everything."""
    if not device:
        return _laplace_glms_host(population, x, n_lo, n_hi)
    import torch
    extras = tuple(extras)
    if any(e not in ('A', 'chol') for e in extras):
        raise ValueError("extras: 'A', 'chol'")
    res, A, pi, shapes = laplace_on_device(population, x, n_lo, n_hi, cov=cov)
    n_hi = population.N if n_hi is None else n_hi
    lps, _ = population.compute_lp_grad_packed(x, n_lo, n_hi)
    P = pi.size
    inv = np.argsort(pi)                                       # theta column of every packed position
    invd = torch.tensor(inv, dtype=torch.long, device=A.device)
    info = res['info'].cpu().numpy()
    pd = res['pd'].cpu().numpy()
    logdet = res['logdet'].cpu().numpy()
    stderr = res['stderr'].cpu().numpy()[:, inv]
    covp = res['cov'][:, invd[:, None], invd[None, :]].cpu().numpy() if cov else None
    Ap = A[:, invd[:, None], invd[None, :]].contiguous() if extras else None
    Ah = Ap.cpu().numpy() if 'A' in extras else None
    if 'chol' in extras:
        h0 = population._handle(population.data_sequences[0])
        torch.cuda.synchronize(A.device)
        sc, _, ci = h0.chol_factor(Ap)
        h0.sync()
        chol = (torch.tril(Ap) * sc[:, :, None]).cpu().numpy()
    out = []
    for i in range(len(lps)):
        ok = bool(pd[i]) and np.isfinite(logdet[i]) and np.all(np.isfinite(stderr[i]))
        if ok:
            r = {'pd': True, 'stderr_vec': stderr[i],
                 'log_evidence': float(lps[i]) + 0.5 * P * np.log(2.0 * np.pi) - 0.5 * float(logdet[i])}
            if cov:
                r['cov'] = covp[i]
            if 'chol' in extras:
                r['chol'] = chol[i]
        else:
            r = _failed(P, cov, extras)
        if 'A' in extras:
            r['A'] = Ah[i]
        r['info'] = int(info[i])
        r['log_post'] = float(lps[i])
        r['stderr'] = unpackdict(r['stderr_vec'], shapes)
        out.append(r)
    return out


def _laplace_glms_host(population, x, n_lo=0, n_hi=None):
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("laplace_glms does not run on a time-sharded population (set_time_shard): "
                         "the Hessians are not all-reduced")
    n_hi = population.N if n_hi is None else n_hi
    if n_hi <= n_lo:
        raise ValueError("empty neuron range")
    H = population.compute_hessian_packed(x, n_lo, n_hi)
    lps, _ = population.compute_lp_grad_packed(x, n_lo, n_hi)
    syms = population.glm_syms()
    out = []
    for i, n in enumerate(range(n_lo, n_hi)):
        _, shapes = packdict(get_vars(syms, x['glms'][n]))
        res = laplace_from_hessian(-0.5 * (H[i] + H[i].T), lps[i])
        res['log_post'] = float(lps[i])
        res['stderr'] = unpackdict(res['stderr_vec'], shapes)
        out.append(res)
    return out
