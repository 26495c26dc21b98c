"""
Laplace approximation of the per-neuron posterior at a MAP estimate.

Given the other neurons' parameters and the network, the log posterior of neuron n's packed GLM parameters theta_n is
log_prior_n + sum_data ll_n (what fit_glm maximises, coord_descent.py:161-204).  Around its mode theta_hat

    log p(theta) ~ log p(theta_hat) - 1/2 (theta - theta_hat)^T A (theta - theta_hat),   A = -Hessian at theta_hat

so the posterior is approximately N(theta_hat, A^-1): standard errors sqrt(diag A^-1) and the evidence

    log Z_n ~ log p(theta_hat) + (P / 2) log 2 pi - 1/2 log det A

which compares models (e.g. values of the group-lasso `lam`) without held-out data.  The dense Hessian comes from the
device (Population.compute_hessian_packed: one Gram contraction per data sequence), the P x P factorisation runs on the
host (P <= 1 221 at the shapes the library serves).  The reference builds the same matrix with hessian_wrt_list
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


def laplace_glms(population, x, n_lo=0, n_hi=None):
    """Laplace approximation of every neuron n in [n_lo, n_hi) at the state x (a MAP estimate, e.g. coord_descent's).
    Returns one dict per neuron: laplace_from_hessian's entries plus 'log_post' (log_prior_n + sum_data ll_n at x) and
    'stderr' (the standard errors unpacked into the shapes of the neuron's differentiable variables)."""
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
