"""
Which couplings are there: per-pair Wald tests of the network GLM with false-discovery control.

For point-process GLMs the standard test of a coupling pre -> post is the Granger-causality test of Kim, Putrino, Ghosh &
Brown (2011): H0: w_{pre -> post} = 0 for the group of B basis weights of the pair, for every ordered pair, with the false
discovery rate controlled over the family (Benjamini & Hochberg 1995).  Here it takes its Wald form on the Laplace
posterior (inference/laplace.py): with S the group's B x B block of the covariance A^-1 at the MAP estimate,

    T = w_g^T S^-1 w_g   ~  chi-square with B degrees of freedom under H0 and the quadratic approximation.

Everything it needs lies on the device after laplace_on_device: the lower factor W of A^-1 per neuron.  pgl_wald_groups_dev
reduces it to one statistic per group (csrc/pglm_wald.h states the rule, wald_groups below restates it in numpy, bit for
bit); the rest is (M, N) numbers on the host.  The reference has no such test.

The likelihood-ratio form needs a restricted refit per pair.  NOT built: the exact restricted refit (a masked lock-step fit
per presynaptic neuron).  Built, with one_step_lr=True: the restricted ONE-STEP point theta - W W_g^T S^-1 w_g, the
minimiser of the quadratic model with the group at zero, and lr1 = 2 [log post(theta_hat) - log post(that point)].  Under
the quadratic approximation lr1 = T; their difference is the user's check of that approximation, not a second test.
"""
import math

import numpy as np

LANES = 64                              # PGL_WALD_LANES
MAX_B = 16                              # PGL_WALD_MAX_B


# ---- the rule of csrc/pglm_wald.h in numpy ------------------------------------------------------------------------------
def _lane_tree_sum(prod):
    """sum of prod[k] in the rule's order: lane k mod 64 adds its terms in ascending k, then the tree p[l] += p[l + h]"""
    n = prod.size
    p = np.zeros(((n + LANES - 1) // LANES) * LANES)
    p[:n] = prod
    acc = np.zeros(LANES)
    for row in p.reshape(-1, LANES):
        acc = acc + row
    h = LANES // 2
    while h:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def _finish(S, w, c):
    """steps 2 .. 5 of the rule in Python floats (IEEE doubles, one rounding per operation): (T, lin, var, info), y"""
    B = len(w)
    nan = float('nan')
    lin = var = 0.0
    for a in range(B):
        lin = lin + c[a] * w[a]
        r = 0.0
        for b in range(B):
            r = r + (S[a][b] if b <= a else S[b][a]) * c[b]
        var = var + c[a] * r
    L = [[0.0] * B for _ in range(B)]
    for a in range(B):
        for b in range(a + 1):
            s = S[a][b]
            for k in range(b):
                s = s - L[a][k] * L[b][k]
            if b < a:
                L[a][b] = s / L[b][b]                          # (a pivot that passed is > 0)
            elif not (math.isfinite(s) and s > 0.0):
                return (nan, nan, nan, float(a + 1)), [nan] * B
            else:
                L[a][a] = math.sqrt(s)
    y = [0.0] * B
    for a in range(B):
        s = w[a]
        for k in range(a):
            s = s - L[a][k] * y[k]
        y[a] = s / L[a][a]
    for a in range(B - 1, -1, -1):
        s = y[a]
        for k in range(a + 1, B):
            s = s - L[k][a] * y[k]
        y[a] = s / L[a][a]
    T = 0.0
    for a in range(B):
        T = T + w[a] * y[a]
    return (T, lin, var, 0.0), y


def wald_groups(W, theta, first, G, B, c, info=None, want_u=False):
    """The numpy statement of pgl_wald_groups_dev: W (M, P, ld) (only j <= i is read), theta (M, P), c (B,), info (M,) or
    None -> out (M, G, 4) = T, lin, var, info and, with want_u, u (G M, P) with row g M + m.  Bit for bit the device's and
    the gcc mirror's result (tests/test_wald_cases.py, tests/test_gpu_wald.py)."""
    W = np.asarray(W, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    c = [float(v) for v in np.asarray(c, dtype=np.float64).reshape(-1)]
    M, P = theta.shape
    first, G, B = int(first), int(G), int(B)
    if not (M > 0 and G > 0 and 0 < B <= MAX_B and first >= 0 and first + G * B <= P and W.shape[:2] == (M, P) and
            W.shape[2] >= P and len(c) == B):
        raise ValueError("wald_groups: W (M, P, ld >= P), theta (M, P), c (B,), 1 <= B <= %d, first + G B <= P" % MAX_B)
    out = np.full((M, G, 4), np.nan)
    u = np.full((G * M, P), np.nan) if want_u else None
    for m in range(M):
        if info is not None and int(info[m]) != 0:
            continue
        for g in range(G):
            o = first + g * B
            S = [[0.0] * B for _ in range(B)]
            for a in range(B):
                for b in range(a + 1):
                    S[a][b] = _lane_tree_sum(W[m, o + a, :o + b + 1] * W[m, o + b, :o + b + 1])
            o4, y = _finish(S, [float(v) for v in theta[m, o:o + B]], c)
            out[m, g] = o4
            if want_u:
                acc = np.zeros(P)
                for a in range(B):
                    t = np.zeros(P)
                    t[:o + a + 1] = W[m, o + a, :o + a + 1] * y[a]
                    acc = acc + t
                u[g * M + m] = acc
    return (out, u) if want_u else out


# ---- the host part ------------------------------------------------------------------------------------------------------
def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values of the finite entries of p (any shape); the others stay NaN and do not count in
    the family.  q_(i) = min_{j >= i} min(1, n p_(j) / j) over the ascending order p_(1) <= .. <= p_(n)
    (scipy.stats.false_discovery_control(method='bh') states the same rule)."""
    p = np.asarray(p, dtype=float)
    q = np.full(p.shape, np.nan)
    ok = np.isfinite(p)
    v = p[ok]
    n = v.size
    if n:
        order = np.argsort(v, kind='stable')
        adj = np.minimum.accumulate((v[order] * n / np.arange(1, n + 1))[::-1])[::-1]
        r = np.empty(n)
        r[order] = np.minimum(adj, 1.0)
        q[ok] = r
    return q


def tests_from_statistics(out, B, n_lo=0, alpha=0.05, include_self=False):
    """coupling_tests' host algebra: out (M, N, 4) = T, lin, var, info per (post = n_lo + m, pre) -> the dict of (M, N)
    arrays 'wald', 'dof', 'p_value', 'q_value', 'significant', 'weight', 'weight_se', 'z', 'group_info'.  The family of the
    false-discovery correction is every ordered pair with a finite statistic, the diagonal post == pre left out unless
    include_self (its entries then keep their p-values and get q = NaN, significant = False)."""
    from scipy.stats import chi2
    out = np.asarray(out, dtype=float)
    M, N = out.shape[:2]
    T, lin, var = out[..., 0], out[..., 1], out[..., 2]
    p = np.where(np.isfinite(T), chi2.sf(np.where(np.isfinite(T), T, 0.0), B), np.nan)
    fam = p.copy()
    if not include_self:
        rows = np.arange(M)
        on = (rows + n_lo < N)
        fam[rows[on], rows[on] + n_lo] = np.nan
    q = benjamini_hochberg(fam)
    with np.errstate(invalid='ignore', divide='ignore'):
        se = np.sqrt(var)
        z = lin / se
    return {'wald': T, 'dof': int(B), 'p_value': p, 'q_value': q, 'significant': np.where(np.isfinite(q), q <= alpha, False),
            'weight': lin, 'weight_se': se, 'z': z, 'group_info': np.where(np.isfinite(out[..., 3]), out[..., 3], -1).astype(int)}


def effective_weight_contrast(population):
    """c_b = dt sum_t basis[t, b]: the integral of the impulse response per unit weight (the "effective weight")."""
    return float(population.glm.dt) * np.asarray(population.glm.imp_model.ibasis, dtype=float).sum(axis=0)


def one_step_points(theta, W, u, first, G, B):
    """theta (M, P), W (M, P, P) lower, u (G M, P) -> the restricted one-step points (G M, P), row g M + m =
    theta_m - W_m u_{m, g} with the group's entries exact zeros (host statement of the device path)."""
    M, P = theta.shape
    X = np.empty((G * M, P))
    for g in range(G):
        for m in range(M):
            X[g * M + m] = theta[m] - np.tril(W[m]).dot(u[g * M + m])
        X[g * M:(g + 1) * M, first + g * B:first + (g + 1) * B] = 0.0
    return X


def _served(population):
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("Hessian-vector products are not implemented for the %s packing" % bad)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("laplace_glms does not run on a time-sharded population (set_time_shard): "
                         "the Hessians are not all-reduced")


EVAL_BUDGET_BYTES = 1 << 30              # one_step_lr: device memory of the points, their steps and evaluations per chunk


def coupling_tests(population, x, alpha=0.05, n_lo=0, n_hi=None, include_self=False, one_step_lr=False, device=True,
                   timings=None):
    """Wald tests of every coupling pre -> post, post in [n_lo, n_hi), at the MAP estimate x (coord_descent's), with
    Benjamini-Hochberg control of the false discovery rate at alpha over all ordered pairs (the diagonal is left out unless
    include_self).  Returns a dict: 'wald' [post - n_lo, pre], 'dof' = B, 'p_value' = chi2.sf(wald, B), 'q_value',
    'significant' = q <= alpha, 'weight' = c^T w_g with c_b = dt sum_t basis[t, b], 'weight_se', 'z' = weight / weight_se,
    'pd' (M,) and 'group_info' (0, or the failing pivot + 1 of the group's block; -1 in a row that is not positive definite).
    'weight' is the integral of the impulse response per unit of the network factor: the current that acts on the neuron is
    W_eff[pre, post] times that response, so where the adjacency or the weights of the network are not all ones the integral
    of the acting coupling is W_eff[pre, post] * weight (z is not changed by the factor, a pair with W_eff = 0 has no
    coupling whatever its weight is).  Rows whose Hessian is not positive definite give NaN and pd = False (under a
    group-lasso prior a zero group has no finite Hessian).

    device=True: laplace_on_device, then pgl_wald_groups_dev on its factor.  device=False: the numpy statement wald_groups on
    the Cholesky factor of the host Laplace route's covariance (theta layout).
    one_step_lr=True (device only) adds 'lr1' and 'lr1_minus_wald': the restricted one-step points by one
    pgl_tri_matvec_shared_dev call with K = N on the kernel's d_u, evaluated by N pgl_ll_grad_dev calls of all rows per data
    sequence, with the log prior added by pgl_bfgs_objective_dev.  Where the (N M, P) arrays of that (u, the steps, the
    points, their gradients) exceed EVAL_BUDGET_BYTES the presynaptic neurons are taken in chunks: kernel, product and
    evaluations per chunk, the same bits.  The exact restricted refit is not built (see the module's text).
    Served: the populations of laplace_glms(device=True); the 'st' and Dirichlet packings and time shards raise as there.
    timings: a dict that receives the seconds of 'hessian', 'factor', 'inverse', 'wald', 'evaluations' (each behind a
    synchronisation; tools/conn_bench.py)."""
    _served(population)
    n_hi = population.N if n_hi is None else n_hi
    if n_hi <= n_lo:
        raise ValueError("empty neuron range")
    N, B = population.N, int(population.glm.imp_model.B)
    first = 1 + int(population.glm.Dstim)
    c = effective_weight_contrast(population)
    if not device:
        if one_step_lr:
            raise ValueError("one_step_lr needs device=True")
        out, pd = _host_statistics(population, x, n_lo, n_hi, first, N, B, c)
        res = tests_from_statistics(out, B, n_lo, alpha, include_self)
        res['pd'] = pd
        return res
    import time
    from theano_pyglm_amd.inference.laplace import laplace_on_device
    from theano_pyglm_amd.inference.lockstep import session
    lap, A, pi, shapes = laplace_on_device(population, x, n_lo, n_hi, timings=timings)
    del A
    lr1 = None
    with session(population) as (torch, dev, stream, handles):
        h0 = handles[0]
        f64 = torch.float64
        t0 = time.perf_counter()
        W = lap['W'].contiguous()
        info = lap['info'].to(torch.int32).contiguous()
        theta = torch.tensor(population.theta_matrix(x, n_lo, n_hi), dtype=f64, device=dev)
        cd = torch.tensor(c, dtype=f64, device=dev)
        out_d = h0.wald_groups(W, theta, first, N, B, cd, info)
        if timings is not None:
            stream.synchronize()
            timings['wald'] = timings.get('wald', 0.0) + time.perf_counter() - t0
        if one_step_lr:
            t0 = time.perf_counter()
            lr1 = _one_step_lr(population, x, torch, dev, handles, W, theta, cd, first, N, B, n_lo, n_hi, info)
            if timings is not None:
                stream.synchronize()
                timings['evaluations'] = timings.get('evaluations', 0.0) + time.perf_counter() - t0
        stream.synchronize()
        out = out_d.cpu().numpy()
        pd = lap['pd'].cpu().numpy().astype(bool)
        if lr1 is not None:
            lr1 = lr1.cpu().numpy()
    res = tests_from_statistics(out, B, n_lo, alpha, include_self)
    res['pd'] = pd
    if lr1 is not None:
        lr1 = np.where(np.isfinite(res['wald']), lr1, np.nan)     # (a failed row or group has no point)
        res['lr1'] = lr1
        res['lr1_minus_wald'] = lr1 - res['wald']
    return res


def _one_step_lr(population, x, torch, dev, handles, W, theta, cd, first, G, B, n_lo, n_hi, info):
    """lr1 (M, G) on the device: per chunk of K presynaptic neurons the kernel's u (K M, P), the steps W u by one
    pgl_tri_matvec_shared_dev, the points with the group's entries at exact zeros, K evaluations of all rows per data
    sequence and the prior.  At most five (K M, P) arrays live at a time (u, the points, the gradients, two temporaries)."""
    from theano_pyglm_amd.inference.batched_bfgs import _Packing
    h0 = handles[0]
    M, P = theta.shape
    f64 = torch.float64
    prm = _Packing(population, torch, handles, (n_lo, n_hi)).prior_params()
    Weff = torch.tensor(population.W_eff(x), dtype=f64, device=dev)

    def neg_log_post(Xt, K, gr):
        """f (K M,) = -(log prior + sum over the data sequences of ll) at the K blocks of M rows of Xt; gr: (K M, P) of room"""
        tot = None
        for h in handles:
            ll = torch.empty(K * M, dtype=f64, device=dev)
            g = gr if tot is None else torch.empty_like(gr)
            for k in range(K):
                h.ll_grad_dev(Xt[k * M:].data_ptr(), Weff.data_ptr(), ll[k * M:].data_ptr(), g[k * M:].data_ptr(), n_lo, n_hi)
            tot = (ll, g) if tot is None else (tot[0].add_(ll), tot[1].add_(g))
        h0.bfgs_objective_dev(K * M, P, Xt.data_ptr(), tot[0].data_ptr(), tot[1].data_ptr(), prm)
        return tot[0]

    f_hat = neg_log_post(theta, 1, torch.empty((M, P), dtype=f64, device=dev))
    per = max(1, min(G, EVAL_BUDGET_BYTES // (5 * M * P * 8)))
    f1 = torch.empty(G * M, dtype=f64, device=dev)
    room = [torch.empty((min(per, G) * M, P), dtype=f64, device=dev) for _ in range(3)]       # u, step -> points, gradients
    for g0 in range(0, G, per):
        K = min(per, G - g0)
        u, X, gr = (r[:K * M] for r in room)
        h0.wald_groups(W, theta, first + g0 * B, K, B, cd, info, u=u)     # (the statistics of the chunk once more: not kept)
        h0.tri_matvec_shared_dev(W, M, K, P, 0, u, X)
        Xv = X.view(K, M, P)
        torch.sub(theta[None], Xv, out=Xv)
        for k in range(K):
            Xv[k, :, first + (g0 + k) * B:first + (g0 + k + 1) * B] = 0.0
        # a failed row or group has NaN here: it is evaluated at theta_hat instead and reported as NaN by the caller
        Xv.copy_(torch.where(torch.isfinite(Xv).all(dim=2, keepdim=True), Xv, theta[None]))
        f1[g0 * M:(g0 + K) * M] = neg_log_post(X, K, gr)
    return 2.0 * (f1.view(G, M) - f_hat[None, :]).t()


def _host_statistics(population, x, n_lo, n_hi, first, N, B, c):
    """out (M, N, 4) and pd (M,) from the host Laplace route: W = the Cholesky factor of the covariance in the theta layout"""
    from theano_pyglm_amd.inference.laplace import laplace_glms, theta_positions
    pi, _ = theta_positions(population, x, n_lo)
    host = laplace_glms(population, x, n_lo, n_hi)
    M, P = n_hi - n_lo, pi.size
    W = np.zeros((M, P, P))
    info = np.zeros(M, dtype=np.int32)
    for m, r in enumerate(host):
        if r['pd']:
            try:
                W[m] = np.linalg.cholesky(r['cov'][np.ix_(pi, pi)])
            except np.linalg.LinAlgError:
                info[m] = 1
        else:
            info[m] = 1
    theta = population.theta_matrix(x, n_lo, n_hi)
    return wald_groups(W, theta, first, N, B, c, info=info), info == 0


def detection_counts(res, truth, include_self=False):
    """Plain counts of coupling_tests' result against a true adjacency truth[post, pre] (bool) over the tested family (finite
    q-values; the diagonal as include_self says): {'n', 'positives', 'negatives', 'tp', 'fp', 'tpr', 'fpr', 'auc'}; auc = the
    area under the ROC of T (the Mann-Whitney statistic, ties at one half); a rate without a denominator is NaN."""
    from scipy.stats import rankdata
    truth = np.asarray(truth, dtype=bool)
    fam = np.isfinite(res['wald']) & (np.isfinite(res['q_value']) if not include_self else True)
    t, sig, T = truth[fam], np.asarray(res['significant'])[fam], res['wald'][fam]
    npos, nneg = int(t.sum()), int((~t).sum())
    tp, fp = int(np.sum(sig & t)), int(np.sum(sig & ~t))
    auc = float('nan')
    if npos and nneg:
        r = rankdata(T)
        auc = float((r[t].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))
    return {'n': int(fam.sum()), 'positives': npos, 'negatives': nneg, 'tp': tp, 'fp': fp,
            'tpr': tp / npos if npos else float('nan'), 'fpr': fp / nneg if nneg else float('nan'), 'auc': auc}


def format_table(res, alpha, truth=None, include_self=False):
    """The text synth_map --coupling-test prints: the number of significant pairs, against a true adjacency the true- and
    false-positive rates and the area under the ROC of T, and with lr1 the median and maximum |lr1 - T| / max(T, 1)."""
    fam = np.isfinite(res['q_value'])
    lines = ["coupling tests (Wald, %d d.o.f., Benjamini-Hochberg at %g): %d of %d pairs significant; %d of %d rows positive definite"
             % (res['dof'], alpha, int(np.sum(res['significant'])), int(fam.sum()), int(np.sum(res['pd'])), len(res['pd']))]
    if truth is not None:
        d = detection_counts(res, truth, include_self)
        lines.append("against the true adjacency: %d true couplings, %d absent; true positives %d (rate %.3f), false positives %d "
                     "(rate %.3f), area under the ROC of T %.3f" % (d['positives'], d['negatives'], d['tp'], d['tpr'], d['fp'],
                                                                    d['fpr'], d['auc']))
    if 'lr1' in res:
        ok = np.isfinite(res['lr1']) & np.isfinite(res['wald'])
        rel = np.abs(res['lr1_minus_wald'][ok]) / np.maximum(res['wald'][ok], 1.0)
        lines.append("one-step likelihood ratio: |lr1 - T| / max(T, 1) median %.3e, maximum %.3e over %d pairs"
                     % ((np.median(rel), np.max(rel), rel.size) if rel.size else (float('nan'), float('nan'), 0)))
    return "\n".join(lines)
