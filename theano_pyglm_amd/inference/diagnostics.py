"""Convergence diagnostics of posterior draws after Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021), "Rank-normalization,
folding, and localization: an improved R-hat for assessing convergence of MCMC": rank-normalised and folded split-R-hat,
bulk and tail effective sample size, the Monte-Carlo standard error of the mean, beside the pooled moments and quantiles.

chain_diagnostics is the readable numpy statement of the rule that csrc/pglm_diag.h states for one column, vectorised over
the columns; diagnose runs the same rule on the device (DeviceGlm.chain_diag, k_diag_column), where the lock-step samplers
keep their draws, and falls back to the numpy statement only above DIAG_MAX_DRAWS pooled draws ('route' says which).

These are not the figures of batched_hmc.summarize: its 'ess' is Geyer's initial positive sequence per chain, summed over the
chains, with no between-chain term and no monotone correction, and its 'rhat' the plain split-R-hat ('rhat_plain' here)."""
import numpy as np

from theano_pyglm_amd._lib import DIAG_MAX_DRAWS, DIAG_ROWS

QUANTILES = ((1, 40), (1, 20), (1, 2), (19, 20), (39, 40))      # q025, q05, median, q95, q975 as fractions


def normal_score(r, S):
    """Phi^-1((r - 3/8) / (S + 1/4)) of average ranks r among S by Wichura's AS 241 (PPND16), entered with the centred argument
    and the probability of the nearer tail (pgl_diag_score)."""
    r = np.asarray(r, dtype=float)
    d = S + 0.25
    q = (r - 0.5 * (S + 1.0)) / d
    out = np.empty_like(q)
    mid = np.abs(q) <= 0.425
    u = 0.180625 - q[mid] ** 2
    num = np.polyval([2.5090809287301226727e3, 3.3430575583588128105e4, 6.7265770927008700853e4, 4.5921953931549871457e4,
                      1.3731693765509461125e4, 1.9715909503065514427e3, 1.3314166789178437745e2, 3.3871328727963666080e0], u)
    den = np.polyval([5.2264952788528545610e3, 2.8729085735721942674e4, 3.9307895800092710610e4, 2.1213794301586595867e4,
                      5.3941960214247511077e3, 6.8718700749205790830e2, 4.2313330701600911252e1, 1.0], u)
    out[mid] = q[mid] * num / den
    rt, qt = r[~mid], q[~mid]
    pt = np.where(qt < 0.0, (rt - 0.375) / d, (S - rt + 0.625) / d)
    u = np.sqrt(-np.log(pt))
    near = u <= 5.0
    a, b = u - 1.6, u - 5.0
    v1 = np.polyval([7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e0,
                     3.64784832476320460504e0, 5.76949722146069140550e0, 4.63033784615654529590e0, 1.42343711074968357734e0], a) / \
        np.polyval([1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                    6.89767334985100004550e-1, 1.67638483018380384940e0, 2.05319162663775882187e0, 1.0], a)
    v2 = np.polyval([2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                     2.96560571828504891230e-1, 1.78482653991729133580e0, 5.46378491116411436990e0, 6.65790464350110377720e0], b) / \
        np.polyval([2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                    1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0], b)
    v = np.where(near, v1, v2)
    out[~mid] = np.where(qt < 0.0, -v, v)
    return out


def average_ranks(v):
    """(r, sorted v) of the pooled values v (S, K) along axis 0: r = #{smaller} + (#{equal} + 1) / 2."""
    S = v.shape[0]
    order = np.argsort(v, axis=0, kind='stable')
    sv = np.take_along_axis(v, order, axis=0)
    idx = np.arange(S)[:, None]
    first = np.ones(sv.shape, dtype=bool)
    first[1:] = sv[1:] != sv[:-1]
    last = np.ones(sv.shape, dtype=bool)
    last[:-1] = first[1:]
    lt = np.maximum.accumulate(np.where(first, idx, 0), axis=0)                       # the start of the run of equals
    end = np.minimum.accumulate(np.where(last, idx, S)[::-1], axis=0)[::-1]           # and its end
    r = np.empty(sv.shape)
    np.put_along_axis(r, order, lt + (end - lt + 2) / 2.0, axis=0)
    return r, sv


def quantile(sv, a, b):
    """The quantile a / b of the sorted columns sv (S, K): numpy.percentile's linear rule with the position in integers."""
    S = sv.shape[0]
    k, rem = divmod(a * (S - 1), b)
    lo, hi = sv[k] + 0.0, sv[min(k + 1, S - 1)] + 0.0       # (a zero order statistic is +0.0)
    g = rem / float(b)
    return lo + (hi - lo) * g if g < 0.5 else hi - (hi - lo) * (1.0 - g)


def split_halves(y):
    """(C, n, K) -> the 2 C split chains (2 C, h, K), chain c's halves at 2 c and 2 c + 1; the middle draw of an odd n is dropped"""
    C, n, K = y.shape
    h = n // 2
    return np.stack([y[:, :h], y[:, n - h:]], axis=1).reshape(2 * C, h, K)


def _acov_mean(yc, t):
    h = yc.shape[1]
    return ((yc[:, :h - t] * yc[:, t:]).sum(axis=1) / h).mean(axis=0)


def series_stats(y, want_ess=True):
    """(rhat, ess, lag) over the columns of the series y (C, n, K): split-R-hat (eqs. 1-4) and the ESS of section 3.2 with its
    truncation lag (pgl_diag_series)."""
    sp = split_halves(np.asarray(y, dtype=float))
    m, h, K = sp.shape
    cm = sp.mean(axis=1)
    yc = sp - cm[:, None]
    bh = cm.var(axis=0, ddof=1)
    W = _acov_mean(yc, 0) * h / (h - 1.0)
    vp = W * (h - 1.0) / h + bh
    with np.errstate(invalid='ignore', divide='ignore'):
        rhat = np.sqrt(vp / W)
    if not want_ess:
        return rhat, None, None
    N = float(m * h)
    live = vp > 0.0                                                  # a series constant over all split chains: ESS 0
    e, o = np.ones(K), np.ones(K)
    pa, pb, acc = np.zeros(K), np.zeros(K), np.zeros(K)
    T = np.zeros(K, dtype=int)
    with np.errstate(invalid='ignore', divide='ignore'):
        rho = lambda t, idx: 1.0 - (W[idx] - _acov_mean(yc[:, :, idx], t)) / vp[idx]
        idx = np.nonzero(live)[0]
        o[idx] = rho(1, idx)
        t = 0
        while True:                                                  # every column still running is at the same pair t
            idx = idx[(e[idx] + o[idx] > 0.0)] if t < h - 5 else idx[:0]
            if idx.size == 0:
                break
            if t >= 2:                                               # initial monotone sequence, against the corrected pair
                fix = idx[e[idx] + o[idx] > pa[idx] + pb[idx]]
                e[fix] = o[fix] = (pa[fix] + pb[fix]) / 2.0
            acc[idx] += e[idx]
            acc[idx] += o[idx]
            pa[idx], pb[idx] = e[idx], o[idx]
            t += 2
            T[idx] = t
            e[idx], o[idx] = rho(t, idx), rho(t + 1, idx)
    last = np.where((e + o >= 0.0) | (e > 0.0), e, 0.0)              # the final odd term
    acc = np.where(T == 0, last, acc)
    tau = np.maximum(-1.0 + 2.0 * acc + last, 1.0 / np.log10(N))
    return rhat, np.where(live, N / tau, 0.0), np.where(live, T, 0).astype(float)


def chain_diagnostics(samples, chains=True):
    """The diagnostics of samples (C, n, ...) -- chains=False: (n, ...), one chain -- as a dict of arrays shaped like one draw,
    keys DIAG_ROWS: 'mean', 'sd', 'median', 'q025', 'q975', 'rhat_plain', 'rhat', 'ess_bulk', 'ess_tail', 'ess_mean',
    'mcse_mean' and the truncation lags 'lag_bulk', 'lag_q05', 'lag_q95', 'lag_mean'.  n >= 8.  The rule, its edge cases
    included, is csrc/pglm_diag.h's."""
    s = np.asarray(samples, dtype=float)
    if not chains:
        s = s[None]
    if s.ndim < 2 or s.shape[1] < 8 or s.shape[0] < 1:
        raise ValueError("chain_diagnostics: samples (n_chains, n_draws >= 8, ...)")
    C, n, shape = s.shape[0], s.shape[1], s.shape[2:]
    x = s.reshape(C, n, -1)
    K, S = x.shape[2], C * n
    pooled = x.reshape(S, K)
    out = dict((k, np.full(K, np.nan)) for k in DIAG_ROWS)
    finite = np.all(np.isfinite(pooled), axis=0)
    const = finite & (pooled.max(axis=0) == pooled.min(axis=0))
    for k in DIAG_ROWS:
        out[k][const] = np.nan if k in ('rhat_plain', 'rhat', 'mcse_mean') else 0.0
    for k in ('mean', 'median', 'q025', 'q975'):
        out[k][const] = pooled[0, const] + 0.0               # (a constant -0.0 / +0.0 column: +0.0)
    go = np.nonzero(finite & ~const)[0]
    if go.size:
        x, pooled = x[:, :, go], pooled[:, go]
        r, sv = average_ranks(pooled)
        Q = [quantile(sv, a, b) for a, b in QUANTILES]
        z = normal_score(r, S).reshape(x.shape)
        zf = normal_score(average_ranks(np.abs(pooled - Q[2]))[0], S).reshape(x.shape)
        rhat_bulk, ess_bulk, lag_bulk = series_stats(z)
        rhat_fold = series_stats(zf, want_ess=False)[0]
        _, ess_lo, lag_lo = series_stats((x <= Q[1]).astype(float))
        _, ess_hi, lag_hi = series_stats((x <= Q[3]).astype(float))
        rhat_plain, ess_mean, lag_mean = series_stats(x)
        sd = pooled.std(axis=0, ddof=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            res = {'mean': pooled.mean(axis=0), 'sd': sd, 'median': Q[2], 'q025': Q[0], 'q975': Q[4], 'rhat_plain': rhat_plain,
                   'rhat': np.where((rhat_fold > rhat_bulk) | np.isnan(rhat_bulk), rhat_fold, rhat_bulk), 'ess_bulk': ess_bulk,
                   'ess_tail': np.minimum(ess_lo, ess_hi), 'ess_mean': ess_mean, 'mcse_mean': sd / np.sqrt(ess_mean),
                   'lag_bulk': lag_bulk, 'lag_q05': lag_lo, 'lag_q95': lag_hi, 'lag_mean': lag_mean}
        for k in DIAG_ROWS:
            out[k][go] = res[k]
    return dict((k, out[k].reshape(shape)) for k in DIAG_ROWS)


def rows_to_dict(rows):
    """The (DIAG_NOUT, ...) result of DeviceGlm.chain_diag as the dict chain_diagnostics returns"""
    return dict((k, np.array(rows[i])) for i, k in enumerate(DIAG_ROWS))


def diagnose(population, samples, chains=True):
    """chain_diagnostics on the device: samples (C, n, ...) -- chains=False: (n, ...) -- as the samplers return them (a numpy
    array is uploaded, a torch device tensor is used where it lies), one workgroup per column (DeviceGlm.chain_diag).
    Returns chain_diagnostics' dict plus 'route': 'device', or 'host' where C n exceeds DIAG_MAX_DRAWS and the numpy
    statement ran instead."""
    from theano_pyglm_amd.inference.lockstep import session
    is_t = hasattr(samples, 'is_cuda')
    shape = tuple(samples.shape)
    if not chains:
        shape = (1,) + shape
    if len(shape) < 2 or shape[1] < 8 or int(np.prod(shape)) == 0:
        raise ValueError("diagnose: samples (n_chains, n_draws >= 8, ...)")
    C, n = shape[0], shape[1]
    if C * n > DIAG_MAX_DRAWS:
        out = chain_diagnostics(samples.cpu().numpy() if is_t else samples, chains=chains)
        out['route'] = 'host'
        return out
    with session(population) as (torch, dev, stream, handles):
        t = samples if is_t else torch.tensor(np.ascontiguousarray(samples, dtype=np.float64), dtype=torch.float64, device=dev)
        t = t.to(dtype=torch.float64).reshape((C, n, -1))
        x = t.permute(1, 0, 2).contiguous()                          # (n, C, K): the samplers' own layout
        rows = handles[0].chain_diag(x, n_chains=C)
        stream.synchronize()
        out = rows_to_dict(rows.cpu().numpy().reshape((len(DIAG_ROWS),) + shape[2:]))
    out['route'] = 'device'
    return out


def queue_summary(handle, samples_dev, n_chains):
    """The samplers' hook, first half: the kernel queued on their tensor (n, n_chains * M, P) where it lies, before the copy.
    -> the device rows, or None where n_chains * n exceeds DIAG_MAX_DRAWS (finish_summary then runs the numpy statement)."""
    n = int(samples_dev.shape[0])
    if n < 8:
        raise ValueError("diagnostics=True needs at least 8 kept draws per chain")
    return handle.chain_diag(samples_dev, n_chains=n_chains) if n * n_chains <= DIAG_MAX_DRAWS else None


def finish_summary(rows, samples, n_chains):
    """Second half, behind the samplers' synchronisation: the 'summary' dict, arrays (M, P), plus 'route'.  samples: the host
    copy as the sampler returns it, (n, M, P) or (n_chains, n, M, P)."""
    if rows is None:
        out = chain_diagnostics(samples, chains=n_chains > 1)
        out['route'] = 'host'
    else:
        out = rows_to_dict(rows.cpu().numpy())
        out['route'] = 'device'
    return out


def worst_table(summary, n_chains, n_lo=0):
    """The per-neuron lines synth_map --diag prints: the worst rhat, the smallest bulk and tail ESS, and the number of
    parameters with rhat > 1.01 or ess_bulk < 100 * n_chains.  summary: arrays (M, P)."""
    rhat, bulk, tail = summary['rhat'], summary['ess_bulk'], summary['ess_tail']
    lines = ["convergence (%d chain%s%s): neuron  max rhat  min ess_bulk  min ess_tail  flagged of %d"
             % (n_chains, '' if n_chains == 1 else 's', ", " + summary['route'] if 'route' in summary else '', rhat.shape[1])]
    total = 0
    for m in range(rhat.shape[0]):
        with np.errstate(invalid='ignore'):
            bad = int(np.sum((rhat[m] > 1.01) | (bulk[m] < 100.0 * n_chains) | np.isnan(rhat[m])))
        total += bad
        lines.append("%6d  %8.4f  %12.1f  %12.1f  %7d" % (n_lo + m, np.nanmax(rhat[m]) if np.any(~np.isnan(rhat[m])) else np.nan,
                                                          bulk[m].min(), tail[m].min(), bad))
    lines.append("%d of %d parameters flagged (rhat > 1.01 or ess_bulk < %d)" % (total, rhat.size, 100 * n_chains))
    return "\n".join(lines)
