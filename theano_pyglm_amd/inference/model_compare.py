"""
Model comparison from posterior draws: WAIC, PSIS-LOO and the held-out log predictive density.

All need only the draws the lock-step samplers already produce (sample_glms_hmc / sample_glms_nuts) and the
log-likelihood of every draw resolved in time.  That comes from the device: per draw one forward pass and a segmented sum
per data sequence (pgl_pointwise_dev), folded over the draws by the same launch (running maximum, rescaled sum of
exponentials, Welford mean and M2 per (block, neuron): csrc/pglm_pointwise.h).  Only the accumulator -- and on request the
(draws, blocks, neurons) matrix -- crosses PCIe, once.

What the pointwise terms are.  The conditional-intensity likelihood of a neuron factorises over time bins given the spike
history: ll_n = sum_t (-dt lam_t + S[t,n] log lam_t).  A block is block_chunks * 256 consecutive bins (counted from the
start of each data sequence; the last block of a sequence may be short) and its term is the sum over its bins, so the
blocks are conditionally independent terms given the history -- not independent observations: the history couples them,
and WAIC's leave-one-out reading holds in that conditional sense only.

WAIC depends on the block length.  lppd_b and p_b are not additive in the block: merging blocks moves variance between
draws from p_waic into lppd (in the limit of ONE block, elpd_waic = log mean exp(ll) - var(ll)).  Compare models at the same
block_chunks, and read n_high_var: blocks whose posterior variance of the term exceeds 0.4, where Vehtari, Gelman & Gabry
(2017) warn that WAIC is unreliable.  PSIS-LOO, their recommended replacement in that case, is loo_glms below.

PSIS-LOO (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024).  The leave-one-block-out predictive
density of block b is an importance-sampling estimate with ratios r_s = 1 / p(y_b | theta_s) = exp(-l_sb); their largest
M = ceil(min(S / 5, 3 sqrt(S))) values are replaced by the quantiles of a generalized Pareto law fitted to them (Zhang &
Stephens 2009), all are truncated at the largest raw ratio and normalised:
    elpd_b = log sum_s w_sb exp(l_sb),    elpd_loo = sum_b elpd_b,    p_loo = sum_b (lppd_b - elpd_b),    looic = -2 elpd_loo
    se     = sqrt(n_blocks var_b(elpd_b))
The fitted shape khat_b is the diagnostic: above min(1 - 1 / log10 S, 0.7) (the 2024 paper's threshold) the estimate of that
block is not to be trusted, and n_khat_bad counts those blocks.  psis_column below is the rule of one column in plain numpy,
the statement to read (csrc/pglm_psis.h states it for the device; k_psis_column runs it one workgroup per column on the matrix
of draws where it lies, and only (4, n_blocks, M) comes back).  Like WAIC it depends on the block length, and the same
caveat holds: the blocks are terms conditional on the spike history.  Leaving a block out does not remove its spikes from the
history of later blocks, so this is leave-one-term-out of the conditional likelihood, not a prediction of unseen spikes.

Per neuron, from S draws and the blocks b (Watanabe 2010; Vehtari, Gelman & Gabry 2017, eqs. 11-13):
    lppd_b    = log (1/S) sum_s exp(l_sb)        = log(e / S) + m
    p_b       = var_s(l_sb), n - 1 form          = M2 / (S - 1)
    elpd_waic = sum_b (lppd_b - p_b),   p_waic = sum_b p_b,   waic = -2 elpd_waic
    se        = sqrt(n_blocks var_b(lppd_b - p_b))

The held-out log predictive density log (1/S) sum_s p(test | theta_s) is what the reference's test/parallel_mcmc.py prints
per Gibbs sample (pred_ll_cbk); here it is one block per data sequence on the same path.
"""
import contextlib

import numpy as np

from theano_pyglm_amd import _lib

WAIC_VAR_WARN = 0.4             # Vehtari, Gelman & Gabry (2017), section 4: p_b above this makes WAIC unreliable
ONE_BLOCK = 1 << 30             # a block_chunks no recording reaches: one block per data sequence


def _draws(samples, P):
    """(tensor or array (S, M, P), is_tensor): a leading chain axis flattened"""
    is_tensor = hasattr(samples, 'data_ptr')
    s = samples if is_tensor else np.asarray(samples, dtype=float)
    if s.ndim == 4:
        s = s.reshape((s.shape[0] * s.shape[1],) + tuple(s.shape[2:]))
    if s.ndim != 3 or s.shape[0] < 1 or s.shape[1] < 1 or s.shape[2] != P:
        raise ValueError("samples: (S, M, P) or (n_chains, S, M, P) rows in the theta layout, P = %d" % P)
    return s, is_tensor


@contextlib.contextmanager
def _draw_loop(population, x, samples, n_lo, what):
    """with _draw_loop(...) as (torch, dev, stream, handles, S, M, run): the session of a quantity folded over posterior draws
    (lock-step's session: the handles of every data sequence on the drivers' stream).  samples: (S, M, P) rows of neurons
    n_lo .. n_lo + M, see _draws; `what` names the quantity where a time-sharded population is turned down.  run(call) is
    the loop: per draw i the rows overwrite a device copy of theta_matrix(x) and every handle k gets
    call(i, k, handle, theta_ptr, Weff_ptr); nothing in it synchronises with the host."""
    from theano_pyglm_amd.inference.lockstep import session
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("%s of a time-sharded population %s not implemented" % what)
    N, P = population.N, population.glm.P
    s, is_tensor = _draws(samples, P)
    S, M = int(s.shape[0]), int(s.shape[1])
    if n_lo < 0 or n_lo + M > N:
        raise ValueError("neurons %d .. %d of %d" % (n_lo, n_lo + M, N))
    population._check_vars(x)
    theta0 = np.ascontiguousarray(population.theta_matrix(x))
    with session(population) as (torch, dev, stream, handles):
        f64 = torch.float64
        theta = torch.tensor(theta0, dtype=f64, device=dev)
        Weff = torch.tensor(np.ascontiguousarray(population.W_eff(x)), dtype=f64, device=dev)
        d_s = s.to(device=dev, dtype=f64).contiguous() if is_tensor else torch.tensor(s, dtype=f64, device=dev)
        rows = theta[n_lo:n_lo + M]

        def run(call):
            for i in range(S):
                rows.copy_(d_s[i])
                for k, h in enumerate(handles):
                    call(i, k, h, theta.data_ptr(), Weff.data_ptr())
        yield torch, dev, stream, handles, S, M, run


def pointwise_ll_draws(population, x, samples, block_chunks=40, n_lo=0, pointwise=False):
    return _pointwise_ll_draws(population, x, samples, block_chunks, n_lo, pointwise, False)


def _pointwise_ll_draws(population, x, samples, block_chunks, n_lo, pointwise, psis):
    """The pointwise log-likelihood of posterior draws, accumulated over the draws on the device.

    samples: (S, M, P) rows of neurons n_lo .. n_lo + M in the theta layout, as sample_glms_hmc / sample_glms_nuts return
    them (a leading chain axis is flattened; a torch device tensor is used where it is).  The other neurons and the
    network stay at x.  Per draw the rows overwrite a device copy of theta_matrix(x) and every data sequence gets one
    pgl_pointwise_dev call; nothing synchronises with the host inside the loop.
    (psis: loo_glms' form -- the matrix is kept on the device and PSIS-LOO runs on it there, 'psis' (4, n_blocks, M) and
    'route' come back instead of 'll'; above PSIS_MAX_DRAWS the matrix comes back for the numpy statement.)
    Returns a dict: 'acc' (4, n_blocks, M) -- m, e, mean, M2 of every (block, neuron), the data sequences one after the
    other --, 'n_draws', 'block_chunks', 'blocks_per_sequence', and with pointwise=True 'll' (S, n_blocks, M)."""
    block_chunks = int(block_chunks)
    if block_chunks < 1:
        raise ValueError("block_chunks must be at least 1")
    N = population.N
    what = ("the pointwise log-likelihood", "is")
    with _draw_loop(population, x, samples, n_lo, what) as (torch, dev, stream, handles, S, M, run):
        f64 = torch.float64
        nb = [h.pointwise_count(block_chunks) for h in handles]
        off = np.concatenate(([0], np.cumsum(nb))).astype(int)
        accs = [torch.empty((4, n, N), dtype=f64, device=dev) for n in nb]
        ll = torch.empty((S, int(off[-1]), N), dtype=f64, device=dev) if pointwise or psis else None
        pointwise = ll is not None
        run(lambda i, k, h, theta, Weff: h.pointwise_dev(theta, Weff, block_chunks, ll[i, off[k]:].data_ptr() if pointwise else 0,
                                                         accs[k].data_ptr(), i))
        if psis and 2 <= S <= _lib.PSIS_MAX_DRAWS:           # the matrix stays where it is: (4, n_blocks, M) comes back
            cols = ll if M == N else ll[:, :, n_lo:n_lo + M].contiguous()
            d_psis = handles[0].psis_loo(cols)
        stream.synchronize()
        acc = np.concatenate([a.cpu().numpy() for a in accs], axis=1)[:, :, n_lo:n_lo + M]
        out = {'acc': np.ascontiguousarray(acc), 'n_draws': S, 'block_chunks': block_chunks, 'blocks_per_sequence': nb}
        if psis and 2 <= S <= _lib.PSIS_MAX_DRAWS:
            out['psis'], out['route'] = d_psis.cpu().numpy(), 'device'
        elif pointwise:
            out['ll'] = np.ascontiguousarray(ll.cpu().numpy()[:, :, n_lo:n_lo + M])
    return out


def _waic(lppd, p, S):
    """the per-neuron criteria from lppd_b and p_b (n_blocks, M)"""
    nb = lppd.shape[0]
    el = lppd - p
    with np.errstate(invalid='ignore'):
        se = np.sqrt(nb * np.var(el, axis=0, ddof=1)) if nb > 1 else np.full(lppd.shape[1], np.nan)
    elpd = el.sum(axis=0)
    return {'elpd_waic': elpd, 'p_waic': p.sum(axis=0), 'lppd': lppd.sum(axis=0), 'waic': -2.0 * elpd, 'se': se, 'elpd_b': el,
            'n_high_var': np.sum(p > WAIC_VAR_WARN, axis=0).astype(np.int64), 'n_blocks': nb, 'n_draws': int(S)}


def waic_from_accumulators(acc, n_draws):
    """WAIC per neuron from the accumulator state (4, n_blocks, M) -- m, e, mean, M2 -- after n_draws >= 2 draws: a dict of
    (M,) arrays elpd_waic, p_waic, lppd, waic, se, n_high_var, and n_blocks, n_draws.  A (block, neuron) that met a
    non-finite term is NaN and so is its neuron."""
    acc = np.asarray(acc, dtype=float)
    S = int(n_draws)
    if acc.ndim != 3 or acc.shape[0] != 4 or S < 2:
        raise ValueError("acc: (4, n_blocks, M) after at least two draws")
    m, e, _, m2 = acc
    return _waic(np.log(e / S) + m, m2 / (S - 1.0), S)


def waic_from_pointwise(ll):
    """The same from the matrix ll (S, n_blocks, M) of pointwise terms, in plain numpy (two passes)."""
    ll = np.asarray(ll, dtype=float)
    if ll.ndim != 3 or ll.shape[0] < 2:
        raise ValueError("ll: (S, n_blocks, M), S >= 2")
    S = ll.shape[0]
    return _waic(log_mean_exp(ll), np.var(ll, axis=0, ddof=1), S)


def log_mean_exp(a):
    """log mean exp over axis 0, shifted by the maximum"""
    a = np.asarray(a, dtype=float)
    m = a.max(axis=0)
    return np.log(np.mean(np.exp(a - m[None]), axis=0)) + m


# ---- PSIS-LOO ----------------------------------------------------------------------------------------------------------
PSIS_MIN_TAIL = 5               # fewer tail elements: khat = +inf, nothing is smoothed
LOG_DBL_MIN = float(np.log(np.finfo(float).tiny))


def _tail_len(S):
    """M = ceil(min(S / 5, 3 sqrt(S)))"""
    return int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S))))


def _quantiles(n):
    """p_i = (i - 0.5) / n, i = 1 .. n"""
    return (np.arange(1, n + 1) - 0.5) / n


def _truncate(x):
    """no ratio above the largest raw one: x <= 0"""
    return np.minimum(x, 0.0)


def gpd_fit(e):
    """(khat, sigma) of the generalized Pareto law fitted to the ascending excesses e (n,) by Zhang & Stephens (2009) with
    the weak prior of the loo package: 30 + floor(sqrt(n)) candidate shapes, their profile likelihoods as weights."""
    n = len(e)
    m = 30 + int(np.sqrt(n))
    i = np.arange(1, m + 1)
    b = 1.0 / e[-1] + (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * e[int(n / 4.0 + 0.5) - 1])
    k = np.array([np.mean(np.log1p(-bi * e)) for bi in b])
    L = n * (np.log(-(b / k)) - k - 1.0)
    w = np.array([1.0 / np.sum(np.exp(L - Li)) for Li in L])
    keep = w >= 10.0 * np.finfo(float).eps
    w = w[keep] / np.sum(w[keep])
    bp = np.sum(w * b[keep])
    k = np.mean(np.log1p(-bp * e))
    return (n * k + 5.0) / (n + 10.0), -k / bp


def _logsumexp(a):
    m = np.max(a)
    return m + np.log(np.sum(np.exp(a - m)))


def psis_column(l):
    """PSIS-LOO of one column l (S,): (elpd, khat, n_eff, tail length, lw (S,)).  The rule of csrc/pglm_psis.h, step by step."""
    l = np.asarray(l, dtype=float)
    S = len(l)
    if not np.all(np.isfinite(l)):
        return np.nan, np.nan, np.nan, np.nan, np.full(S, np.nan)
    x = -l - np.max(-l)                                     # 1. log ratios, the largest at 0
    order = np.argsort(-l, kind='stable')                   # 2. on the raw input: descending l, ties by the draw index
    M = _tail_len(S)
    cut = order[S - M - 1]                                  # 3. the cutoff element, and the tail strictly beyond it
    x_cut = max(x[cut], LOG_DBL_MIN)
    tail = order[l[order] < l[cut]]
    n = len(tail)
    khat = np.inf                                           # 4. a short tail is not fitted
    if n >= PSIS_MIN_TAIL:
        with np.errstate(all='ignore'):
            khat, sigma = gpd_fit(np.exp(x[tail]) - np.exp(x_cut))                                              # 5.
            if np.isfinite(khat):                                                                                # 6.
                a = np.log1p(-_quantiles(n))
                q = -a if abs(khat) < np.finfo(float).eps else np.expm1(-khat * a) / khat
                x = x.copy()
                x[tail] = np.log(np.exp(x_cut) + sigma * q)
    x = _truncate(x)                                        # 7.
    lw = x - _logsumexp(x)
    return _logsumexp(lw + l), khat, 1.0 / np.sum(np.exp(2.0 * lw)), float(n), lw                                # 8.


def psis_loo_from_pointwise(ll, weights=False):
    """PSIS-LOO of every column of ll (S, n_blocks, M) -- any (S, ...) -- in plain numpy: out (4, ...) = elpd, khat, n_eff, tail
    length, as DeviceGlm.psis_loo returns them; with weights=True (out, lw (S, ...))."""
    ll = np.asarray(ll, dtype=float)
    if ll.ndim < 2 or ll.shape[0] < 2:
        raise ValueError("ll: (S, ...), S >= 2")
    S, shape = ll.shape[0], ll.shape[1:]
    cols = ll.reshape(S, -1)
    out = np.empty((4, cols.shape[1]))
    lw = np.empty(cols.shape)
    for c in range(cols.shape[1]):
        out[0, c], out[1, c], out[2, c], out[3, c], lw[:, c] = psis_column(cols[:, c])
    out = out.reshape((4,) + shape)
    return (out, lw.reshape(ll.shape)) if weights else out


def khat_threshold(S):
    """min(1 - 1 / log10 S, 0.7): Vehtari, Simpson, Gelman, Yao & Gabry (2024)"""
    return min(1.0 - 1.0 / np.log10(S), 0.7)


def loo_from_columns(out, lppd_b, S):
    """The per-neuron criteria from psis_loo's out (4, n_blocks, M), lppd_b (n_blocks, M) and the number of draws S: a dict of
    (M,) arrays elpd_loo, p_loo, looic, se, khat_max, n_khat_bad, the pointwise elpd_b and khat_b (n_blocks, M), and n_blocks,
    n_draws, khat_threshold."""
    out = np.asarray(out, dtype=float)
    lppd_b = np.asarray(lppd_b, dtype=float)
    if out.ndim != 3 or out.shape[0] != 4 or lppd_b.shape != out.shape[1:]:
        raise ValueError("out: (4, n_blocks, M) and lppd_b: (n_blocks, M)")
    el, kh = out[0], out[1]
    nb = el.shape[0]
    thr = khat_threshold(S)
    with np.errstate(invalid='ignore'):
        se = np.sqrt(nb * np.var(el, axis=0, ddof=1)) if nb > 1 else np.full(el.shape[1], np.nan)
    elpd = el.sum(axis=0)
    return {'elpd_loo': elpd, 'p_loo': (lppd_b - el).sum(axis=0), 'looic': -2.0 * elpd, 'se': se, 'khat_max': kh.max(axis=0),
            'n_khat_bad': np.sum(kh > thr, axis=0).astype(np.int64), 'elpd_b': el, 'khat_b': kh, 'n_eff_b': out[2],
            'n_blocks': nb, 'n_draws': int(S), 'khat_threshold': thr}


def loo_glms(population, x, samples, block_chunks=40, n_lo=0):
    """PSIS-LOO of neurons n_lo .. n_lo + M on the population's data from the draws `samples`.  The draws run as in
    pointwise_ll_draws; their matrix ll (S, n_blocks, N) stays on the device, DeviceGlm.psis_loo runs on it there, and
    (4, n_blocks, M) and the accumulator that gives lppd_b come back ('route' = 'device').  With more than PSIS_MAX_DRAWS
    draws the matrix is copied and psis_loo_from_pointwise takes it ('route' = 'host').  Returns loo_from_columns' dict with
    'route', 'block_bins', 'n_lo'."""
    r = _pointwise_ll_draws(population, x, samples, block_chunks, n_lo, False, True)
    S = r['n_draws']
    if S < 2:
        raise ValueError("PSIS-LOO needs at least two draws")
    if 'psis' not in r:
        r['psis'], r['route'] = psis_loo_from_pointwise(r['ll']), 'host'
    m, e = r['acc'][0], r['acc'][1]
    res = loo_from_columns(r['psis'], np.log(e / S) + m, S)
    res['route'] = r['route']
    res['block_bins'] = 256 * r['block_chunks']
    res['n_lo'] = int(n_lo)
    return res


def elpd_diff(res_a, res_b):
    """Paired comparison of two models on the same data and blocks, from two LOO or two WAIC results (their pointwise
    'elpd_b' (n_blocks, M)): {'elpd_diff': sum_b d_b, 'se_diff': sqrt(n_blocks var_b d_b)} per neuron, d_b = elpd_b^a - elpd_b^b."""
    a, b = np.asarray(res_a['elpd_b'], dtype=float), np.asarray(res_b['elpd_b'], dtype=float)
    if a.shape[0] != b.shape[0]:
        raise ValueError("the two results have %d and %d blocks: compare at the same block_chunks on the same data"
                         % (a.shape[0], b.shape[0]))
    if a.shape != b.shape:
        raise ValueError("the two results cover %d and %d neurons" % (a.shape[1], b.shape[1]))
    d = a - b
    nb = d.shape[0]
    with np.errstate(invalid='ignore'):
        se = np.sqrt(nb * np.var(d, axis=0, ddof=1)) if nb > 1 else np.full(d.shape[1], np.nan)
    return {'elpd_diff': d.sum(axis=0), 'se_diff': se, 'n_blocks': nb}


def waic_glms(population, x, samples, block_chunks=40, n_lo=0):
    """WAIC of neurons n_lo .. n_lo + M on the population's data from the draws `samples` (pointwise_ll_draws, then
    waic_from_accumulators).  'block_bins' = 256 block_chunks, the bins of a whole block."""
    r = pointwise_ll_draws(population, x, samples, block_chunks, n_lo)
    res = waic_from_accumulators(r['acc'], r['n_draws'])
    res['block_bins'] = 256 * r['block_chunks']
    res['n_lo'] = int(n_lo)
    return res


def heldout_lpd(test_population, x, samples, n_lo=0):
    """Held-out log predictive density log (1/S) sum_s p(test | theta_s) per neuron, on the data of test_population (same
    model, conditioned on the held-out recording).  The per-draw totals are block sums on the device: one block per data
    sequence.  Returns {'lpd': (M,), 'trace': (S, M) the ll of the held-out data under every draw -- what the reference prints
    per sample --, 'n_draws'}."""
    r = pointwise_ll_draws(test_population, x, samples, ONE_BLOCK, n_lo, pointwise=True)
    trace = r['ll'].sum(axis=1)
    return {'lpd': log_mean_exp(trace), 'trace': trace, 'n_draws': r['n_draws'], 'n_lo': int(n_lo)}


def format_table(res):
    n_lo = res.get('n_lo', 0)
    if 'lpd' in res:
        lines = ["held-out log predictive density (%d draws)" % res['n_draws'],
                 "%6s %14s %14s %14s" % ('neuron', 'lpd', 'mean ll', 'sd ll')]
        tr = res['trace']
        for i in range(len(res['lpd'])):
            lines.append("%6d %14.3f %14.3f %14.3f" % (n_lo + i, res['lpd'][i], tr[:, i].mean(),
                                                        tr[:, i].std(ddof=1) if tr.shape[0] > 1 else 0.0))
        lines.append("total %.3f" % float(np.sum(res['lpd'])))
        return "\n".join(lines)
    if 'elpd_loo' in res:
        lines = ["PSIS-LOO (%d draws, %d blocks of %d bins, %s)" % (res['n_draws'], res['n_blocks'], res.get('block_bins', 0),
                                                                   res.get('route', 'host')),
                 "%6s %14s %10s %14s %10s %9s %9s" % ('neuron', 'elpd_loo', 'p_loo', 'looic', 'se', 'max khat',
                                                      'khat>%.2f' % res['khat_threshold'])]
        for i in range(len(res['looic'])):
            lines.append("%6d %14.3f %10.3f %14.3f %10.3f %9.3f %9d" % (n_lo + i, res['elpd_loo'][i], res['p_loo'][i], res['looic'][i],
                                                                         res['se'][i], res['khat_max'][i], res['n_khat_bad'][i]))
        lines.append("total elpd_loo %.3f, p_loo %.3f; %d of %d blocks above the khat threshold (their elpd is unreliable)"
                     % (float(np.sum(res['elpd_loo'])), float(np.sum(res['p_loo'])), int(np.sum(res['n_khat_bad'])),
                        res['n_blocks'] * len(res['looic'])))
        return "\n".join(lines)
    lines = ["WAIC (%d draws, %d blocks of %d bins)" % (res['n_draws'], res['n_blocks'], res.get('block_bins', 0)),
             "%6s %14s %10s %14s %10s %9s" % ('neuron', 'elpd_waic', 'p_waic', 'waic', 'se', 'p_b>0.4')]
    for i in range(len(res['waic'])):
        lines.append("%6d %14.3f %10.3f %14.3f %10.3f %9d" % (n_lo + i, res['elpd_waic'][i], res['p_waic'][i], res['waic'][i],
                                                              res['se'][i], res['n_high_var'][i]))
    lines.append("total elpd_waic %.3f, p_waic %.3f; %d of %d blocks above the variance warning (WAIC unreliable there; "
                 "use PSIS-LOO: --loo, loo_glms)" % (float(np.sum(res['elpd_waic'])), float(np.sum(res['p_waic'])),
                                                   int(np.sum(res['n_high_var'])), res['n_blocks'] * len(res['waic'])))
    return "\n".join(lines)
