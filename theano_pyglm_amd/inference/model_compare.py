"""
Model comparison from posterior draws: WAIC and the held-out log predictive density.

Both need only the draws the lock-step samplers already produce (sample_glms_hmc / sample_glms_nuts) and the
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
(2017) warn that WAIC is unreliable.  PSIS-LOO, their recommended replacement in that case, is not implemented.

Per neuron, from S draws and the blocks b (Watanabe 2010; Vehtari, Gelman & Gabry 2017, eqs. 11-13):
    lppd_b    = log (1/S) sum_s exp(l_sb)        = log(e / S) + m
    p_b       = var_s(l_sb), n - 1 form          = M2 / (S - 1)
    elpd_waic = sum_b (lppd_b - p_b),   p_waic = sum_b p_b,   waic = -2 elpd_waic
    se        = sqrt(n_blocks var_b(lppd_b - p_b))

The held-out log predictive density log (1/S) sum_s p(test | theta_s) is what the reference's test/parallel_mcmc.py prints
per Gibbs sample (pred_ll_cbk); here it is one block per data sequence on the same path.
"""
import numpy as np

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


def pointwise_ll_draws(population, x, samples, block_chunks=40, n_lo=0, pointwise=False):
    """The pointwise log-likelihood of posterior draws, accumulated over the draws on the device.

    samples: (S, M, P) rows of neurons n_lo .. n_lo + M in the theta layout, as sample_glms_hmc / sample_glms_nuts return
    them (a leading chain axis is flattened; a torch device tensor is used where it is).  The other neurons and the
    network stay at x.  Per draw the rows overwrite a device copy of theta_matrix(x) and every data sequence gets one
    pgl_pointwise_dev call; nothing synchronises with the host inside the loop.
    Returns a dict: 'acc' (4, n_blocks, M) -- m, e, mean, M2 of every (block, neuron), the data sequences one after the
    other --, 'n_draws', 'block_chunks', 'blocks_per_sequence', and with pointwise=True 'll' (S, n_blocks, M)."""
    from theano_pyglm_amd.inference.lockstep import session
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("the pointwise log-likelihood of a time-sharded population is not implemented")
    block_chunks = int(block_chunks)
    if block_chunks < 1:
        raise ValueError("block_chunks must be at least 1")
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
        nb = [h.pointwise_count(block_chunks) for h in handles]
        off = np.concatenate(([0], np.cumsum(nb))).astype(int)
        accs = [torch.empty((4, n, N), dtype=f64, device=dev) for n in nb]
        ll = torch.empty((S, int(off[-1]), N), dtype=f64, device=dev) if pointwise else None
        rows = theta[n_lo:n_lo + M]
        for i in range(S):
            rows.copy_(d_s[i])
            for k, h in enumerate(handles):
                h.pointwise_dev(theta.data_ptr(), Weff.data_ptr(), block_chunks, ll[i, off[k]:].data_ptr() if pointwise else 0,
                                accs[k].data_ptr(), i)
        stream.synchronize()
        acc = np.concatenate([a.cpu().numpy() for a in accs], axis=1)[:, :, n_lo:n_lo + M]
        out = {'acc': np.ascontiguousarray(acc), 'n_draws': S, 'block_chunks': block_chunks, 'blocks_per_sequence': nb}
        if pointwise:
            out['ll'] = np.ascontiguousarray(ll.cpu().numpy()[:, :, n_lo:n_lo + M])
    return out


def _waic(lppd, p, S):
    """the per-neuron criteria from lppd_b and p_b (n_blocks, M)"""
    nb = lppd.shape[0]
    el = lppd - p
    with np.errstate(invalid='ignore'):
        se = np.sqrt(nb * np.var(el, axis=0, ddof=1)) if nb > 1 else np.full(lppd.shape[1], np.nan)
    elpd = el.sum(axis=0)
    return {'elpd_waic': elpd, 'p_waic': p.sum(axis=0), 'lppd': lppd.sum(axis=0), 'waic': -2.0 * elpd, 'se': se,
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
    lines = ["WAIC (%d draws, %d blocks of %d bins)" % (res['n_draws'], res['n_blocks'], res.get('block_bins', 0)),
             "%6s %14s %10s %14s %10s %9s" % ('neuron', 'elpd_waic', 'p_waic', 'waic', 'se', 'p_b>0.4')]
    for i in range(len(res['waic'])):
        lines.append("%6d %14.3f %10.3f %14.3f %10.3f %9d" % (n_lo + i, res['elpd_waic'][i], res['p_waic'][i], res['waic'][i],
                                                              res['se'][i], res['n_high_var'][i]))
    lines.append("total elpd_waic %.3f, p_waic %.3f; %d of %d blocks above the variance warning (WAIC unreliable there; "
                 "PSIS-LOO is not implemented)" % (float(np.sum(res['elpd_waic'])), float(np.sum(res['p_waic'])),
                                                   int(np.sum(res['n_high_var'])), res['n_blocks'] * len(res['waic'])))
    return "\n".join(lines)
