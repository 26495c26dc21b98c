"""
Posterior-predictive check of the spike counts: draw many spike trains from the model at the parameters x on the current
data's length and stimulus (pgl_simulate_batch_dev: one workgroup per replicate, only the counts come back) and compare
every neuron's observed count with the replicates.

A count far in a tail of its predictive distribution says the model does not reproduce that neuron's rate; it says nothing
about timing (inference/gof.py tests that).  The reference has no counterpart.

Resolved in time: rate_bands folds the expected count of every time window over posterior draws on the device (one forward
pass plus pgl_rate_windows_dev per draw and data sequence; only the accumulator and the observed counts come back, once) --
the firing rate with its posterior band that the reference's plot_firing_rate(s_glm, s_glm_std) draws from per-draw
eval_state dicts, plus windowed residuals:
    pearson = (obs - mean) / sqrt(mean + var)     the law of total variance of a Poisson count whose mean is random;
    pit     the posterior mean of the Poisson mid-p value of the observed count, GIVEN THE OBSERVED HISTORY (the currents
            are computed from the recorded spikes): exact for win = 1, an approximation for longer windows because spikes
            inside a window feed back into its rate.  NaN where a draw's expected count exceeds 700 or the observed count
            exceeds RW_MAX_COUNT = 1024.
"""
import numpy as np

from theano_pyglm_amd import _lib


def replicate_counts(population, x, n_rep, seed=0, rep0=0):
    """(counts (n_rep, N) int64, exceptions (n_rep) int64) of n_rep replicates of the current data set simulated at x.  Always
    on the device: X0, AW and the results stay there, the spike trains are never materialised."""
    import torch
    if population._time_shard is not None:
        raise ValueError("predictive counts of a time-sharded population are not implemented")
    data = population._current
    if data is None:
        raise ValueError("no current data set: add_data / set_data first")
    nT, N = np.asarray(data['S']).shape
    dt = population.glm.dt
    X0, AW = population._simulation_inputs(x, (0.0, nT * dt), dt, data.get('stim', None), data.get('dt_stim', None), nT=nT)
    AW = np.ascontiguousarray(np.transpose(AW, (0, 2, 1)))
    R = AW.shape[1]
    n_rep = int(n_rep)
    in_lds, ws_bytes = _lib.simulate_batch_plan(N, R)
    dev = torch.device('cuda:%d' % population.device)
    d_X0 = torch.from_numpy(X0).to(dev)
    d_AW = torch.from_numpy(AW).to(dev)
    d_counts = torch.empty((n_rep, N), dtype=torch.int64, device=dev)
    d_exc = torch.empty(n_rep, dtype=torch.int64, device=dev)
    d_ws = None if in_lds else torch.empty(n_rep * ws_bytes // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                               # (the uploads, before the library's launch on the null stream)
    _lib.simulate_batch_dev(N, nT, R, population.glm.nlin_model.kind, dt, d_X0.data_ptr(), d_AW.data_ptr(), n_rep,
                            d_counts.data_ptr(), d_exc.data_ptr(), seed=seed, rep0=rep0,
                            d_workspace=0 if d_ws is None else d_ws.data_ptr(), device=population.device)
    torch.cuda.synchronize(dev)
    return d_counts.cpu().numpy(), d_exc.cpu().numpy()


def summarize_counts(observed, counts):
    """Per-neuron summary of replicate counts (n_rep, N) against the observed counts (N): mean, std (ddof = 0), the central
    95 % interval (2.5 and 97.5 percentiles), and the two-sided predictive p-value from the rank of the observed count,
    p = min(1, 2 min(P(rep <= obs), P(rep >= obs))) with P the replicate frequencies."""
    observed = np.asarray(observed, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    lo, hi = np.percentile(counts, [2.5, 97.5], axis=0)
    le = np.mean(counts <= observed[None, :], axis=0)
    ge = np.mean(counts >= observed[None, :], axis=0)
    return {'observed': observed, 'mean': counts.mean(axis=0), 'std': counts.std(axis=0), 'lo': lo, 'hi': hi,
            'min': counts.min(axis=0), 'max': counts.max(axis=0), 'p_value': np.minimum(1.0, 2.0 * np.minimum(le, ge))}


def predictive_counts(population, x, n_rep, seed=0):
    """Predictive check of the spike counts of the population's current data under x.  Returns a dict of per-neuron arrays:
    observed, mean, std, lo / hi (central 95 % interval), min / max, p_value (two-sided, from the rank of the observed
    count among the replicates), plus counts (n_rep, N), exceptions (n_rep) and n_rep."""
    counts, exc = replicate_counts(population, x, n_rep, seed=seed)
    observed = np.asarray(population._current['S']).sum(axis=0).astype(np.int64)
    res = summarize_counts(observed, counts)
    res.update({'counts': counts, 'exceptions': exc, 'n_rep': int(n_rep)})
    return res


def ks_uniform(u):
    """KS distance of the values u from the uniform law on [0, 1] (NaN for an empty sample)"""
    u = np.sort(np.asarray(u, dtype=float))
    n = u.size
    if n == 0:
        return float('nan')
    return float(max(np.max(np.arange(1, n + 1) / n - u), np.max(u - np.arange(n) / n)))


def rate_bands(population, x, samples, win=50, n_lo=0, keep=False):
    """Posterior bands of the expected spike count of neurons n_lo .. n_lo + M over windows of `win` bins, and the windowed
    predictive residuals of the recorded counts, from the draws `samples`.

    samples: (S, M, P) rows in the theta layout, as waic_glms takes them (a leading chain axis is flattened; a torch device
    tensor is used where it is).  The other neurons and the network stay at x.  Per draw the rows overwrite a device copy of
    theta_matrix(x) and every data sequence gets one pgl_rate_windows_dev call; nothing synchronises with the host inside
    the loop.  Windows are counted from the start of each data sequence (the last one of a sequence may be short).
    Returns a dict of (n_win, M) arrays -- obs, mean, sd (n - 1 form; NaN for one draw), min, max, pit, pearson -- with t0
    (n_win) the windows' start times in seconds within their sequence, width (n_win) their lengths in seconds, and per
    neuron pit_ks (the KS distance of the finite pit values from the uniform law) and n_pit_nan; n_draws, win,
    windows_per_sequence, n_lo.  keep=True adds 'draws' (S, n_win, M), every draw's expected counts (for quantile bands),
    kept on the device until the end.  mean / width[:, None] is the firing rate in Hz."""
    from theano_pyglm_amd.inference.model_compare import _draw_loop
    win = int(win)
    if win < 1:
        raise ValueError("win must be at least 1")
    N, dt = population.N, population.glm.dt
    with _draw_loop(population, x, samples, n_lo, ("the rate bands", "are")) as (torch, dev, stream, handles, S, M, run):
        f64 = torch.float64
        nw = [h.rate_windows_count(win) for h in handles]
        off = np.concatenate(([0], np.cumsum(nw))).astype(int)
        accs = [torch.empty((_lib.RW_NACC, n, N), dtype=f64, device=dev) for n in nw]
        obss = [torch.empty((n, N), dtype=f64, device=dev) for n in nw]
        lam = torch.empty((S, int(off[-1]), N), dtype=f64, device=dev) if keep else None
        run(lambda i, k, h, theta, Weff: h.rate_windows_dev(theta, Weff, win, lam[i, off[k]:].data_ptr() if keep else 0,
                                                            obss[k].data_ptr() if i == 0 else 0, accs[k].data_ptr(), i))
        stream.synchronize()
        acc = np.concatenate([a.cpu().numpy() for a in accs], axis=1)[:, :, n_lo:n_lo + M]
        obs = np.concatenate([o.cpu().numpy() for o in obss], axis=0)[:, n_lo:n_lo + M]
        kept = np.ascontiguousarray(lam.cpu().numpy()[:, :, n_lo:n_lo + M]) if keep else None
    mean, m2, mn, mx, pit = acc
    with np.errstate(invalid='ignore', divide='ignore'):
        var = m2 / (S - 1.0) if S > 1 else np.full(m2.shape, np.nan)
        pearson = (obs - mean) / np.sqrt(mean + (var if S > 1 else 0.0))
    t0 = np.concatenate([np.arange(n) * (win * dt) for n in nw]) if nw else np.zeros(0)
    # (a sequence's last window may be short: its length is what is left of the sequence)
    width = np.full(t0.shape, win * dt)
    for k, data in enumerate(population.data_sequences):
        nT = int(np.asarray(data['S']).shape[0])
        if nw[k] > 0:
            width[off[k + 1] - 1] = (nT - (nw[k] - 1) * win) * dt
    fin = np.isfinite(pit)
    out = {'t0': t0, 'width': width, 'obs': np.ascontiguousarray(obs), 'mean': np.ascontiguousarray(mean),
           'sd': np.sqrt(var), 'min': np.ascontiguousarray(mn), 'max': np.ascontiguousarray(mx),
           'pit': np.ascontiguousarray(pit), 'pearson': pearson,
           'pit_ks': np.array([ks_uniform(pit[fin[:, m], m]) for m in range(M)]),
           'n_pit_nan': np.sum(~fin, axis=0).astype(np.int64), 'n_draws': S, 'win': win, 'windows_per_sequence': nw,
           'n_lo': int(n_lo)}
    if keep:
        out['draws'] = kept
    return out


def format_rate_table(res):
    """Per neuron: the largest |pearson| and its window, pit_ks, and the share of windows whose observed count lies outside
    the draws' [min, max]."""
    lines = ["windowed predictive residuals (%d draws, %d windows of %d bins)" % (res['n_draws'], len(res['t0']), res['win']),
             "%6s %12s %10s %10s %10s %12s" % ('neuron', 'max|pearson|', 'window', 'pit KS', 'pit NaN', 'outside band')]
    pe = np.where(np.isfinite(res['pearson']), np.abs(res['pearson']), -1.0)
    outside = np.mean((res['obs'] < res['min']) | (res['obs'] > res['max']), axis=0)
    for m in range(res['obs'].shape[1]):
        w = int(np.argmax(pe[:, m]))
        lines.append("%6d %12.3f %10d %10.4f %10d %11.1f%%" % (res['n_lo'] + m, pe[w, m], w, res['pit_ks'][m],
                                                               res['n_pit_nan'][m], 100.0 * outside[m]))
    lines.append("pit: conditional on the recorded history; exact for one-bin windows, approximate for longer ones")
    return "\n".join(lines)


def format_table(res):
    lines = ["predictive spike counts (%d replicates)" % res['n_rep'],
             "%6s %10s %12s %10s %10s %10s %8s" % ('neuron', 'observed', 'mean', 'std', '2.5%', '97.5%', 'p')]
    for n in range(len(res['observed'])):
        lines.append("%6d %10d %12.1f %10.1f %10.1f %10.1f %8.3f"
                     % (n, res['observed'][n], res['mean'][n], res['std'][n], res['lo'][n], res['hi'][n], res['p_value'][n]))
    inside = np.sum((res['observed'] >= res['lo']) & (res['observed'] <= res['hi']))
    lines.append("%d of %d neurons inside the central 95 %% interval" % (int(inside), len(res['observed'])))
    return "\n".join(lines)
