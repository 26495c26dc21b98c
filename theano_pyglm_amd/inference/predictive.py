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

Between the two: conditional_counts holds every OTHER neuron at its recorded spikes and simulates each neuron with only its own
history fed back (the single-neuron prediction given the population activity of Pillow et al. 2008; the rules: csrc/
pglm_condsim.h, restated below in numpy).  Its pit is the exact predictive law of a window's count for any window length --
conditional on the other neurons' recorded spikes -- and its residuals show where in time coupling plus self-history fail to
explain a neuron.
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


# ---- clamped simulation: each neuron given the others' recorded spikes ---------------------------------------------------
def cond_currents_numpy(X0, AW, S):
    """The clamped currents (csrc/pglm_condsim.h): Xc = X0 plus, for every recorded spike of a neuron p at a bin s, AW[p, tau, q]
    on the bins s + 1 + tau of every OTHER neuron q -- bins ascending, inside a bin p ascending, once per spike of the count
    (repeated addition), which is the order of the rule for every element.  X0 (nT, N), AW (N, R, N) [pre][tau][post],
    S (nT, N) counts."""
    Xc = np.array(X0, dtype=np.float64)
    S = np.asarray(S)
    nT, N = Xc.shape
    R = AW.shape[1]
    for s in range(nT):
        n = min(R, nT - s - 1)
        for p in np.flatnonzero(S[s]):
            others = np.arange(N) != p
            for _ in range(int(S[s, p])):
                Xc[s + 1:s + 1 + n, others] += AW[p, :n][:, others]
    return Xc


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


_G = np.uint64(0x9e3779b97f4a7c15)


def _thresholds(seed, reps, N, k):
    """-log u of the k-th draw (k (n_rep, N) uint64) of the streams (seed, r, n): the rule of include/pyglm_hip.h"""
    with np.errstate(over='ignore'):
        z = _mix(np.array([seed], dtype=np.uint64) + _G)
        z = _mix(z[:, None] + _G * (np.asarray(reps, dtype=np.uint64)[:, None] + np.uint64(1)))
        key = _mix(z + _G * (np.arange(N, dtype=np.uint64)[None, :] + np.uint64(1)))
        z = _mix(key + _G * (k + np.uint64(1)))
    return -np.log(((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53)


def simulate_cond_numpy(Xc, AW, nlin, dt, n_rep, seed=0, rep0=0):
    """The chains (replicate r, neuron n) of the clamped simulation, all at once: pgl_simulate_streams' loop for neurons that
    are alone.  Only AW[n, :, n] is read.  Returns (S (n_rep, nT, N) uint8, exceptions (N) int64 summed over the replicates).
    The cap of 10 spikes per bin is each chain's own: a round that starts at 10 is dropped (recorded, not scattered)."""
    nT, N = Xc.shape
    R = AW.shape[1]
    h = np.ascontiguousarray(AW[np.arange(N), :, np.arange(N)].T)                       # (R, N): h[tau, n] = AW[n, tau, n]
    f = (lambda v: np.exp(v)) if nlin in ('exp', 0) else (lambda v: np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v))))
    reps = rep0 + np.arange(n_rep)
    X = np.repeat(np.asarray(Xc, dtype=np.float64)[None], n_rep, axis=0)
    k = np.zeros((n_rep, N), dtype=np.uint64)
    thr = _thresholds(seed, reps, N, k)
    k += np.uint64(1)
    acc = np.zeros((n_rep, N))
    S = np.zeros((n_rep, nT, N), dtype=np.uint8)
    exc = np.zeros(N, dtype=np.int64)
    for t in range(nT):
        acc += f(X[:, t]) * dt
        spk = acc > thr
        S[:, t][spk] += 1
        n = min(R, nT - t - 1)
        while spk.any():
            capped = spk & (S[:, t] >= 10)
            exc += capped.sum(axis=0)
            spk &= ~capped                                                          # a dropped round ends the chain's bin
            ri, ni = np.nonzero(spk)
            X[ri, t + 1:t + 1 + n, ni] += h[:n, ni].T
            acc[spk] -= thr[spk]
            thr[spk] = _thresholds(seed, reps, N, k)[spk]
            k[spk] += np.uint64(1)
            np.maximum(acc, 0.0, out=acc, where=spk)
            spk = spk & (acc > thr)
            S[:, t][spk] += 1
    return S, exc


def cond_accumulate_numpy(S, obs, win, acc=None):
    """The six planes (sum c, sum c^2, #(c < obs), #(c = obs), min c, max c), (6, n_win, N) int64, of the replicates' window
    counts c from S (n_rep, nT, N); folded onto acc where given."""
    c = np.stack([_lib.window_counts(s, win) for s in S])                             # (n_rep, n_win, N)
    new = np.stack([c.sum(axis=0), (c * c).sum(axis=0), (c < obs[None]).sum(axis=0), (c == obs[None]).sum(axis=0),
                    c.min(axis=0), c.max(axis=0)]).astype(np.int64)
    if acc is None:
        return new
    return np.concatenate([acc[:4] + new[:4], np.minimum(acc[4:5], new[4:5]), np.maximum(acc[5:6], new[5:6])])


def _cond_draws(population, x, samples, n_draws):
    """the parameter sets of a conditional check: x itself, or n_draws evenly spaced draws of a sampler's result written into x"""
    if samples is None:
        return [x]
    from theano_pyglm_amd.inference.batched_hmc import samples_to_states
    if isinstance(samples, dict):
        samples = samples['samples']
    if hasattr(samples, 'cpu'):
        samples = samples.cpu().numpy()
    s = np.asarray(samples, dtype=np.float64)
    s = s.reshape((-1,) + s.shape[-2:])
    if s.ndim != 3 or s.shape[1] != population.N:
        raise ValueError("samples must be (n, N, P) draws of all neurons")
    idx = np.unique(np.round(np.linspace(0, s.shape[0] - 1, min(int(n_draws), s.shape[0]))).astype(int))
    out = []
    for i in idx:
        xi = dict(x)
        xi['glms'] = samples_to_states(population, x, s, int(i))
        out.append(xi)
    return out


def conditional_counts(population, x, n_rep=256, win=50, samples=None, n_draws=8, seed=0, rep0=0, keep_counts=False,
                       device=True):
    """Clamped predictive check of the current data under x: every neuron simulated n_rep times with its own spikes fed back
    and the other neurons held at their recorded spikes; windows of `win` bins from bin 0 (the last may be short).

    Uploads X0, AW and the event lists, runs k_cond_currents and k_simulate_cond and brings back the accumulators (and the
    replicates' total counts, n_rep x N integers).  With `samples` (a sampler's result dict or (n, N, P) draws; a chain axis is
    flattened) it takes n_draws evenly spaced draws and runs n_rep replicates of each: draw i uses the stream indices rep0 +
    i n_rep .., the accumulators continue across the calls; X0 and AW of a draw come from the host's _simulation_inputs.
    device=False is the numpy statement of both rules (cond_currents_numpy, simulate_cond_numpy): slow, for checking.

    Returns a dict.  Per (window, neuron), (n_win, N): obs, mean, sd (n - 1 form; NaN for one replicate), min, max,
    pit = (n_less + n_equal / 2) / replicates -- the mid-p predictive value of the recorded count, exact for any window length
    but CONDITIONAL on the other neurons' recorded spikes, and for small counts uniform in mean and variance only --,
    pearson = (obs - mean) / sd (NaN where sd = 0).  t0, width (n_win) in seconds.  Per neuron: pit_ks, exceptions (dropped
    rounds at the neuron's own cap of 10 spikes per bin), total (summarize_counts of the replicates' total counts).  acc
    (6, n_win, N) int64, n_rep (all replicates), n_draws, win, fallbacks (chains whose queue of own spikes overflowed; None on
    the host route); keep_counts adds counts (replicates, N)."""
    if population._time_shard is not None:
        raise ValueError("conditional counts of a time-sharded population are not implemented")
    data = population._current
    if data is None:
        raise ValueError("no current data set: add_data / set_data first")
    n_rep, win = int(n_rep), int(win)
    if win < 1 or n_rep < 1:
        raise ValueError("win and n_rep must be at least 1")
    S_obs = np.asarray(data['S'])
    nT, N = S_obs.shape
    dt = population.glm.dt
    kind = population.glm.nlin_model.kind
    obs = _lib.window_counts(S_obs, win)
    n_win = obs.shape[0]
    draws = _cond_draws(population, x, samples, n_draws)

    def inputs(xi):
        X0, AW = population._simulation_inputs(xi, (0.0, nT * dt), dt, data.get('stim', None), data.get('dt_stim', None), nT=nT)
        return X0, np.ascontiguousarray(np.transpose(AW, (0, 2, 1)))

    counts = []
    if device:
        import torch
        dev = torch.device('cuda:%d' % population.device)
        ev_pre, ev_cnt, bin_off = _lib.spike_events(S_obs)
        d_pre = torch.from_numpy(ev_pre).to(dev)
        d_cnt = torch.from_numpy(ev_cnt).to(dev)
        d_off = torch.from_numpy(bin_off).to(dev)
        d_obs = torch.from_numpy(obs).to(dev)
        d_Xc = torch.empty((nT, N), dtype=torch.float64, device=dev)
        d_acc = torch.empty((_lib.CS_NACC, n_win, N), dtype=torch.int64, device=dev)
        d_exc = torch.empty(N, dtype=torch.int64, device=dev)
        d_fb = torch.empty(1, dtype=torch.int64, device=dev)
        d_counts = torch.empty((len(draws), n_rep, N), dtype=torch.int64, device=dev)
        d_ws = None
        for i, xi in enumerate(draws):
            X0, AW = inputs(xi)
            R = AW.shape[1]
            d_X0 = torch.from_numpy(X0).to(dev)
            d_AW = torch.from_numpy(AW).to(dev)
            if d_ws is None:
                d_ws = torch.empty(_lib.simulate_cond_workspace(N, R, n_rep) // 8, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)                       # (the uploads, before the library's launches on the null stream)
            _lib.cond_currents_dev(N, nT, R, d_X0, d_AW, d_pre, d_cnt, d_off, d_Xc, device=population.device)
            _lib.simulate_cond_dev(N, nT, R, kind, dt, d_Xc, d_AW, d_obs, win, n_rep, d_acc, d_exc, d_ws, seed=seed,
                                   rep0=rep0 + i * n_rep, accumulate=i > 0, d_counts=d_counts[i], d_fallbacks=d_fb,
                                   device=population.device)
            torch.cuda.synchronize(dev)                       # (d_X0 / d_AW of this draw are released next)
        acc = d_acc.cpu().numpy()
        exc = d_exc.cpu().numpy()
        fallbacks = int(d_fb.cpu().numpy()[0])
        counts = d_counts.cpu().numpy().reshape(-1, N)
    else:
        acc, exc, fallbacks = None, np.zeros(N, dtype=np.int64), None
        for i, xi in enumerate(draws):
            X0, AW = inputs(xi)
            S, e = simulate_cond_numpy(cond_currents_numpy(X0, AW, S_obs), AW, kind, dt, n_rep, seed=seed, rep0=rep0 + i * n_rep)
            acc = cond_accumulate_numpy(S, obs, win, acc)
            exc += e
            counts.append(S.sum(axis=1, dtype=np.int64))
        counts = np.concatenate(counts)
    res = cond_summary(acc, obs, n_rep * len(draws))
    width = np.full(n_win, win * dt)
    width[-1] = (nT - (n_win - 1) * win) * dt
    res.update({'t0': np.arange(n_win) * (win * dt), 'width': width, 'exceptions': exc, 'fallbacks': fallbacks,
                'total': summarize_counts(S_obs.sum(axis=0).astype(np.int64), counts), 'n_draws': len(draws), 'win': win})
    if keep_counts:
        res['counts'] = counts
    return res


def cond_summary(acc, obs, n):
    """obs, mean, sd, min, max, pit, pearson (n_win, N) and pit_ks (N) from the six planes of n replicates"""
    s1, s2, less, equal, mn, mx = [np.asarray(a, dtype=np.int64) for a in acc]
    mean = s1 / float(n)
    with np.errstate(invalid='ignore', divide='ignore'):
        # (n s2 - s1^2 in integers: exact, no cancellation)
        sd = np.sqrt((n * s2 - s1 * s1) / float(n * (n - 1))) if n > 1 else np.full(mean.shape, np.nan)
        pearson = np.where(sd > 0, (obs - mean) / sd, np.nan)
    pit = (less + 0.5 * equal) / float(n)
    return {'obs': np.asarray(obs, dtype=np.int64), 'mean': mean, 'sd': sd, 'min': mn, 'max': mx, 'pit': pit, 'pearson': pearson,
            'pit_ks': np.array([ks_uniform(pit[:, m]) for m in range(pit.shape[1])]), 'acc': np.asarray(acc), 'n_rep': int(n)}


def format_cond_table(res):
    """Per neuron: the largest |pearson| and its window, pit_ks, and the share of windows whose observed count lies outside
    the replicates' [min, max]."""
    lines = ["clamped predictive residuals (%d replicates, %d windows of %d bins)" % (res['n_rep'], len(res['t0']), res['win']),
             "%6s %12s %10s %10s %10s %12s" % ('neuron', 'max|pearson|', 'window', 'pit KS', 'exceptions', 'outside band')]
    pe = np.where(np.isfinite(res['pearson']), np.abs(res['pearson']), -1.0)
    outside = np.mean((res['obs'] < res['min']) | (res['obs'] > res['max']), axis=0)
    for m in range(res['obs'].shape[1]):
        w = int(np.argmax(pe[:, m]))
        lines.append("%6d %12.3f %10d %10.4f %10d %11.1f%%" % (m, pe[w, m], w, res['pit_ks'][m], res['exceptions'][m],
                                                               100.0 * outside[m]))
    lines.append("pit: exact for any window length, conditional on the other neurons' recorded spikes")
    return "\n".join(lines)
