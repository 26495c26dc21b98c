"""
Goodness of fit of a fitted population by time rescaling (Brown, Barbieri, Ventura, Kass & Frank 2002).

Under the true model the integrated intensity tau_k between consecutive spikes of a neuron is Exp(1), so
z_k = 1 - exp(-tau_k) is uniform on [0, 1); a Kolmogorov-Smirnov test of the z_k against that law is the usual pass / fail.
The intervals come from the device (Population.compute_rescaled_intervals: one forward pass and a segmented sum per data
sequence); the sort and the KS statistic run here in numpy (device=False, the default of ks_time_rescaling) or on the
device (device=True and ks_time_rescaling_draws: pgl_ks_uniform_dev, a sorting network per neuron; only (N, 4) numbers come
back per parameter point).

Spikes are binned: a bin with several spikes counts as one event and the rate is summed over whole bins.  At high rates
(lam * dt not << 1) this biases the test: at lam * dt = 0.2 .. 0.5 a TRUE model has D about 0.2 and fails.
correct=True applies the discrete-time correction of Haslinger, Pipa & Brown (2010) to the event bin's term
(include/pyglm_hip.h, pgl_rescale_corr): it places the event inside its bin by a uniform number, so the corrected statistic
is a random function of `seed` (and of `draw`); the same seed gives the same bits.  correct=False is the default of the
single-point test, as before; the test over posterior draws corrects by default.
The reference has no counterpart (its result plots start from the rates of eval_state).
"""
import numpy as np


def ks_uniform(z):
    """sup |F_emp(z) - z| of a sample against the uniform law on [0, 1] (scipy.stats.kstest(z, 'uniform').statistic);
    NaN for an empty sample."""
    z = np.sort(np.asarray(z, dtype=float))
    n = z.size
    if n == 0:
        return np.nan
    d_plus = (np.arange(1.0, n + 1) / n - z).max()
    d_minus = (z - np.arange(0.0, n) / n).max()
    return float(max(d_plus, d_minus))


def ks_band(n, alpha=0.05):
    """Large-sample critical value of the KS statistic for n samples: 1.36 / sqrt(n) at alpha = 0.05, in general
    sqrt(-ln(alpha / 2) / 2) / sqrt(n)."""
    c = 1.36 if alpha == 0.05 else np.sqrt(-0.5 * np.log(alpha / 2.0))
    return c / np.sqrt(n) if n > 0 else np.nan


def ks_from_intervals(taus, alpha=0.05):
    """(D, band, passed, n_intervals) arrays over the neurons of a list of rescaled-interval arrays.  Fewer than two
    intervals: D = NaN, passed = False."""
    N = len(taus)
    D, band = np.full(N, np.nan), np.full(N, np.nan)
    passed = np.zeros(N, dtype=bool)
    cnt = np.zeros(N, dtype=np.int64)
    for n, tau in enumerate(taus):
        tau = np.asarray(tau, dtype=float)
        cnt[n] = tau.size
        if tau.size < 2:
            continue
        D[n] = ks_uniform(-np.expm1(-tau))
        band[n] = ks_band(tau.size, alpha)
        passed[n] = bool(D[n] <= band[n])
    return D, band, passed, cnt


def ks_sides(z):
    """(D+, D-) of ks_uniform; NaN for an empty sample"""
    z = np.sort(np.asarray(z, dtype=float))
    n = z.size
    if n == 0:
        return np.nan, np.nan
    return float((np.arange(1.0, n + 1) / n - z).max()), float((z - np.arange(0.0, n) / n).max())


def _bands(cnt, alpha):
    return np.array([ks_band(int(n), alpha) if n >= 2 else np.nan for n in cnt], dtype=float)


def _result(D, Dp, Dm, cnt, stats, alpha, route):
    band = _bands(cnt, alpha)
    passed = np.array([bool(d <= b) for d, b in zip(D, band)], dtype=bool)         # (NaN: False, as ks_from_intervals)
    return {'D': D, 'band': band, 'passed': passed, 'n_intervals': cnt, 'expected_count': stats[:, 0].copy(),
            'observed_count': np.rint(stats[:, 1]).astype(np.int64), 'multi_spike_bins': np.rint(stats[:, 2]).astype(np.int64),
            'alpha': alpha, 'D_plus': Dp, 'D_minus': Dm, 'route': route}


class _DeviceKs(object):
    """The device route of one parameter point after the other: per data sequence the (corrected) rescale into that
    sequence's buffer, the intervals gathered per neuron (torch indexing, layout only), pgl_ks_uniform_dev into a row of
    the caller's.  Nothing in point() synchronises with the host."""

    def __init__(self, torch, dev, handles, N):
        self.torch, self.handles, self.N = torch, handles, N
        f64 = torch.float64
        offs = [h.rescale_count() for h in handles]
        cnt = np.sum([np.diff(o) for o in offs], axis=0).astype(np.int64)
        self.cnt = cnt
        self.off = np.concatenate(([0], np.cumsum(cnt))).astype(np.int64)
        total = self.total = int(self.off[-1])
        self.totals = [int(o[-1]) for o in offs]
        self.d_offs = [torch.tensor(o, dtype=torch.int64, device=dev) for o in offs]
        self.d_off = torch.tensor(self.off, dtype=torch.int64, device=dev)
        self.taus = [torch.empty(max(int(o[-1]), 1), dtype=f64, device=dev) for o in offs]
        self.stats = [torch.empty((N, 4), dtype=f64, device=dev) for _ in handles]
        self.work = torch.empty(max(total, 1), dtype=f64, device=dev)
        self.index = None
        if len(handles) > 1:                         # neuron n: its intervals of sequence 0, of sequence 1, ..
            base = np.concatenate(([0], np.cumsum([int(o[-1]) for o in offs])))
            idx = [np.arange(o[n], o[n + 1]) + base[k] for n in range(N) for k, o in enumerate(offs)]
            self.index = torch.tensor(np.concatenate(idx) if total else np.zeros(0, dtype=np.int64), dtype=torch.int64, device=dev)
            self.gathered = torch.empty(max(total, 1), dtype=f64, device=dev)

    def point(self, theta, Weff, correct, seed, draw, ks_out, stats_out):
        """theta, Weff: device pointers; ks_out (N, 4), stats_out (N, 4): device tensors written"""
        for k, h in enumerate(self.handles):
            a = (theta, Weff, self.taus[k].data_ptr(), self.d_offs[k].data_ptr(), self.stats[k].data_ptr())
            if correct:
                h.rescale_corr_dev(*a, seed=seed, draw=draw)
            else:
                h.rescale_dev(*a)
        tau = self.taus[0]
        if self.index is not None:
            self.torch.index_select(self.torch.cat([t[:n] for t, n in zip(self.taus, self.totals)]), 0, self.index,
                                    out=self.gathered[:self.total])
            tau = self.gathered
        self.handles[0].ks_uniform(tau[:self.total], self.d_off, out=ks_out, zsorted=self.work)
        stats_out.copy_(self.stats[0])
        for st in self.stats[1:]:
            stats_out.add_(st)


def ks_time_rescaling(population, x, alpha=0.05, correct=False, seed=0, device=False, draw=0):
    """KS test of every neuron's rescaled inter-spike intervals under the parameters x on the population's data.
    Returns a dict of per-neuron arrays: D, band (1.36 / sqrt(n_intervals) at alpha = 0.05), passed (D <= band),
    n_intervals, expected_count (the integrated rate), observed_count (event bins), multi_spike_bins; D_plus, D_minus (the
    one-sided distances) and 'route' ('host' or 'device').  draw: the draw index of the uniforms (ks_time_rescaling_draws gives
    draw s to posterior draw s; a single point is draw 0).
    correct: the discrete-time correction at the uniforms of (seed, draw) -- the statistic is then a random function of
    seed.  device: the intervals of all data sequences stay on the device, are gathered per neuron there and go through
    pgl_ks_uniform_dev; only (N, 4) distances and the stats come back.  The default is the host route."""
    if not device:
        taus, stats = population.compute_rescaled_intervals(x, correct=correct, seed=seed, draw=draw) if correct else \
            population.compute_rescaled_intervals(x)
        cnt = np.array([len(t) for t in taus], dtype=np.int64)
        sides = np.array([ks_sides(-np.expm1(-np.asarray(t, dtype=float))) if len(t) >= 2 else (np.nan, np.nan) for t in taus])
        sides = sides.reshape(len(taus), 2)
        D = np.fmax(sides[:, 0], sides[:, 1])          # (ks_uniform's max(d_plus, d_minus): the same bits)
        return _result(D, sides[:, 0].copy(), sides[:, 1].copy(), cnt, stats, alpha, 'host')
    from theano_pyglm_amd.inference.lockstep import session
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("rescaled intervals of a time-sharded population are not implemented")
    population._check_vars(x)
    N = population.N
    theta0 = np.ascontiguousarray(population.theta_matrix(x))
    Weff0 = np.ascontiguousarray(population.W_eff(x))
    with session(population) as (torch, dev, stream, handles):
        f64 = torch.float64
        theta = torch.tensor(theta0, dtype=f64, device=dev)
        Weff = torch.tensor(Weff0, dtype=f64, device=dev)
        dk = _DeviceKs(torch, dev, handles, N)
        out = torch.empty((2, N, 4), dtype=f64, device=dev)
        dk.point(theta.data_ptr(), Weff.data_ptr(), correct, seed, draw, out[0], out[1])
        stream.synchronize()
        o = out.cpu().numpy()
    return _result(o[0, :, 0].copy(), o[0, :, 1].copy(), o[0, :, 2].copy(), dk.cnt.copy(), o[1], alpha, 'device')


def ks_time_rescaling_draws(population, x, samples, alpha=0.05, correct=True, seed=0, n_lo=0):
    """The posterior distribution of the KS distance: per posterior draw one forward pass, the (corrected) rescale with
    draw = s and the KS kernel on the device, into row s of a device matrix that is copied once at the end.

    samples: (S, M, P) rows of neurons n_lo .. n_lo + M in the theta layout, as sample_glms_hmc / sample_glms_nuts return
    them (a leading chain axis is flattened; a torch device tensor is used where it is), exactly as waic_glms takes them.
    The other neurons and the network stay at x.  Returns a dict: 'D' (S, M), 'D_mean', 'D_q05', 'D_q95' (M), 'band' (M),
    'pass_share' (the share of draws with D <= band), 'n_intervals' (M), 'expected_count_mean' (M), 'n_void' (M: the draws
    whose D is not finite -- a NaN or negative interval, a rate that overflowed; they are left out of D_mean and the quantiles
    and count as not passed), 'n_draws', 'alpha', 'seed', 'correct'.  With correct=True draw s uses its own uniforms: the spread of D over the draws holds the
    randomisation of the correction as well as the posterior's.  A time-sharded population raises."""
    from theano_pyglm_amd.inference.model_compare import _draw_loop
    N = population.N
    what = ("rescaled intervals", "are")
    with _draw_loop(population, x, samples, n_lo, what) as (torch, dev, stream, handles, S, M, run):
        f64 = torch.float64
        dk = _DeviceKs(torch, dev, handles, N)
        ks = torch.empty((S, N, 4), dtype=f64, device=dev)
        st = torch.empty((S, N, 4), dtype=f64, device=dev)

        def call(i, k, h, theta, Weff):
            if k == len(handles) - 1:                 # once per draw: the point covers every data sequence
                dk.point(theta, Weff, correct, seed, i, ks[i], st[i])
        run(call)
        stream.synchronize()
        ks_h, st_h = ks.cpu().numpy(), st.cpu().numpy()
    D = np.ascontiguousarray(ks_h[:, n_lo:n_lo + M, 0])
    cnt = dk.cnt[n_lo:n_lo + M].copy()
    band = _bands(cnt, alpha)
    with np.errstate(invalid='ignore'):
        share = np.mean(D <= band[None, :], axis=0)
    Dn = np.where(np.isfinite(D), D, np.nan)
    n_void = np.sum(np.isnan(Dn), axis=0).astype(np.int64)
    some = n_void < S                                 # (a neuron with fewer than two intervals is void in every draw)

    def over_draws(fn, *a):
        out = np.full(M, np.nan)
        if np.any(some):
            out[some] = fn(Dn[:, some], *a, axis=0)
        return out
    return {'D': D, 'D_mean': over_draws(np.nanmean), 'D_q05': over_draws(np.nanquantile, 0.05),
            'D_q95': over_draws(np.nanquantile, 0.95), 'band': band, 'pass_share': share, 'n_void': n_void, 'n_intervals': cnt,
            'expected_count_mean': st_h[:, n_lo:n_lo + M, 0].mean(axis=0), 'n_draws': S, 'alpha': alpha, 'seed': seed,
            'correct': bool(correct)}


def format_draws_table(res):
    lines = ["time-rescaling KS test over %d posterior draws (alpha = %g%s)"
             % (res['n_draws'], res['alpha'], ", discrete-time correction, seed %d" % res['seed'] if res['correct'] else ""),
             "%6s %10s %10s %10s %10s %8s %10s %12s" % ('neuron', 'D mean', 'D q05', 'D q95', 'band', 'pass', 'intervals', 'expected')]
    for n in range(len(res['D_mean'])):
        lines.append("%6d %10.4f %10.4f %10.4f %10.4f %7.0f%% %10d %12.1f"
                     % (n, res['D_mean'][n], res['D_q05'][n], res['D_q95'][n], res['band'][n], 100.0 * res['pass_share'][n],
                        res['n_intervals'][n], res['expected_count_mean'][n]))
    return "\n".join(lines)


def format_table(res):
    lines = ["time-rescaling KS test (alpha = %g)" % res['alpha'],
             "%6s %10s %10s %6s %10s %12s %10s %8s" % ('neuron', 'D', 'band', 'pass', 'intervals', 'expected', 'observed', 'multi')]
    for n in range(len(res['D'])):
        lines.append("%6d %10.4f %10.4f %6s %10d %12.1f %10d %8d"
                     % (n, res['D'][n], res['band'][n], 'yes' if res['passed'][n] else 'no', res['n_intervals'][n],
                        res['expected_count'][n], res['observed_count'][n], res['multi_spike_bins'][n]))
    lines.append("%d of %d neurons inside the band" % (int(np.sum(res['passed'])), len(res['D'])))
    return "\n".join(lines)
