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

The KS distance tests the marginal law only.  Under the true model the intervals are also INDEPENDENT; missing refractoriness,
an impulse response that is too short or an unmodelled slow drift leave the marginal law nearly uniform and make consecutive
intervals correlated.  independence_time_rescaling is the companion check: the serial correlation r_k of the normal scores
g = Phi^-1(z) at the lags 1 .. L with the band z_{1-alpha/2} sqrt(v_k), and the portmanteau statistic Q (Ljung-Box where a
neuron has one data sequence) against chi-square with dof degrees of freedom.  The rule -- scores, sums in pieces of 256,
pairs that never cross from one data sequence into the next -- is csrc/pglm_acf.h; acf_scores states it in numpy (the host
route), pgl_rescale_acf_dev runs it on the device (device=True and independence_time_rescaling_draws).  The first interval
of each sequence is censored, so a run starts at the sequence's second event.  With correct=True the statistic is a random
function of `seed`, and uncorrected intervals at lam * dt not << 1 are biased here as they are for the KS distance.
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


def ks_pvalue(D, n):
    """Two-sided p-value of the KS distance D of n samples, elementwise: scipy's exact law scipy.stats.kstwo.sf(D, n) where
    the installed scipy has it, else the asymptotic kstwobign.sf((sqrt(n) + 0.12 + 0.11 / sqrt(n)) D) (Stephens 1970).  NaN
    where D is not finite or n < 1."""
    from scipy import stats
    D, n = np.broadcast_arrays(np.asarray(D, dtype=float), np.asarray(n, dtype=float))
    p = np.full(D.shape, np.nan)
    ok = np.isfinite(D) & (n >= 1)
    if np.any(ok):
        if hasattr(stats, 'kstwo'):
            p[ok] = stats.kstwo.sf(D[ok], np.rint(n[ok]).astype(np.int64))
        else:
            rn = np.sqrt(n[ok])
            p[ok] = stats.kstwobign.sf((rn + 0.12 + 0.11 / rn) * D[ok])
    return p


def _result(D, Dp, Dm, cnt, stats, alpha, route):
    band = _bands(cnt, alpha)
    passed = np.array([bool(d <= b) for d, b in zip(D, band)], dtype=bool)         # (NaN: False, as ks_from_intervals)
    return {'D': D, 'band': band, 'passed': passed, 'n_intervals': cnt, 'expected_count': stats[:, 0].copy(),
            'observed_count': np.rint(stats[:, 1]).astype(np.int64), 'multi_spike_bins': np.rint(stats[:, 2]).astype(np.int64),
            'alpha': alpha, 'D_plus': Dp, 'D_minus': Dm, 'route': route, 'p_value': ks_pvalue(D, cnt)}


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
        self.offs, self.d_run_off = offs, None
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

    def _intervals(self, theta, Weff, correct, seed, draw, stats_out):
        """the (corrected) intervals of every data sequence, gathered per neuron: a device vector of self.total values"""
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
        stats_out.copy_(self.stats[0])
        for st in self.stats[1:]:
            stats_out.add_(st)
        return tau[:self.total]

    def point(self, theta, Weff, correct, seed, draw, ks_out, stats_out):
        """theta, Weff: device pointers; ks_out (N, 4), stats_out (N, 4): device tensors written"""
        tau = self._intervals(theta, Weff, correct, seed, draw, stats_out)
        self.handles[0].ks_uniform(tau, self.d_off, out=ks_out, zsorted=self.work)

    def acf_point(self, theta, Weff, correct, seed, draw, max_lag, acf_out, stats_out):
        """the same for the serial correlation of the normal scores: acf_out (N, 6 + max_lag).  The runs of neuron n are its
        intervals of sequence 0, of sequence 1, ..: the gathered layout, with the offsets rescale_count gave."""
        if self.d_run_off is None:
            K = len(self.offs)
            lens = np.stack([np.diff(o) for o in self.offs], axis=1).reshape(-1)           # (neuron, sequence)
            self.run_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
            self.seg_run = (np.arange(self.N + 1) * K).astype(np.int64)
            self.d_run_off = self.torch.tensor(self.run_off, dtype=self.torch.int64, device=self.work.device)
            self.d_seg_run = self.torch.tensor(self.seg_run, dtype=self.torch.int64, device=self.work.device)
        tau = self._intervals(theta, Weff, correct, seed, draw, stats_out)
        self.handles[0].rescale_acf(tau, self.d_run_off, self.d_seg_run, max_lag, out=acf_out, scores=self.work)


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
            'correct': bool(correct), 'p_value': ks_pvalue(D, cnt[None, :])}


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


# ---- independence of the rescaled intervals -------------------------------------------------------------------------------
ACF_PIECE = 256                     # PGL_ACF_PIECE
ACF_NHEAD = 6                       # PGL_ACF_NHEAD
ACF_MAX_LAG = 64                    # PGL_ACF_MAX_LAG
_LN2_HI, _LN2_LO = 0.6931471805599453094, 2.319046813846299558e-17
_DBL_MIN = np.finfo(float).tiny

_A = (3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
      4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
_B = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4,
      3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, u):
    v = np.full_like(u, c[-1])
    for a in c[-2::-1]:
        v = v * u + a
    return v


def normal_scores(tau):
    """g = Phi^-1(1 - exp(-tau)) by the rule of csrc/pglm_acf.h (AS 241 PPND16): the central branch on z - 1/2 evaluated without
    the cancellation at tau = log 2, the tail branches on the nearer tail's own probability (the upper one is exp(-tau), not
    1 - z), clamped at the smallest normal double."""
    tau = np.asarray(tau, dtype=float)
    g = np.full(tau.shape, np.nan)
    with np.errstate(all='ignore'):
        z = -np.expm1(-tau)
        q = z - 0.5
        mid = np.abs(q) <= 0.425
        qq = -0.5 * np.expm1((_LN2_HI - tau[mid]) + _LN2_LO)
        u = 0.180625 - qq * qq
        g[mid] = qq * _horner(_A, u) / _horner(_B, u)
        tail = ~mid & ~np.isnan(tau)
        r = np.where(q[tail] < 0.0, z[tail], np.exp(-tau[tail]))
        r = np.where(r < _DBL_MIN, _DBL_MIN, r)
        u = np.sqrt(-np.log(r))
        near = u <= 5.0
        v = np.where(near, _horner(_C, u - 1.6) / _horner(_D, u - 1.6), _horner(_E, u - 5.0) / _horner(_F, u - 5.0))
        g[tail] = np.where(q[tail] < 0.0, -v, v)
    return g


def _piece_sum(terms):
    """the rule's sum of terms[0 .. n): pieces of 256 from the first element, ascending inside a piece, then the piece totals
    ascending (np.add.accumulate adds strictly in order; a skipped term is a +0.0)"""
    n = terms.size
    if n == 0:
        return 0.0
    npc = -(-n // ACF_PIECE)
    t = np.zeros(npc * ACF_PIECE)
    t[:n] = terms
    return float(np.add.accumulate(np.add.accumulate(t.reshape(npc, ACF_PIECE), axis=1)[:, -1])[-1])


def acf_from_scores(scores_runs, max_lag, void=None):
    """The statistics of the rule from given scores: scores_runs[m] is the list of the runs of segment m (arrays of scores,
    consecutive in time inside a run).  void[m]: the segment held a NaN or negative tau.  -> (M, 6 + max_lag):
    n, mean, c_0, Q, dof, 0, r_1 .. r_L."""
    L = int(max_lag)
    if not 1 <= L <= ACF_MAX_LAG:
        raise ValueError("max_lag must lie in 1 .. %d" % ACF_MAX_LAG)
    out = np.full((len(scores_runs), ACF_NHEAD + L), np.nan)
    for m, runs in enumerate(scores_runs):
        runs = [np.asarray(r, dtype=float).ravel() for r in runs]
        g = np.concatenate(runs) if runs else np.zeros(0)
        n = g.size
        out[m, 0] = n
        if void is not None and void[m]:
            continue
        out[m, 5] = 0.0
        end = np.concatenate([np.full(r.size, e) for r, e in zip(runs, np.cumsum([r.size for r in runs]))]) if n else np.zeros(0)
        with np.errstate(all='ignore'):
            mean = np.float64(_piece_sum(g)) / np.float64(n)
        d = g - mean
        c0 = _piece_sum(d * d)
        out[m, 1], out[m, 2], out[m, 4] = mean, c0, 0.0
        if n < 3 or c0 == 0.0:
            continue
        nn = float(n) * (float(n) + 2.0)
        Q, dof = 0.0, 0
        i = np.arange(n)
        for k in range(1, L + 1):
            ok = i + k < end
            nk = int(np.sum(ok))
            if nk < 1:
                continue
            prod = np.zeros(n)
            prod[ok] = d[ok] * d[i[ok] + k]
            r = _piece_sum(prod) / c0
            v = float(nk) / nn
            Q = Q + (r * r) / v
            dof += 1
            out[m, ACF_NHEAD + k - 1] = r
        out[m, 3], out[m, 4] = Q, float(dof)
    return out


def acf_scores(taus_runs, max_lag):
    """The independence rule of csrc/pglm_acf.h in numpy -- same pieces, same order: taus_runs[m] is the list of the runs of
    segment m (arrays of rescaled intervals).  -> (M, 6 + max_lag) as pgl_rescale_acf: n, mean, c_0, Q, dof, 0, r_1 .. r_L."""
    runs = [[np.asarray(r, dtype=float).ravel() for r in seg] for seg in taus_runs]
    void = [any(bool(np.any(~(r >= 0.0))) for r in seg) for seg in runs]
    return acf_from_scores([[normal_scores(r) for r in seg] for seg in runs], max_lag, void)


def _independence_result(acf, stats, max_lag, alpha, route):
    from scipy import special, stats as sstats
    L = int(max_lag)
    n = acf[:, 0]
    r = acf[:, ACF_NHEAD:ACF_NHEAD + L].copy()
    Q, dof = acf[:, 3].copy(), acf[:, 4].copy()
    cnt = np.rint(n).astype(np.int64)
    with np.errstate(all='ignore'):
        # (the block does not carry n_k: the caller counts the pairs inside runs from the run lengths, which it knows)
        v = stats['n_pairs'] / (n * (n + 2.0))[:, None]
        band = sstats.norm.ppf(1.0 - alpha / 2.0) * np.sqrt(v)
        band = np.where(np.isfinite(r), band, np.nan)
        outside = np.sum(np.abs(r) > band, axis=1).astype(np.int64)
        p = np.where(dof >= 1, special.gammaincc(np.where(dof >= 1, dof, 1.0) / 2.0, Q / 2.0), np.nan)
        var = np.where(n > 1, acf[:, 2] / (n - 1.0), np.nan)
    passed = np.array([bool(x >= alpha) for x in p], dtype=bool)                     # (NaN: False)
    return {'r': r, 'r_band': band, 'n_outside': outside, 'Q': Q, 'dof': np.where(np.isnan(dof), 0, dof).astype(np.int64),
            'p_value': p, 'passed': passed, 'n_intervals': cnt, 'mean_score': acf[:, 1].copy(), 'var_score': var, 'alpha': alpha,
            'route': route, 'max_lag': L}


def _pair_counts(run_lens, max_lag):
    """n_k (segments, L) from the run lengths of every segment: sum over its runs of max(len - k, 0)"""
    k = np.arange(1, int(max_lag) + 1)
    return np.array([np.sum(np.maximum(np.asarray(ls, dtype=np.int64)[:, None] - k[None, :], 0), axis=0) if len(ls) else
                     np.zeros(k.size, dtype=np.int64) for ls in run_lens], dtype=float).reshape(len(run_lens), k.size)


def independence_time_rescaling(population, x, max_lag=20, alpha=0.05, correct=False, seed=0, draw=0, device=False):
    """Independence test of every neuron's rescaled intervals under the parameters x: the serial correlation of their normal
    scores at the lags 1 .. max_lag.  Returns a dict of per-neuron arrays: 'r' (N, L), 'r_band' (N, L) = z_{1-alpha/2}
    sqrt(v_k), 'n_outside' (the lags with |r_k| beyond the band), 'Q', 'dof', 'p_value' = gammaincc(dof / 2, Q / 2), 'passed'
    (p_value >= alpha; NaN: False), 'n_intervals', 'mean_score', 'var_score' (c_0 / (n - 1)), and 'alpha', 'route'.
    Pairs never cross from one data sequence into the next.  correct, seed, draw: as ks_time_rescaling -- with correct=True
    the statistic is a random function of seed.  device: the intervals stay on the device (pgl_rescale_acf_dev); only the
    (N, 6 + max_lag) block and the stats come back.  A time-sharded population raises."""
    L = int(max_lag)
    if not 1 <= L <= ACF_MAX_LAG:
        raise ValueError("max_lag must lie in 1 .. %d" % ACF_MAX_LAG)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("rescaled intervals of a time-sharded population are not implemented")
    N = population.N
    if not device:
        runs = [[] for _ in range(N)]
        call = (lambda h, theta, Weff: h.rescale_corr(theta, Weff, seed, draw)) if correct else \
            (lambda h, theta, Weff: h.rescale(theta, Weff))
        for tau, off, st in population._per_sequence(x, ("rescaled intervals", "are"), call):
            for n in range(N):
                runs[n].append(np.asarray(tau[off[n]:off[n + 1]], dtype=float))
        acf = acf_scores(runs, L)
        pairs = _pair_counts([[r.size for r in seg] for seg in runs], L)
        return _independence_result(acf, {'n_pairs': pairs}, L, alpha, 'host')
    from theano_pyglm_amd.inference.lockstep import session
    population._check_vars(x)
    theta0 = np.ascontiguousarray(population.theta_matrix(x))
    Weff0 = np.ascontiguousarray(population.W_eff(x))
    with session(population) as (torch, dev, stream, handles):
        f64 = torch.float64
        theta = torch.tensor(theta0, dtype=f64, device=dev)
        Weff = torch.tensor(Weff0, dtype=f64, device=dev)
        dk = _DeviceKs(torch, dev, handles, N)
        out = torch.empty((N, ACF_NHEAD + L), dtype=f64, device=dev)
        st = torch.empty((N, 4), dtype=f64, device=dev)
        dk.acf_point(theta.data_ptr(), Weff.data_ptr(), correct, seed, draw, L, out, st)
        stream.synchronize()
        o = out.cpu().numpy()
    pairs = _pair_counts([[int(o_[n + 1] - o_[n]) for o_ in dk.offs] for n in range(N)], L)
    return _independence_result(o, {'n_pairs': pairs}, L, alpha, 'device')


def independence_time_rescaling_draws(population, x, samples, max_lag=20, alpha=0.05, correct=True, seed=0, n_lo=0):
    """The posterior distribution of the independence statistic: per posterior draw one forward pass, the (corrected) rescale
    with draw = s and the ACF kernel on the device, into row s of a device block that is copied once at the end.  samples as
    ks_time_rescaling_draws takes them.  Returns a dict: 'Q', 'r1', 'p_value' (S, M), 'pass_share' (the share of draws with
    p_value >= alpha; a void draw counts as not passed), 'r1_mean', 'r1_q05', 'r1_q95' (M, over the draws that are not void),
    'n_void' (M: the draws whose Q is not finite), 'n_intervals' (M), 'n_draws', 'alpha', 'seed', 'correct'.  With correct=True
    draw s uses its own uniforms.  A time-sharded population raises."""
    from scipy import special
    from theano_pyglm_amd.inference.model_compare import _draw_loop
    L = int(max_lag)
    if not 1 <= L <= ACF_MAX_LAG:
        raise ValueError("max_lag must lie in 1 .. %d" % ACF_MAX_LAG)
    N = population.N
    what = ("rescaled intervals", "are")
    with _draw_loop(population, x, samples, n_lo, what) as (torch, dev, stream, handles, S, M, run):
        f64 = torch.float64
        dk = _DeviceKs(torch, dev, handles, N)
        acf = torch.empty((S, N, ACF_NHEAD + L), dtype=f64, device=dev)
        st = torch.empty((N, 4), dtype=f64, device=dev)

        def call(i, k, h, theta, Weff):
            if k == len(handles) - 1:                 # once per draw: the point covers every data sequence
                dk.acf_point(theta, Weff, correct, seed, i, L, acf[i], st)
        run(call)
        stream.synchronize()
        a = acf.cpu().numpy()[:, n_lo:n_lo + M]
    Q = np.ascontiguousarray(a[:, :, 3])
    r1 = np.ascontiguousarray(a[:, :, ACF_NHEAD])
    dof = a[:, :, 4]
    with np.errstate(all='ignore'):
        p = np.where(dof >= 1, special.gammaincc(np.where(dof >= 1, dof, 1.0) / 2.0, Q / 2.0), np.nan)
        share = np.mean(p >= alpha, axis=0)
    n_void = np.sum(~np.isfinite(Q), axis=0).astype(np.int64)
    some = n_void < S
    r1n = np.where(np.isfinite(Q), r1, np.nan)

    def over_draws(fn, *args):
        out = np.full(M, np.nan)
        if np.any(some):
            out[some] = fn(r1n[:, some], *args, axis=0)
        return out
    return {'Q': Q, 'r1': r1, 'p_value': p, 'pass_share': share, 'r1_mean': over_draws(np.nanmean),
            'r1_q05': over_draws(np.nanquantile, 0.05), 'r1_q95': over_draws(np.nanquantile, 0.95), 'n_void': n_void,
            'n_intervals': dk.cnt[n_lo:n_lo + M].copy(), 'n_draws': S, 'alpha': alpha, 'seed': seed, 'correct': bool(correct),
            'max_lag': L}


def format_independence_table(res):
    L = res['r'].shape[1]
    lines = ["time-rescaling independence test: serial correlation of the normal scores, lags 1 .. %d (alpha = %g)" % (L, res['alpha']),
             "%6s %10s %10s %8s %10s %5s %10s %6s %10s" % ('neuron', 'r_1', 'band_1', 'outside', 'Q', 'dof', 'p', 'pass', 'intervals')]
    for n in range(len(res['Q'])):
        lines.append("%6d %10.4f %10.4f %8d %10.2f %5d %10.4f %6s %10d"
                     % (n, res['r'][n, 0], res['r_band'][n, 0], res['n_outside'][n], res['Q'][n], res['dof'][n], res['p_value'][n],
                        'yes' if res['passed'][n] else 'no', res['n_intervals'][n]))
    lines.append("%d of %d neurons pass" % (int(np.sum(res['passed'])), len(res['Q'])))
    return "\n".join(lines)


def format_independence_draws_table(res):
    lines = ["time-rescaling independence test over %d posterior draws, lags 1 .. %d (alpha = %g%s)"
             % (res['n_draws'], res['max_lag'], res['alpha'],
                ", discrete-time correction, seed %d" % res['seed'] if res['correct'] else ""),
             "%6s %10s %10s %10s %10s %8s %6s %10s" % ('neuron', 'r_1 mean', 'r_1 q05', 'r_1 q95', 'Q median', 'pass', 'void', 'intervals')]
    with np.errstate(all='ignore'):
        Qn = np.where(np.isfinite(res['Q']), res['Q'], np.nan)
        med = np.array([np.nanmedian(Qn[:, m]) if np.any(np.isfinite(Qn[:, m])) else np.nan for m in range(Qn.shape[1])])
    for n in range(len(res['r1_mean'])):
        lines.append("%6d %10.4f %10.4f %10.4f %10.2f %7.0f%% %6d %10d"
                     % (n, res['r1_mean'][n], res['r1_q05'][n], res['r1_q95'][n], med[n], 100.0 * res['pass_share'][n],
                        res['n_void'][n], res['n_intervals'][n]))
    return "\n".join(lines)
