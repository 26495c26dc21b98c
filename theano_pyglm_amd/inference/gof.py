"""
Goodness of fit of a fitted population by time rescaling (Brown, Barbieri, Ventura, Kass & Frank 2002).

Under the true model the integrated intensity tau_k between consecutive spikes of a neuron is Exp(1), so
z_k = 1 - exp(-tau_k) is uniform on [0, 1); a Kolmogorov-Smirnov test of the z_k against that law is the usual pass / fail.
The intervals come from the device (Population.compute_rescaled_intervals: one forward pass and a segmented sum per data
sequence); the sort and the KS statistic run here in numpy.

Spikes are binned: a bin with several spikes counts as one event and the rate is summed over whole bins.  At high rates
(lam * dt not << 1) this biases the test; the discrete-time correction of Haslinger, Pipa & Brown (2010) is not applied.
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


def ks_time_rescaling(population, x, alpha=0.05):
    """KS test of every neuron's rescaled inter-spike intervals under the parameters x on the population's data.
    Returns a dict of per-neuron arrays: D, band (1.36 / sqrt(n_intervals) at alpha = 0.05), passed (D <= band),
    n_intervals, expected_count (the integrated rate), observed_count (event bins), multi_spike_bins."""
    taus, stats = population.compute_rescaled_intervals(x)
    D, band, passed, cnt = ks_from_intervals(taus, alpha)
    return {'D': D, 'band': band, 'passed': passed, 'n_intervals': cnt, 'expected_count': stats[:, 0].copy(),
            'observed_count': np.rint(stats[:, 1]).astype(np.int64), 'multi_spike_bins': np.rint(stats[:, 2]).astype(np.int64),
            'alpha': alpha}


def format_table(res):
    lines = ["time-rescaling KS test (alpha = %g)" % res['alpha'],
             "%6s %10s %10s %6s %10s %12s %10s %8s" % ('neuron', 'D', 'band', 'pass', 'intervals', 'expected', 'observed', 'multi')]
    for n in range(len(res['D'])):
        lines.append("%6d %10.4f %10.4f %6s %10d %12.1f %10d %8d"
                     % (n, res['D'][n], res['band'][n], 'yes' if res['passed'][n] else 'no', res['n_intervals'][n],
                        res['expected_count'][n], res['observed_count'][n], res['multi_spike_bins'][n]))
    lines.append("%d of %d neurons inside the band" % (int(np.sum(res['passed'])), len(res['D'])))
    return "\n".join(lines)
