// Expected and observed spike counts of one time window of one neuron, folded over posterior draws, in the style of
// pglm_pointwise.h: the rule of one (window, neuron) and nothing else -- the caller (k_rw_window of pglm_ratewin.hip.h, one
// thread per (window, neuron); tests/csrc/ratewin_host.c on the host) owns the arrays.
//
// Windows: win >= 1 consecutive bins counted from the first bin of the range; the last one may be short:
//   n_win = ceil(n / win) for a range of n bins.
// Expected count of a window: Lam = dt * sum_t lam_t.  The order of the sum is part of the rule (it must not depend on the
// launch geometry): the window is cut into pieces of at most PGL_RW_PIECE = 256 bins counted from the window's OWN first bin;
// a piece is summed in ascending time from 0; the piece sums are added in ascending order from 0; dt multiplies last.
// Observed count y: the sum of the spike counts of the window's bins (exact in any order).
//
// The state over the draws Lam_0 .. Lam_{S-1} is five doubles:
//   mean   Welford's running mean:  d = Lam - mean;  mean += d / (s + 1);
//   M2     M2 = fma(d, Lam - mean, M2), the sum of squared deviations:  var = M2 / (S - 1)  (the fused form is spelt out so that
//          host and device round alike, whatever a compiler contracts);
//   min, max
//   pit    the running mean of the draw's mid-p predictive value  u_s = F(y - 1) + 0.5 f(y)  of the observed count under a
//          Poisson law of mean Lam_s:  term_0 = exp(-Lam), term_k = term_{k-1} * Lam / k, F(y - 1) = term_0 + .. + term_{y-1}
//          added in ascending k from 0, f(y) = term_y;  pit += (u - pit) / (s + 1).
//          u is NaN where Lam > PGL_RW_MAX_LAM = 700 (exp(-Lam) leaves the normal doubles soon after) or y > PGL_RW_MAX_COUNT =
//          1024 (the length of the loop): the pit of that (window, neuron) is then NaN for good and the other four values are
//          not affected.
// Draw s = 0 initialises the state (mean = min = max = Lam, M2 = 0, pit = u): the caller need not clear it.  A non-finite Lam
// (NaN or +-inf) makes the five values NaN, and NaN stays: a state that has met one says so (the mean is the witness).
//
// What pit is: the posterior mean of the one-step-ahead predictive probability of the observed window count GIVEN THE OBSERVED
// HISTORY (the currents are computed from the recorded spikes).  For win = 1 that is the exact conditional law of the bin's
// count; for longer windows it is an approximation, because spikes inside the window feed back into the rate of its later
// bins: the count of a window is then not Poisson with mean Lam.  Under a well-specified model the values are uniform on
// [0, 1] (mid-p: in mean and variance only for small counts).
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_RATEWIN_H
#define PGLM_RATEWIN_H

#include "pglm_hmc.h"

#define PGL_RW_FN PGL_HMC_FN
#define PGL_RW_NACC 5             // planes of the accumulator block (5, n_win, N): mean, M2, min, max, pit
#define PGL_RW_PIECE 256          // bins per piece of a window's sum
#define PGL_RW_MAX_COUNT 1024     // largest observed window count with a pit
#define PGL_RW_MAX_LAM 700.0      // largest expected window count with a pit

PGL_RW_FN long long pgl_rw_windows(long long n, long long win) { return (n + win - 1) / win; }

// pieces of a window of len bins
PGL_RW_FN long long pgl_rw_pieces(long long len) { return (len + PGL_RW_PIECE - 1) / PGL_RW_PIECE; }

// mid-p value of the count y (a non-negative integer as a double) under Poisson(lam), lam finite and >= 0
PGL_RW_FN double pgl_rw_midp(double lam, double y)
{
    if (!(lam <= PGL_RW_MAX_LAM) || !(y <= (double)PGL_RW_MAX_COUNT)) return __builtin_nan("");
    double term = exp(-lam), cdf = 0.0;
    const int n = (int)y;
    for (int k = 1; k <= n; ++k) {
        cdf += term;
        term = term * lam / (double)k;
    }
    return cdf + 0.5 * term;
}

PGL_RW_FN void pgl_rw_fold(double lam, double y, long long s, double* mean, double* m2, double* mn, double* mx, double* pit)
{
    if (!pgl_hmc_finite(lam) || (s > 0 && !pgl_hmc_finite(*mean))) {
        *mean = *m2 = *mn = *mx = *pit = __builtin_nan("");
        return;
    }
    const double u = pgl_rw_midp(lam, y);
    if (s == 0) {
        *mean = lam; *m2 = 0.0; *mn = lam; *mx = lam; *pit = u;
        return;
    }
    const double d = lam - *mean;
    const double m = *mean + d / (double)(s + 1);
    *mean = m;
    *m2 = fma(d, lam - m, *m2);
    if (lam < *mn) *mn = lam;
    if (lam > *mx) *mx = lam;
    *pit = *pit + (u - *pit) / (double)(s + 1);
}

#endif
