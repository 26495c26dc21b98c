// Posterior bands of ONE filter of one neuron from the samplers' draws: the curve h(tau) = sum_b basis[tau, b] w_b of one
// group of B weights of a theta row (an impulse response of one presynaptic neuron, or the stimulus filter of one stimulus
// dimension), summarised over the pooled draws lag by lag, a simultaneous credible band over the whole curve, and the
// group's effective weight.  The counterpart of the reference's average_list_of_dicts / std_list_of_dicts over eval_state for
// the curves plot_imp_responses and the stimulus plot draw as mean +- 2 sd.  In the style of pglm_wald.h and pglm_diag.h: the
// rule in plain C, pgl_filt_group the whole rule of one group with serial loops -- the host mirror (tests/csrc/filters_host.c).
// k_filter_bands (pglm_filters.hip.h, one workgroup per (group, row)) calls the same scalar pieces and owns the parallel form.
//
// Inputs of row m, group g: the draws of the row, draw i of chain c at x[i si + c sc], pooled s = c n + i, S = C n (the order
// k_diag_column pools them); the offset o = first + g B of the group's B weights w_s = x_s[o .. o + B); a basis (R, B), row
// major; a contrast c (B); a level in (0, 1).
//
// The rule:
//  1. curve      h_s[tau] = sum_b basis[tau, b] w_s[b], b ascending from 0.0.
//  2. per lag    mean = sum_s h_s / S and sd = sqrt(sum_s (h_s - mean)^2 / (S - 1)), two passes.  Order of both sums (part of
//                the rule): pieces of PGL_FILT_PIECE = 256 consecutive draws, a piece summed ascending from 0.0, the pieces
//                added in order from 0.0.
//                q_lo, median, q_hi at p = (1 - level) / 2, 1 / 2, (1 + level) / 2 from the sorted values x_(0) <= ..
//                <= x_(S-1) by the linear rule of diagnostics.quantile (numpy.percentile's) with the position in doubles:
//                pos = p (S - 1), k = floor(pos), g = pos - k (exact), lo = x_(k) + 0.0, hi = x_(min(k + 1, S - 1)) + 0.0
//                (a zero order statistic is +0.0 whichever of -0.0 / +0.0 supplies it), and
//                Q = lo for g = 0,  lo + (hi - lo) g for g < 1/2,  hi - (hi - lo) (1 - g) otherwise -- here every product and
//                sum is rounded on its own, as the numpy statement of pglm_diag.h's rule does (the C form there fuses them).
//                These depend on the order statistics only: any sort gives the same bits, ties included.
//                A lag at which some h_s is not finite (finite weights can overflow): its five figures are NaN and it does
//                not enter step 3.
//  3. band       d_s = max over the lags with sd > 0 of r_s[tau] = |h_s[tau] - mean[tau]| / sd[tau], 0 if there is none (a
//                ratio that is NaN, inf / inf, is skipped).  c_sim = the k-th smallest d_s, k = ceil(level S) computed as
//                t = level S in double, k = trunc(t) + (trunc(t) < t), clamped to [1, S]: an exact order statistic.
//                Theorem (tested): at least k >= level S draws have r_s[tau] <= c_sim at EVERY lag with sd > 0 at once, with
//                r the rounded ratio above; and c_sim is >= the k-th smallest r_s[tau] of every such lag (the simultaneous
//                band is no narrower than the symmetric pointwise band in sd units), since d_s >= r_s[tau] draw by draw.
//                It need NOT contain the pointwise quantiles (q_hi - mean) / sd: those are one-sided.
//  4. weight     omega_s = sum_b c[b] w_s[b], b ascending from 0.0; its mean, sd, q_lo, median, q_hi as in 2 (NaN, p_pos too,
//                where some omega_s is not finite); p_pos = #{omega_s > 0} / S.
//  5. info       0; 1 where any weight of the group in any draw is not finite: then every output of the group is NaN (info
//                itself is 1) and no other group is affected.
// Every product and every sum is rounded on its own: the functions below are compiled with FP contraction off, as
// pglm_wald.h's.  Only + - x / sqrt and comparisons occur.  The order depends on (S, B, R, o) alone: a group gives the same
// bits alone or among others, run after run, and the device, this file under gcc and the numpy statement
// inference/filters.py: filter_bands_numpy agree bit for bit on the same input (NaNs compare as NaNs: their sign and payload
// are the machine's).
//
// Outputs: out (R, PGL_FILT_NLAG) = mean, sd, q_lo, median, q_hi per lag; grp (PGL_FILT_NGRP) = c_sim, the five figures of
// omega, p_pos, info (as a double).
//
// Layout of a theta row (glm.py: _Packing / theta_row): [bias, w_stim (D groups of B_stim, dimension-major: weight b of
// stimulus dimension d at 1 + d B_stim + b), w_ir (N groups of B_imp, presynaptic-neuron-major: weight b of neuron j at
// 1 + D B_stim + j B_imp + b)].  So the impulse groups are first = 1 + D B_stim, G = N, B = B_imp, and the stimulus filters
// first = 1, G = D, B = B_stim with the stimulus basis.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_FILTERS_H
#define PGLM_FILTERS_H

#include "pglm_wald.h"

#define PGL_FILT_MAX_B 16
#define PGL_FILT_MAX_DRAWS 4096     // the largest S a workgroup serves: its sort buffer is the next power of two of S doubles
#define PGL_FILT_PIECE 256
#define PGL_FILT_NLAG 5
#define PGL_FILT_NGRP 8
#define PGL_FILT_FN PGL_WALD_FN
#define PGL_FILT_NOCONTRACT PGL_WALD_NOCONTRACT
#define PGL_FILT_SQRT(x) PGL_WALD_SQRT(x)

// h_s[tau] (b: the basis row, stride 1) or omega_s (b: the contrast) of weights w with stride sw
PGL_FILT_FN double pgl_filt_dot(const double* b, const double* w, long long sw, int B)
{
    PGL_FILT_NOCONTRACT
    double s = 0.0;
    for (int a = 0; a < B; ++a) {
        const double t = b[a] * w[a * sw];
        s = s + t;
    }
    return s;
}

// one term of the second pass: acc + (x - mean)^2
PGL_FILT_FN double pgl_filt_sq_add(double acc, double x, double mean)
{
    PGL_FILT_NOCONTRACT
    const double t = x - mean;
    const double q = t * t;
    return acc + q;
}

// one piece of a sum over v[lo .. hi): plain (sq = 0) or of squared deviations from mean
PGL_FILT_FN double pgl_filt_piece(const double* v, long long lo, long long hi, int sq, double mean)
{
    PGL_FILT_NOCONTRACT
    double a = 0.0;
    if (sq) for (long long i = lo; i < hi; ++i) a = pgl_filt_sq_add(a, v[i], mean);
    else for (long long i = lo; i < hi; ++i) a = a + v[i];
    return a;
}

PGL_FILT_FN double pgl_filt_sd(double ss, long long S)
{
    PGL_FILT_NOCONTRACT
    const double q = ss / (double)(S - 1);
    return PGL_FILT_SQRT(q);
}

// r_s[tau]
PGL_FILT_FN double pgl_filt_ratio(double x, double mean, double sd)
{
    PGL_FILT_NOCONTRACT
    const double t = x - mean;
    return (t < 0.0 ? -t : t) / sd;
}

// the probabilities of step 2: q = 0, 1, 2 -> (1 - level) / 2, 1 / 2, (1 + level) / 2
PGL_FILT_FN double pgl_filt_prob(int q, double level)
{
    PGL_FILT_NOCONTRACT
    return q == 0 ? (1.0 - level) / 2.0 : (q == 1 ? 0.5 : (1.0 + level) / 2.0);
}

// the quantile p of the sorted values sv[0 .. S)
PGL_FILT_FN double pgl_filt_quantile(const double* sv, long long S, double p)
{
    PGL_FILT_NOCONTRACT
    const double pos = p * (double)(S - 1);
    long long k = (long long)pos;
    if (k > S - 1) k = S - 1;
    const double g = pos - (double)k;
    const double lo = sv[k] + 0.0, hi = sv[k + 1 < S ? k + 1 : S - 1] + 0.0;
    if (g == 0.0) return lo;
    const double d = hi - lo;
    if (g < 0.5) {
        const double t = d * g;
        return lo + t;
    }
    const double u = 1.0 - g;
    const double t = d * u;
    return hi - t;
}

// k of step 3, 1 .. S
PGL_FILT_FN long long pgl_filt_rank(double level, long long S)
{
    PGL_FILT_NOCONTRACT
    const double t = level * (double)S;
    long long k = (long long)t;
    if ((double)k < t) ++k;
    return k < 1 ? 1 : (k > S ? S : k);
}

// ---- the serial form ------------------------------------------------------------------------------------------------------
PGL_FILT_FN double pgl_filt_sum(const double* v, long long S, int sq, double mean)
{
    PGL_FILT_NOCONTRACT
    double s = 0.0;
    for (long long lo = 0; lo < S; lo += PGL_FILT_PIECE)
        s = s + pgl_filt_piece(v, lo, lo + PGL_FILT_PIECE < S ? lo + PGL_FILT_PIECE : S, sq, mean);
    return s;
}

// ascending, in place (any sort would do: the outputs depend on the order statistics only)
PGL_FILT_FN void pgl_filt_sort(double* v, long long S)
{
    for (long long gap = S / 2; gap > 0; gap /= 2)                 // Shell's sort
        for (long long i = gap; i < S; ++i) {
            const double x = v[i];
            long long j = i;
            for (; j >= gap && v[j - gap] > x; j -= gap) v[j] = v[j - gap];
            v[j] = x;
        }
}

// mean and sd of v[0 .. S)
PGL_FILT_FN void pgl_filt_moments(const double* v, long long S, double* mean, double* sd)
{
    PGL_FILT_NOCONTRACT
    *mean = pgl_filt_sum(v, S, 0, 0.0) / (double)S;
    *sd = pgl_filt_sd(pgl_filt_sum(v, S, 1, *mean), S);
}

// The whole rule of one group.  x: the first weight of the group in draw 0 of chain 0; draw i of chain c at x[i si + c sc].
// out (R, 5), grp (8).  work: (B + 2) S doubles.  Returns info.
PGL_FILT_FN int pgl_filt_group(const double* x, long long n, long long C, long long si, long long sc, int B, const double* basis,
                               long long R, const double* c, double level, double* out, double* grp, double* work)
{
    PGL_FILT_NOCONTRACT
    const long long S = n * C;
    double* w = work;                   // (S, B)
    double* v = work + S * B;           // the values of one lag
    double* d = v + S;
    const double nan = __builtin_nan("");
    int ok = 1;
    for (long long cc = 0; cc < C; ++cc)
        for (long long i = 0; i < n; ++i)
            for (int b = 0; b < B; ++b) {
                const double val = x[i * si + cc * sc + b];
                w[(cc * n + i) * B + b] = val;
                ok &= pgl_hmc_finite(val);
            }
    if (!ok) {
        for (long long q = 0; q < R * PGL_FILT_NLAG; ++q) out[q] = nan;
        for (int q = 0; q < PGL_FILT_NGRP - 1; ++q) grp[q] = nan;
        grp[PGL_FILT_NGRP - 1] = 1.0;
        return 1;
    }
    for (long long s = 0; s < S; ++s) d[s] = 0.0;
    for (long long tau = 0; tau <= R; ++tau) {                     // tau = R: the effective weight
        double* o5 = tau < R ? out + tau * PGL_FILT_NLAG : grp + 1;
        const double* brow = tau < R ? basis + tau * B : c;
        int fin = 1, pos = 0;
        for (long long s = 0; s < S; ++s) {
            v[s] = pgl_filt_dot(brow, w + s * B, 1, B);
            fin &= pgl_hmc_finite(v[s]);
            pos += v[s] > 0.0;
        }
        if (tau == R) grp[6] = fin ? (double)pos / (double)S : nan;
        if (!fin) {
            for (int q = 0; q < PGL_FILT_NLAG; ++q) o5[q] = nan;
            continue;
        }
        double mean, sd;
        pgl_filt_moments(v, S, &mean, &sd);
        if (tau < R && sd > 0.0)
            for (long long s = 0; s < S; ++s) {
                const double r = pgl_filt_ratio(v[s], mean, sd);
                d[s] = r > d[s] ? r : d[s];
            }
        pgl_filt_sort(v, S);
        o5[0] = mean;
        o5[1] = sd;
        for (int q = 0; q < 3; ++q) o5[2 + q] = pgl_filt_quantile(v, S, pgl_filt_prob(q, level));
    }
    pgl_filt_sort(d, S);
    grp[0] = d[pgl_filt_rank(level, S) - 1] + 0.0;
    grp[PGL_FILT_NGRP - 1] = 0.0;
    return 0;
}

#endif
