// Independence of the rescaled intervals (the second half of the time-rescaling check of Brown et al. 2002 and Haslinger, Pipa
// & Brown 2010): the serial correlation of the normal scores g_k = Phi^-1(z_k), z_k = 1 - exp(-tau_k), at the lags 1 .. L and a
// portmanteau statistic over the lags.  The rules every implementation shares: k_acf_segment of pglm_acf.hip.h, the host mirror
// tests/csrc/acf_host.c, gof.acf_scores in numpy.
//
// Segments and runs.  A segment is one neuron; it is made of runs, one per data sequence.  The intervals of one run are
// consecutive in time, intervals of different runs are not neighbours.  run_off (R + 1, non-decreasing from 0): run r is
// tau[run_off[r] .. run_off[r+1]);  seg_run (M + 1, non-decreasing from 0): segment m holds the runs seg_run[m] .. seg_run[m+1],
// n = run_off[seg_run[m+1]] - run_off[seg_run[m]] intervals.  Empty runs and empty segments are legal.
//
// Score.  z = -expm1(-tau), q = z - 1/2.
//     |q| <= 0.425:  g = PPND16's central branch on q (pgl_ppnd16_central of pglm_diag.h, Wichura's AS 241).  The q that enters
//                    it is the same number z - 1/2 = -expm1(log 2 - tau) / 2 computed without the cancellation at tau = log 2:
//                    t = (LN2_HI - tau) + LN2_LO, q = -0.5 expm1(t) -- z carries an absolute error of 2^-54, which is any
//                    relative error of z - 1/2 near the median.  The branch is chosen on the plain z - 0.5.
//     otherwise:     the tail probability r = z for q < 0 and r = exp(-tau) for q > 0 (the upper tail directly, not 1 - z),
//                    r = max(r, DBL_MIN), g = -+ pgl_ppnd16_tail(r).  tau = 0, a subnormal tau and tau = +inf give finite scores
//                    of magnitude about 37.5.  A NaN tau gives a NaN score.
//
// Statistics of a segment g_0 .. g_{n-1}:
//     m = (sum g_i) / n,  d_i = g_i - m,  c_0 = sum d_i^2,
//     c_k = sum d_i d_{i+k} over the pairs whose two members lie in the same run, n_k the number of such pairs,
//     r_k = c_k / c_0 (k = 1 .. L),  v_k = n_k / (n (n + 2)),  Q = sum_{k: n_k >= 1} r_k^2 / v_k in ascending k,
//     dof = #{k: n_k >= 1}.  With one run n_k = n - k and Q is Ljung-Box.  A lag with n_k = 0: r_k = NaN, left out of Q.
//
// Order of the sums (part of the rule).  Every sum runs over the segment's index i.  The index is cut into pieces of
// PGL_ACF_PIECE = 256 consecutive i counted from the segment's FIRST element (not from a run's); inside a piece the terms are
// added in ascending i from 0.0, invalid pairs skipped (the pair (i, i + k) belongs to the piece of i); the piece totals are
// added in ascending piece order from 0.0.  Every product and every sum is rounded on its own: the functions that hold them are
// compiled with FP contraction off (PGL_ACF_NOCONTRACT below: `#pragma clang fp contract(off)` under clang, hipcc's device
// pass included; the optimize("fp-contract=off") attribute under gcc) -- the other host-mirrored headers spell fma() out where
// they want one and have no sum that must stay unfused; this one has.  The bits therefore do not depend on the grid, on M, on
// the other segments or on how the lags are grouped.
//
// Voids.  Any tau of the segment NaN or negative: every output but n is NaN (the reserved one too).  n < 3 or c_0 == 0: every
// r_k and Q are NaN and dof = 0 (mean and c_0 are reported; n = 0: mean = 0 / 0 = NaN, c_0 = 0).
//
// Output: PGL_ACF_NHEAD + L doubles per segment: n, mean, c_0, Q, dof, 0 (reserved), r_1 .. r_L.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_ACF_H
#define PGLM_ACF_H

#include "pglm_diag.h"
#include "pglm_gof.h"

#define PGL_ACF_MAX_LAG 64
#define PGL_ACF_NHEAD 6
#define PGL_ACF_PIECE 256
#define PGL_ACF_DBL_MIN 2.2250738585072014e-308
#define PGL_ACF_LN2_HI 0.6931471805599453094          // the double nearest log 2
#define PGL_ACF_LN2_LO 2.319046813846299558e-17       // log 2 minus that double

#if defined(__clang__)
#define PGL_ACF_FN PGL_HMC_FN
#define PGL_ACF_NOCONTRACT _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define PGL_ACF_FN __attribute__((optimize("fp-contract=off"))) PGL_HMC_FN
#define PGL_ACF_NOCONTRACT
#else
#define PGL_ACF_FN PGL_HMC_FN
#define PGL_ACF_NOCONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

PGL_HMC_FN double pgl_acf_score(double tau)
{
    const double z = pgl_gof_z(tau), q = z - 0.5;
    if (fabs(q) <= 0.425) return pgl_ppnd16_central(-0.5 * expm1((PGL_ACF_LN2_HI - tau) + PGL_ACF_LN2_LO));
    double r = q < 0.0 ? z : exp(-tau);
    r = r < PGL_ACF_DBL_MIN ? PGL_ACF_DBL_MIN : r;
    const double v = pgl_ppnd16_tail(r);
    return q < 0.0 ? -v : v;
}

PGL_HMC_FN long long pgl_acf_pieces(long long n) { return (n + PGL_ACF_PIECE - 1) / PGL_ACF_PIECE; }

// one term and one step of a sum, each rounded on its own
PGL_ACF_FN double pgl_acf_mul(double a, double b)
{
    PGL_ACF_NOCONTRACT
    return a * b;
}
PGL_ACF_FN double pgl_acf_add(double s, double t)
{
    PGL_ACF_NOCONTRACT
    return s + t;
}
PGL_ACF_FN double pgl_acf_madd(double s, double a, double b)     // s + a b in two roundings
{
    PGL_ACF_NOCONTRACT
    const double t = a * b;
    return s + t;
}

PGL_ACF_FN double pgl_acf_mean(double sum, long long n)
{
    PGL_ACF_NOCONTRACT
    return sum / (double)n;
}
PGL_ACF_FN double pgl_acf_centre(double g, double mean)
{
    PGL_ACF_NOCONTRACT
    return g - mean;
}

// The outputs of a segment from its sums: c[0 .. L] (c[0] = c_0), cnt[1 .. L] = n_k (cnt[0] unused), bad: a void tau.
PGL_ACF_FN void pgl_acf_finish(long long n, double mean, const double* c, const long long* cnt, int L, int bad, double* out)
{
    PGL_ACF_NOCONTRACT
    const double nan = __builtin_nan("");
    out[0] = (double)n;
    if (bad) {
        for (int j = 1; j < PGL_ACF_NHEAD + L; ++j) out[j] = nan;
        return;
    }
    out[5] = 0.0;
    out[1] = mean;
    out[2] = c[0];
    if (n < 3 || c[0] == 0.0) {
        out[3] = nan;
        out[4] = 0.0;
        for (int k = 1; k <= L; ++k) out[PGL_ACF_NHEAD + k - 1] = nan;
        return;
    }
    const double nn = (double)n * ((double)n + 2.0);
    double Q = 0.0;
    int dof = 0;
    for (int k = 1; k <= L; ++k) {
        if (cnt[k] < 1) {
            out[PGL_ACF_NHEAD + k - 1] = nan;
            continue;
        }
        const double r = c[k] / c[0];
        const double v = (double)cnt[k] / nn;
        const double r2 = r * r;
        const double t = r2 / v;
        Q = Q + t;
        ++dof;
        out[PGL_ACF_NHEAD + k - 1] = r;
    }
    out[3] = Q;
    out[4] = (double)dof;
}

// ---- the serial form (the host mirror) --------------------------------------------------------------------------------------
// The statistics of one segment from its scores g[0 .. n): run_off points at the segment's first run boundary (run_off[0] is the
// absolute index of g[0]), nruns runs.  work: n doubles (the centred scores) and n long longs (the end of every element's run).
PGL_ACF_FN int pgl_acf_bad_any(const double* tau, long long n)
{
    int bad = 0;
    for (long long i = 0; i < n; ++i) bad |= pgl_gof_bad(tau[i]);
    return bad;
}

PGL_ACF_FN void pgl_acf_stats(const double* g, const long long* run_off, long long nruns, int L, int bad, double* d, long long* end,
                              double* out)
{
    PGL_ACF_NOCONTRACT
    const long long o0 = run_off[0], n = run_off[nruns] - o0, np = pgl_acf_pieces(n);
    double c[PGL_ACF_MAX_LAG + 1];
    long long cnt[PGL_ACF_MAX_LAG + 1];
    for (long long r = 0; r < nruns; ++r)
        for (long long i = run_off[r] - o0; i < run_off[r + 1] - o0; ++i) end[i] = run_off[r + 1] - o0;
    double sum = 0.0;
    for (long long p = 0; p < np; ++p) {
        const long long a = p * PGL_ACF_PIECE, b = a + PGL_ACF_PIECE < n ? a + PGL_ACF_PIECE : n;
        double s = 0.0;
        for (long long i = a; i < b; ++i) s = s + g[i];
        sum = sum + s;
    }
    const double mean = pgl_acf_mean(sum, n);
    for (long long i = 0; i < n; ++i) d[i] = pgl_acf_centre(g[i], mean);
    for (int k = 0; k <= L; ++k) {
        double ck = 0.0;
        long long nk = 0;
        for (long long p = 0; p < np; ++p) {
            const long long a = p * PGL_ACF_PIECE, b = a + PGL_ACF_PIECE < n ? a + PGL_ACF_PIECE : n;
            double s = 0.0;
            for (long long i = a; i < b; ++i)
                if (i + k < end[i]) {
                    s = pgl_acf_madd(s, d[i], d[i + k]);
                    ++nk;
                }
            ck = ck + s;
        }
        c[k] = ck;
        cnt[k] = nk;
    }
    pgl_acf_finish(n, mean, c, cnt, L, bad, out);
}

#endif
