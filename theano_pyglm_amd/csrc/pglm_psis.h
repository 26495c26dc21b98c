// Pareto-smoothed importance sampling leave-one-out (PSIS-LOO) of ONE column: the log-likelihood l_0 .. l_{S-1} of one time
// block of one neuron under the S posterior draws (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024;
// the generalized-Pareto fit of Zhang & Stephens 2009 as the loo package and ArviZ state it).  In the style of pglm_pointwise.h
// and pglm_adapt.h: the scalar rules (tail length, candidate shapes, profile likelihood, quantile replacement) that every
// implementation shares, and pgl_psis_column, the whole rule of one column with serial sums -- the host mirror
// (tests/csrc/psis_host.c).  k_psis_column (pglm_psis.hip.h, one workgroup per column) calls the same scalar rules and owns
// the parallel sums.
//
// The rule:
//  1. ratios       r_s = -l_s,  x_s = r_s - max_s r_s  (<= 0).
//  2. order        all ordering and every tie decision is made on the raw input doubles l_s, before any arithmetic:
//                  descending l (= ascending r), ties by the draw index, smaller s first.  pos(s) = #{j : l_j > l_s or
//                  (l_j == l_s and j < s)} is the 0-based rank.  Tail membership and the order inside the tail are exact
//                  facts of the input, the same in every implementation and precision.
//  3. tail         M = ceil(min(S / 5, 3 sqrt(S)))  (pgl_psis_tail_len: integer arithmetic, exact).  The cutoff element is
//                  the one of rank S - M - 1; x_cut = max(x of that element, log(DBL_MIN)).  The tail is the set of elements
//                  whose raw l is strictly smaller than the cutoff element's raw l (raw r strictly larger): the last n ranks,
//                  n <= M, n < M with ties at the cutoff.
//  4. short tails  n < PGL_PSIS_MIN_TAIL (5): khat = +inf, nothing is smoothed.
//  5. fit          excesses e_i = exp(x_tail,i) - exp(x_cut), i = 1 .. n ascending (the tail in rank order).
//                  m = 30 + floor(sqrt(n));  b_i = 1 / e_n + (1 - sqrt(m / (i - 0.5))) / (3 e_q),  q = floor(n / 4 + 0.5)
//                  (1-based), i = 1 .. m;  k_i = (1/n) sum_j log1p(-b_i e_j);  L_i = n (log(-b_i / k_i) - k_i - 1);
//                  w_i = 1 / sum_j exp(L_j - L_i)  (j = 1 .. m ascending);  weights below 10 DBL_EPSILON are dropped, W = sum
//                  of the kept w_i (i ascending);  b = sum_i (w_i / W) b_i over the kept i ascending;
//                  k = (1/n) sum_j log1p(-b e_j);  sigma = -k / b;  khat = (n k + 10 / 2) / (n + 10).
//  6. smooth       when khat is finite the tail element of rank i (1-based, of n) gets
//                  x = log(exp(x_cut) + sigma expm1(-khat log1p(-p_i)) / khat),  p_i = (i - 0.5) / n;  for
//                  |khat| < PGL_PSIS_K_TINY (DBL_EPSILON, ArviZ's threshold) the limit  -sigma log1p(-p_i)  replaces the ratio.
//  7. truncate     every x is truncated at 0: x = min(x, 0); a NaN stays (where every candidate weight is dropped b = 0 and
//                  sigma = 0 / 0: khat = 0.1 is finite, the smoothed x are NaN and so are elpd, n_eff and the weights).
//                  lw_s = x_s - (mx + log sum_s exp(x_s - mx)),  mx = max_s x_s.
//  8. outputs      elpd  = a + log sum_s exp(lw_s + l_s - a),  a = max_s (lw_s + l_s);
//                  khat;   n_eff = 1 / sum_s exp(2 lw_s);   n, the tail length used (as a double).
//  9. non-finite   a column holding a NaN or an infinite l yields four NaNs (and NaN weights where weights are written).
// Sums: the serial form below adds in ascending index.  The kernel adds the sums over s and over the tail as
// thread-strided partial sums (thread t takes t, t + 256, ... in ascending order) combined by a binary tree over the 256
// partials (pglm_psis.hip.h); the sums over the m candidates are serial there too.  Either order is fixed: two runs give
// the same bits, and a column gives the same bits wherever it stands in a call.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_PSIS_H
#define PGLM_PSIS_H

#include "pglm_hmc.h"

#define PGL_PSIS_FN PGL_HMC_FN
#define PGL_PSIS_NOUT 4                         // planes of the result (4, C): elpd, khat, n_eff, tail length
#define PGL_PSIS_MIN_TAIL 5                     // fewer tail elements: khat = +inf
#define PGL_PSIS_K_TINY 2.220446049250313e-16   // |khat| below this (DBL_EPSILON): the khat -> 0 limit of the quantile
#define PGL_PSIS_W_DROP 2.220446049250313e-15   // 10 DBL_EPSILON: candidate weights below this are dropped
#define PGL_PSIS_LOG_DBL_MIN -708.3964185322641 // log(DBL_MIN), the floor of the cutoff
#define PGL_PSIS_MAX_CAND 64                    // room for the candidates: m = 30 + floor(sqrt(n)) <= 64 up to n = 1155
// PGL_PSIS_MAX_DRAWS, the largest S a workgroup holds.  k_psis_column keeps per draw the raw l (8 bytes) and its rank (4
// bytes) in LDS, beside PGL_PSIS_MAX_TAIL excesses and as many smoothed values (2 x 8 x 192 = 3072 bytes), the 256 doubles
// of the reduction tree (2048 bytes) and 3 x PGL_PSIS_MAX_CAND doubles of the fit (1536 bytes).  A workgroup may use 64 KiB of
// LDS without the opt-in for more: 12 x 4096 + 3072 + 2048 + 1536 + 16 (two scalars) = 55 824 bytes
// <= 65 536, and the next power of two does not fit.  (At S = 1000 a workgroup takes 14.6 KiB and the 160 KiB of a compute unit hold its 8 workgroups of 4 waves.)
#define PGL_PSIS_MAX_DRAWS 4096
#define PGL_PSIS_MAX_TAIL 192                   // pgl_psis_tail_len(PGL_PSIS_MAX_DRAWS) = 3 sqrt(4096)

// M = ceil(min(S / 5, 3 sqrt(S))) in integers: S / 5 <= 3 sqrt(S) iff S <= 225; else the smallest m with m^2 >= 9 S
PGL_PSIS_FN long long pgl_psis_tail_len(long long S)
{
    if (S <= 225) return (S + 4) / 5;
    long long m = (long long)sqrt((double)(9 * S));
    while (m * m < 9 * S) ++m;
    while ((m - 1) * (m - 1) >= 9 * S) --m;
    return m;
}

PGL_PSIS_FN int pgl_psis_candidates(long long n) { return 30 + (int)sqrt((double)n); }    // (n <= 1155: exact, <= 64)

// candidate shape b_i, i = 1 .. m, from the largest excess e_n and the quartile excess e_q
PGL_PSIS_FN double pgl_psis_cand(int i, int m, double e_n, double e_q)
{
    return 1.0 / e_n + (1.0 - sqrt((double)m / ((double)i - 0.5))) / (3.0 * e_q);
}

PGL_PSIS_FN long long pgl_psis_quartile(long long n) { return (long long)((double)n / 4.0 + 0.5); }   // 1-based

PGL_PSIS_FN double pgl_psis_profile(double b, double k, long long n) { return (double)n * (log(-(b / k)) - k - 1.0); }

// w_i of candidate i (0-based) from the profile log-likelihoods L[0 .. m)
PGL_PSIS_FN double pgl_psis_weight(const double* L, int m, int i)
{
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += exp(L[j] - L[i]);
    return 1.0 / s;
}

// b = sum of (w_i / W) b_i over the kept candidates
PGL_PSIS_FN double pgl_psis_posterior_b(const double* w, const double* b, int m)
{
    double W = 0.0, r = 0.0;
    for (int i = 0; i < m; ++i) if (w[i] >= PGL_PSIS_W_DROP) W += w[i];
    for (int i = 0; i < m; ++i) if (w[i] >= PGL_PSIS_W_DROP) r += (w[i] / W) * b[i];
    return r;
}

PGL_PSIS_FN double pgl_psis_khat(double k, long long n) { return ((double)n * k + 5.0) / ((double)n + 10.0); }

// the smoothed x of the tail element of rank i (0-based here) of n
PGL_PSIS_FN double pgl_psis_smoothed(long long i, long long n, double khat, double sigma, double exp_cut)
{
    const double a = log1p(-((double)i + 0.5) / (double)n);
    const double q = (fabs(khat) < PGL_PSIS_K_TINY) ? -a : expm1(-khat * a) / khat;
    return log(exp_cut + sigma * q);
}

// truncation at 0; a NaN (a fit that failed: sigma = 0 / 0 when every candidate weight was dropped) stays a NaN
PGL_PSIS_FN double pgl_psis_truncate(double x) { return x > 0.0 ? 0.0 : x; }

PGL_PSIS_FN double pgl_psis_cutoff(double l_cut, double rmax)
{
    const double x = -l_cut - rmax;
    return x > PGL_PSIS_LOG_DBL_MIN ? x : PGL_PSIS_LOG_DBL_MIN;
}

// The whole rule of one column with serial sums: l (stride ld) -> out (stride ldo: elpd, khat, n_eff, tail length) and,
// where lw is given, the log weights (stride ld).  pos: S ints of work space, tail: 2 * pgl_psis_tail_len(S) doubles.
PGL_PSIS_FN void pgl_psis_column(const double* l, long long S, long long ld, double* out, long long ldo, double* lw, int* pos,
                                 double* tail)
{
    const double nan = __builtin_nan("");
    int ok = 1;
    for (long long s = 0; s < S; ++s) ok &= pgl_hmc_finite(l[s * ld]);
    if (!ok) {
        for (int q = 0; q < PGL_PSIS_NOUT; ++q) out[q * ldo] = nan;
        if (lw) for (long long s = 0; s < S; ++s) lw[s * ld] = nan;
        return;
    }
    double lmin = l[0];
    for (long long s = 1; s < S; ++s) lmin = l[s * ld] < lmin ? l[s * ld] : lmin;
    const double rmax = -lmin;
    for (long long s = 0; s < S; ++s) {
        const double a = l[s * ld];
        int p = 0;
        for (long long j = 0; j < S; ++j) {
            const double c = l[j * ld];
            p += (c > a) || (c == a && j < s);
        }
        pos[s] = p;
    }
    const long long M = pgl_psis_tail_len(S);
    double l_cut = 0.0;
    for (long long s = 0; s < S; ++s) if (pos[s] == S - M - 1) l_cut = l[s * ld];
    long long n = 0;
    for (long long s = 0; s < S; ++s) n += l[s * ld] < l_cut;
    const double x_cut = pgl_psis_cutoff(l_cut, rmax), exp_cut = exp(x_cut);
    double* e = tail;
    double* sm = tail + M;
    double khat = (double)INFINITY;
    if (n >= PGL_PSIS_MIN_TAIL) {
        for (long long s = 0; s < S; ++s) if (pos[s] >= S - n) e[pos[s] - (S - n)] = exp(-l[s * ld] - rmax) - exp_cut;
        const int m = pgl_psis_candidates(n);
        double b[PGL_PSIS_MAX_CAND], L[PGL_PSIS_MAX_CAND], w[PGL_PSIS_MAX_CAND];
        for (int i = 0; i < m; ++i) {
            b[i] = pgl_psis_cand(i + 1, m, e[n - 1], e[pgl_psis_quartile(n) - 1]);
            double k = 0.0;
            for (long long j = 0; j < n; ++j) k += log1p(-b[i] * e[j]);
            L[i] = pgl_psis_profile(b[i], k / (double)n, n);
        }
        for (int i = 0; i < m; ++i) w[i] = pgl_psis_weight(L, m, i);
        const double bp = pgl_psis_posterior_b(w, b, m);
        double k = 0.0;
        for (long long j = 0; j < n; ++j) k += log1p(-bp * e[j]);
        k /= (double)n;
        const double sigma = -k / bp;
        khat = pgl_psis_khat(k, n);
        if (pgl_hmc_finite(khat)) for (long long i = 0; i < n; ++i) sm[i] = pgl_psis_smoothed(i, n, khat, sigma, exp_cut);
    }
    const int smooth = n >= PGL_PSIS_MIN_TAIL && pgl_hmc_finite(khat);
#define PGL_PSIS_X(s) ((smooth && pos[s] >= S - n) ? sm[pos[s] - (S - n)] : -l[(s) * ld] - rmax)
    double mx = -(double)INFINITY;
    for (long long s = 0; s < S; ++s) { double x = PGL_PSIS_X(s); x = pgl_psis_truncate(x); mx = x > mx ? x : mx; }
    double z = 0.0;
    for (long long s = 0; s < S; ++s) { double x = PGL_PSIS_X(s); x = pgl_psis_truncate(x); z += exp(x - mx); }
    const double lse = mx + log(z);
    double a = -(double)INFINITY;
    for (long long s = 0; s < S; ++s) { double x = PGL_PSIS_X(s); x = pgl_psis_truncate(x); const double v = x - lse + l[s * ld]; a = v > a ? v : a; }
    double se = 0.0, s2 = 0.0;
    for (long long s = 0; s < S; ++s) {
        double x = PGL_PSIS_X(s);
        x = pgl_psis_truncate(x);
        const double w_s = x - lse;
        se += exp(w_s + l[s * ld] - a);
        s2 += exp(2.0 * w_s);
        if (lw) lw[s * ld] = w_s;
    }
#undef PGL_PSIS_X
    out[0] = a + log(se);
    out[ldo] = khat;
    out[2 * ldo] = 1.0 / s2;
    out[3 * ldo] = (double)n;
}

#endif
