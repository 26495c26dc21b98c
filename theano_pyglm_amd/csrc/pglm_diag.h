// Convergence diagnostics of ONE column: the draws of one parameter of one neuron over C chains of n draws each, pooled size
// S = C n (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021, "Rank-normalization, folding, and localization: an improved
// R-hat for assessing convergence of MCMC", Bayesian Analysis 16; equation and section numbers below are the paper's).  In the
// style of pglm_psis.h: the scalar rules every implementation shares (the quantile positions, the normal score, the split
// chains, Geyer's sequence as a state machine that is fed pair after pair) and pgl_diag_column, the whole rule of one column
// with serial sums -- the host mirror (tests/csrc/diag_host.c).  k_diag_column (pglm_diag.hip.h, one workgroup per column)
// calls the same scalar rules and owns the parallel sums.
//
// The rule:
//  1. pooled       x_s, s = c n + i (chain c, draw i).  mean = sum x / S, sd = sqrt(sum (x - mean)^2 / (S - 1)).
//  2. ranks        on the raw doubles, before any arithmetic: lt_s = #{j : x_j < x_s}, eq_s = #{j : x_j == x_s} (itself
//                  included); ties get average ranks r_s = lt_s + (eq_s + 1) / 2, a multiple of 1/2 in [1, S].
//  3. quantiles    from ranks, not from a sort: the order statistic x_(k), k = 0 .. S - 1, is the x_s with lt_s <= k < lt_s +
//                  eq_s.  The quantile a / b (1/40, 1/20, 1/2, 19/20, 39/40) by the linear interpolation of numpy.percentile
//                  with the position in integers: k = a (S - 1) div b, g = (a (S - 1) mod b) / b,
//                  Q = x_(k) + (x_(k+1) - x_(k)) g  for g < 1/2,  x_(k+1) - (x_(k+1) - x_(k)) (1 - g)  otherwise (numpy's
//                  lerp), each product and sum one fused multiply-add, so that every compiler gives the same bits; g = 0
//                  gives x_(k) itself.  An order statistic is taken as x_s + 0.0: -0.0 and +0.0 compare equal and may tie,
//                  and a zero order statistic is +0.0 whichever of the tied draws supplies it (so is a constant column's value).
//  4. scores       z_s = Phi^-1((r_s - 3/8) / (S + 1/4))  (the paper's eq. 14 with Blom's offsets), Phi^-1 by Wichura's AS 241
//                  PPND16 (Applied Statistics 37, 1988; relative accuracy 1e-16), entered with the centred argument
//                  (r - (S + 1) / 2) / (S + 1/4) and, in the upper tail, with the upper tail probability (S - r + 5/8) / (S +
//                  1/4), so that z(r) = -z(S + 1 - r) to the bit.
//  5. folding      f_s = |x_s - median| in double, by exactly this subtraction; its ranks and scores as in 2 and 4: zf_s.
//  6. split        every chain is cut into halves of h = n div 2 draws: split chain j = 2 c + half holds the draws
//                  i = half (n - h) .. half (n - h) + h - 1 of chain c; the middle draw of an odd n belongs to no split chain
//                  (it is ranked and pooled all the same).  m = 2 C split chains, N = m h draws in them.
//  7. split-R-hat  of a series y (eqs. 1-4): mean_j and acov_j[0] = sum_i (y_i - mean_j)^2 / h of every split chain;
//                  W = (sum_j acov_j[0] / m) h / (h - 1);  B / h = sum_j (mean_j - mean)^2 / (m - 1), mean = sum_j mean_j / m;
//                  var+ = W (h - 1) / h + B / h  (eq. 3);  R-hat = sqrt(var+ / W)  (eq. 4).
//  8. ESS          of a series y (section 3.2; the rule of Stan and of the posterior package): the biased autocovariances
//                  acov_j[t] = sum_{i = 0}^{h - 1 - t} (y_i - mean_j)(y_{i+t} - mean_j) / h, i ascending, each product
//                  added by one fused multiply-add;  rho_t = 1 - (W - sum_j acov_j[t] / m) / var+  (eq. 10), rho_0 = 1 by
//                  definition.  Geyer's initial positive sequence on the pairs P_t = rho_t + rho_{t+1}, t even: starting
//                  at t = 0, while t < h - 5 and P_t > 0 go on to t + 2; T, the truncation lag, is the t at which this
//                  stops.  Initial monotone sequence: for t = 2, 4, .. T - 2 in turn, a pair with P_t > P_{t-2} has both
//                  its terms replaced by P_{t-2} / 2 (P_{t-2} as already corrected).  The final odd term: rho_T counts
//                  once where P_T >= 0 or rho_T > 0, else not at all.
//                  tau = -1 + 2 sum_{t < T} rho_t + rho_T  (T = 0: the sum is rho_0; h < 6 always ends there, with tau = 2),
//                  tau = max(tau, 1 / log10(N)), ESS = N / tau: the cap ESS <= N log10(N)  (N = S for an even n).
//  9. outputs      PGL_DIAG_NOUT rows (below): mean, sd, median, q025, q975; rhat_plain = the split-R-hat of x itself
//                  (mass_adapt.rhat); rhat = the larger of the split-R-hats of z and of zf (a NaN one is ignored);
//                  ess_bulk = ESS of z; ess_tail = the smaller of the ESS of I(x <= Q 1/20) and of I(x <= Q 19/20);
//                  ess_mean = ESS of x; mcse_mean = sd / sqrt(ess_mean); the truncation lags T of the four ESS, as doubles.
// 10. edges        a non-finite draw anywhere: every output of the column is NaN.
//                  max x == min x: mean, median and the quantiles are that constant, sd = 0, every ESS and lag is 0 (the
//                  convention of effective_sample_size), the R-hats and mcse_mean are NaN.
//                  a series that is constant over all split chains (var+ = 0; an indicator that is 1 everywhere, the folded
//                  scores of a symmetric two-valued column): its ESS and lag are 0, its R-hat NaN.
//                  a series constant within every split chain but not across them (W = 0, var+ = B / h > 0): R-hat = +inf;
//                  every acov is 0, so rho_t = 1 at every lag, the sequence runs to its end T (the first even t >= h - 5)
//                  and tau = 2 T for T > 0: ESS = N / (2 T), which is about m.
// Sums: the serial form below adds in ascending index.  The kernel's sums over the pooled draws are thread-strided partial
// sums combined by a binary tree, its chain means partial sums over an interleaved power-of-two group of threads combined by a
// tree, every acov_j[t] the serial sum of one thread, the sums over j serial.  Either order is fixed: two runs give the same
// bits, and a column gives the same bits wherever it stands in a call.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_DIAG_H
#define PGLM_DIAG_H

#include "pglm_hmc.h"

#define PGL_DIAG_FN PGL_HMC_FN
#define PGL_DIAG_NOUT 15
#define PGL_DIAG_MEAN 0
#define PGL_DIAG_SD 1
#define PGL_DIAG_MEDIAN 2
#define PGL_DIAG_Q025 3
#define PGL_DIAG_Q975 4
#define PGL_DIAG_RHAT_PLAIN 5
#define PGL_DIAG_RHAT 6
#define PGL_DIAG_ESS_BULK 7
#define PGL_DIAG_ESS_TAIL 8
#define PGL_DIAG_ESS_MEAN 9
#define PGL_DIAG_MCSE_MEAN 10
#define PGL_DIAG_LAG_BULK 11
#define PGL_DIAG_LAG_Q05 12
#define PGL_DIAG_LAG_Q95 13
#define PGL_DIAG_LAG_MEAN 14
#define PGL_DIAG_MIN_N 8                        // fewer draws per chain: PGL_ERR_ARG
// PGL_DIAG_MAX_DRAWS, the largest S a workgroup holds.  k_diag_column keeps per draw the raw x and the current series y (16
// bytes) in dynamic LDS, beside the m <= S / 4 split-chain means (<= 2 bytes per draw) and the autocovariances of one batch of
// lags, m x L doubles with m L <= max(256, 2 m) (<= 4 bytes per draw, at least 2048 bytes), and 3 168 bytes of static LDS (the
// reduction tree, a batch of rho, the order statistics, scalars).  At S = 4096 that is 65 536 + 8 192 + 16 384 + 3 168 =
// 93 280 bytes in the worst case (n = 8) and 70 816 bytes with four chains: above the 64 KiB a kernel gets without asking, so
// the launch opts in to the dynamic size it needs (as k_simulate does for its ring) whenever that exceeds 64 KiB; the 160 KiB
// of a compute unit hold it, and do not hold the next power of two (8192 draws: 131 072 bytes of x and y alone, 186 KiB in
// the worst case).  At 4 x 1000 draws a workgroup takes 69 280 bytes and a compute unit holds two of them.
#define PGL_DIAG_MAX_DRAWS 4096

// ---- quantile positions -------------------------------------------------------------------------------------------------
#define PGL_DIAG_NQ 5                           // 1/40, 1/20, 1/2, 19/20, 39/40
PGL_DIAG_FN long long pgl_diag_q_num(int q) { return q == 0 ? 1 : q == 1 ? 1 : q == 2 ? 1 : q == 3 ? 19 : 39; }
PGL_DIAG_FN long long pgl_diag_q_den(int q) { return q == 0 ? 40 : q == 1 ? 20 : q == 2 ? 2 : q == 3 ? 20 : 40; }
PGL_DIAG_FN long long pgl_diag_q_lo(int q, long long S) { return pgl_diag_q_num(q) * (S - 1) / pgl_diag_q_den(q); }
PGL_DIAG_FN long long pgl_diag_q_hi(int q, long long S)
{
    const long long k = pgl_diag_q_lo(q, S) + 1;
    return k < S ? k : S - 1;
}
PGL_DIAG_FN double pgl_diag_q_frac(int q, long long S)
{
    return (double)(pgl_diag_q_num(q) * (S - 1) % pgl_diag_q_den(q)) / (double)pgl_diag_q_den(q);
}
PGL_DIAG_FN double pgl_diag_lerp(double a, double b, double g)
{
    const double d = b - a;
    return g < 0.5 ? fma(d, g, a) : fma(-d, 1.0 - g, b);
}

// ---- the normal score (AS 241, PPND16) -------------------------------------------------------------------------------------
// The two branches of PPND16 in their probability-argument form, shared with the normal scores of pglm_acf.h: the centred
// probability q = p - 1/2 with |q| <= 0.425, and the probability pt of the nearer tail (the magnitude of the quantile).
PGL_DIAG_FN double pgl_ppnd16_central(double q)
{
    const double u = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e3 * u + 3.3430575583588128105e4) * u + 6.7265770927008700853e4) * u +
                            4.5921953931549871457e4) * u + 1.3731693765509461125e4) * u + 1.9715909503065514427e3) * u +
                         1.3314166789178437745e2) * u + 3.3871328727963666080e0);
    const double den = (((((((5.2264952788528545610e3 * u + 2.8729085735721942674e4) * u + 3.9307895800092710610e4) * u +
                            2.1213794301586595867e4) * u + 5.3941960214247511077e3) * u + 6.8718700749205790830e2) * u +
                         4.2313330701600911252e1) * u + 1.0);
    return q * num / den;
}
PGL_DIAG_FN double pgl_ppnd16_tail(double pt)
{
    double u = sqrt(-log(pt)), v;
    if (u <= 5.0) {
        u -= 1.6;
        const double num = (((((((7.74545014278341407640e-4 * u + 2.27238449892691845833e-2) * u + 2.41780725177450611770e-1) * u +
                                1.27045825245236838258e0) * u + 3.64784832476320460504e0) * u + 5.76949722146069140550e0) * u +
                             4.63033784615654529590e0) * u + 1.42343711074968357734e0);
        const double den = (((((((1.05075007164441684324e-9 * u + 5.47593808499534494600e-4) * u + 1.51986665636164571966e-2) * u +
                                1.48103976427480074590e-1) * u + 6.89767334985100004550e-1) * u + 1.67638483018380384940e0) * u +
                             2.05319162663775882187e0) * u + 1.0);
        v = num / den;
    } else {
        u -= 5.0;
        const double num = (((((((2.01033439929228813265e-7 * u + 2.71155556874348757815e-5) * u + 1.24266094738807843860e-3) * u +
                                2.65321895265761230930e-2) * u + 2.96560571828504891230e-1) * u + 1.78482653991729133580e0) * u +
                             5.46378491116411436990e0) * u + 6.65790464350110377720e0);
        const double den = (((((((2.04426310338993978564e-15 * u + 1.42151175831644588870e-7) * u + 1.84631831751005468180e-5) * u +
                                7.86869131145613259100e-4) * u + 1.48753612908506148525e-2) * u + 1.36929880922735805310e-1) * u +
                             5.99832206555887937690e-1) * u + 1.0);
        v = num / den;
    }
    return v;
}

// the normal score of an average rank r among S
PGL_DIAG_FN double pgl_diag_score(double r, double S)
{
    const double d = S + 0.25, q = (r - 0.5 * (S + 1.0)) / d;
    if (fabs(q) <= 0.425) return pgl_ppnd16_central(q);
    const double pt = q < 0.0 ? (r - 0.375) / d : (S - r + 0.625) / d;       // the probability of the nearer tail
    const double v = pgl_ppnd16_tail(pt);
    return q < 0.0 ? -v : v;
}

// the score from the counts of the rank walk
PGL_DIAG_FN double pgl_diag_score_counts(int lt, int eq, long long S)
{
    return pgl_diag_score((double)lt + 0.5 * (double)(eq + 1), (double)S);
}

// ---- split chains ---------------------------------------------------------------------------------------------------------
// the pooled index of draw 0 of split chain j (chains of n draws, halves of h)
PGL_DIAG_FN long long pgl_diag_split_base(long long j, long long n, long long h) { return (j >> 1) * n + (j & 1) * (n - h); }

PGL_DIAG_FN double pgl_diag_rhat(double W, double var_plus) { return sqrt(var_plus / W); }

PGL_DIAG_FN double pgl_diag_max_nan(double a, double b) { return (b > a || a != a) ? b : a; }   // a NaN is ignored

// ---- Geyer's sequence, fed pair after pair --------------------------------------------------------------------------------
typedef struct PglGeyer {
    int t, h;                // the current pair (rho_t, rho_{t+1}) and the length of a split chain
    double e, o;             // that pair
    double pa, pb;           // the pair before it, as corrected
    double acc;              // sum of the corrected terms before the current pair
} PglGeyer;

PGL_DIAG_FN void pgl_geyer_init(PglGeyer* g, int h, double rho1)
{
    g->t = 0;
    g->h = h;
    g->e = 1.0;
    g->o = rho1;
    g->pa = g->pb = 0.0;
    g->acc = 0.0;
}

// 1 while the pair (t + 2, t + 3) is wanted
PGL_DIAG_FN int pgl_geyer_wants(const PglGeyer* g) { return g->t < g->h - 5 && g->e + g->o > 0.0; }

// the current pair is not the last one: correct it against the pair before, add it, take the next
PGL_DIAG_FN void pgl_geyer_push(PglGeyer* g, double e, double o)
{
    if (g->t >= 2 && g->e + g->o > g->pa + g->pb) g->e = g->o = (g->pa + g->pb) / 2.0;
    g->acc += g->e;
    g->acc += g->o;
    g->pa = g->e;
    g->pb = g->o;
    g->t += 2;
    g->e = e;
    g->o = o;
}

// ESS = N / tau once no further pair is wanted; *lag = T
PGL_DIAG_FN double pgl_geyer_ess(const PglGeyer* g, double N, double* lag)
{
    const double last = (g->e + g->o >= 0.0 || g->e > 0.0) ? g->e : 0.0;
    const double acc = g->t == 0 ? last : g->acc;
    double tau = -1.0 + 2.0 * acc + last;
    const double floor_tau = 1.0 / log10(N);
    tau = tau > floor_tau ? tau : floor_tau;
    *lag = (double)g->t;
    return N / tau;
}

PGL_DIAG_FN double pgl_diag_rho(double W, double acov_mean, double var_plus) { return 1.0 - (W - acov_mean) / var_plus; }

// ---- the serial form ------------------------------------------------------------------------------------------------------
// mean over the m split chains of acov_j[t] of the centred series y (pooled layout)
PGL_DIAG_FN double pgl_diag_acov_mean(const double* y, long long n, long long h, long long m, long long t)
{
    double s = 0.0;
    for (long long j = 0; j < m; ++j) {
        const double* c = y + pgl_diag_split_base(j, n, h);
        double a = 0.0;
        for (long long i = 0; i + t < h; ++i) a = fma(c[i], c[i + t], a);
        s += a / (double)h;
    }
    return s / (double)m;
}

// Split-R-hat and ESS of the series y (pooled layout, S = C n values; centred in place per split chain).  cm: m doubles.
PGL_DIAG_FN void pgl_diag_series(double* y, long long n, long long C, double* cm, int want_ess, double* rhat, double* ess,
                                 double* lag)
{
    const long long h = n / 2, m = 2 * C;
    double mm = 0.0;
    for (long long j = 0; j < m; ++j) {
        double* c = y + pgl_diag_split_base(j, n, h);
        double s = 0.0;
        for (long long i = 0; i < h; ++i) s += c[i];
        cm[j] = s / (double)h;
        for (long long i = 0; i < h; ++i) c[i] -= cm[j];
        mm += cm[j];
    }
    mm /= (double)m;
    double bh = 0.0;
    for (long long j = 0; j < m; ++j) bh += (cm[j] - mm) * (cm[j] - mm);
    bh /= (double)(m - 1);
    const double a0 = pgl_diag_acov_mean(y, n, h, m, 0);
    const double W = a0 * (double)h / (double)(h - 1);
    const double vp = W * (double)(h - 1) / (double)h + bh;
    *rhat = pgl_diag_rhat(W, vp);
    if (!want_ess) return;
    if (!(vp > 0.0)) {
        *ess = 0.0;
        *lag = 0.0;
        return;
    }
    PglGeyer g;
    pgl_geyer_init(&g, (int)h, pgl_diag_rho(W, pgl_diag_acov_mean(y, n, h, m, 1), vp));
    while (pgl_geyer_wants(&g)) {
        const double e = pgl_diag_rho(W, pgl_diag_acov_mean(y, n, h, m, g.t + 2), vp);
        const double o = pgl_diag_rho(W, pgl_diag_acov_mean(y, n, h, m, g.t + 3), vp);
        pgl_geyer_push(&g, e, o);
    }
    *ess = pgl_geyer_ess(&g, (double)(m * h), lag);
}

// scores of the pooled values v[0 .. S) into z (ranks by counting)
PGL_DIAG_FN void pgl_diag_scores(const double* v, long long S, double* z)
{
    for (long long s = 0; s < S; ++s) {
        int lt = 0, eq = 0;
        for (long long j = 0; j < S; ++j) {
            lt += v[j] < v[s];
            eq += v[j] == v[s];
        }
        z[s] = pgl_diag_score_counts(lt, eq, S);
    }
}

// The whole rule of one column with serial sums.  Draw i of chain c at x[i * si + c * sc]; out has stride ldo between its
// PGL_DIAG_NOUT rows.  work: 3 S + 2 C doubles.
PGL_DIAG_FN void pgl_diag_column(const double* x, long long n, long long C, long long si, long long sc, double* out,
                                 long long ldo, double* work)
{
    const long long S = n * C;
    double* p = work;                // the pooled draws
    double* y = work + S;            // the current series
    double* f = work + 2 * S;        // the folded values
    double* cm = work + 3 * S;
    const double nan = __builtin_nan("");
    int ok = 1;
    for (long long c = 0; c < C; ++c)
        for (long long i = 0; i < n; ++i) {
            p[c * n + i] = x[i * si + c * sc];
            ok &= pgl_hmc_finite(p[c * n + i]);
        }
    if (!ok) {
        for (int r = 0; r < PGL_DIAG_NOUT; ++r) out[r * ldo] = nan;
        return;
    }
    double lo = p[0], hi = p[0];
    for (long long s = 1; s < S; ++s) {
        lo = p[s] < lo ? p[s] : lo;
        hi = p[s] > hi ? p[s] : hi;
    }
    if (lo == hi) {
        for (int r = 0; r < PGL_DIAG_NOUT; ++r) out[r * ldo] = 0.0;
        out[PGL_DIAG_MEAN * ldo] = out[PGL_DIAG_MEDIAN * ldo] = out[PGL_DIAG_Q025 * ldo] = out[PGL_DIAG_Q975 * ldo] = lo + 0.0;
        out[PGL_DIAG_RHAT_PLAIN * ldo] = out[PGL_DIAG_RHAT * ldo] = out[PGL_DIAG_MCSE_MEAN * ldo] = nan;
        return;
    }
    double mean = 0.0, ss = 0.0;
    for (long long s = 0; s < S; ++s) mean += p[s];
    mean /= (double)S;
    for (long long s = 0; s < S; ++s) ss += (p[s] - mean) * (p[s] - mean);
    const double sd = sqrt(ss / (double)(S - 1));
    // ranks, scores and the order statistics the quantiles need
    double os_lo[PGL_DIAG_NQ], os_hi[PGL_DIAG_NQ], Q[PGL_DIAG_NQ];
    for (long long s = 0; s < S; ++s) {
        int lt = 0, eq = 0;
        for (long long j = 0; j < S; ++j) {
            lt += p[j] < p[s];
            eq += p[j] == p[s];
        }
        y[s] = pgl_diag_score_counts(lt, eq, S);
        for (int q = 0; q < PGL_DIAG_NQ; ++q) {
            const long long k0 = pgl_diag_q_lo(q, S), k1 = pgl_diag_q_hi(q, S);
            if (lt <= k0 && k0 < lt + eq) os_lo[q] = p[s] + 0.0;
            if (lt <= k1 && k1 < lt + eq) os_hi[q] = p[s] + 0.0;
        }
    }
    for (int q = 0; q < PGL_DIAG_NQ; ++q) Q[q] = pgl_diag_lerp(os_lo[q], os_hi[q], pgl_diag_q_frac(q, S));
    double rhat_bulk, rhat_fold, rhat_plain, ess_bulk, ess_lo, ess_hi, ess_mean, lag_bulk, lag_lo, lag_hi, lag_mean, dummy;
    pgl_diag_series(y, n, C, cm, 1, &rhat_bulk, &ess_bulk, &lag_bulk);
    for (long long s = 0; s < S; ++s) f[s] = fabs(p[s] - Q[2]);
    pgl_diag_scores(f, S, y);
    pgl_diag_series(y, n, C, cm, 0, &rhat_fold, &dummy, &dummy);
    for (long long s = 0; s < S; ++s) y[s] = p[s] <= Q[1] ? 1.0 : 0.0;
    pgl_diag_series(y, n, C, cm, 1, &dummy, &ess_lo, &lag_lo);
    for (long long s = 0; s < S; ++s) y[s] = p[s] <= Q[3] ? 1.0 : 0.0;
    pgl_diag_series(y, n, C, cm, 1, &dummy, &ess_hi, &lag_hi);
    for (long long s = 0; s < S; ++s) y[s] = p[s];
    pgl_diag_series(y, n, C, cm, 1, &rhat_plain, &ess_mean, &lag_mean);
    out[PGL_DIAG_MEAN * ldo] = mean;
    out[PGL_DIAG_SD * ldo] = sd;
    out[PGL_DIAG_MEDIAN * ldo] = Q[2];
    out[PGL_DIAG_Q025 * ldo] = Q[0];
    out[PGL_DIAG_Q975 * ldo] = Q[4];
    out[PGL_DIAG_RHAT_PLAIN * ldo] = rhat_plain;
    out[PGL_DIAG_RHAT * ldo] = pgl_diag_max_nan(rhat_bulk, rhat_fold);
    out[PGL_DIAG_ESS_BULK * ldo] = ess_bulk;
    out[PGL_DIAG_ESS_TAIL * ldo] = ess_lo < ess_hi ? ess_lo : ess_hi;
    out[PGL_DIAG_ESS_MEAN * ldo] = ess_mean;
    out[PGL_DIAG_MCSE_MEAN * ldo] = sd / sqrt(ess_mean);
    out[PGL_DIAG_LAG_BULK * ldo] = lag_bulk;
    out[PGL_DIAG_LAG_Q05 * ldo] = lag_lo;
    out[PGL_DIAG_LAG_Q95 * ldo] = lag_hi;
    out[PGL_DIAG_LAG_MEAN * ldo] = lag_mean;
}

#endif
