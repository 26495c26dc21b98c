// Convergence diagnostics on the device: k_diag_column, one workgroup of 256 threads per column of the samplers' tensor
// (n, C, K) as it lies (draw i of chain c of column k at (i * C + c) * ld + k), the pooled column resident in LDS.  The rule of
// a column and the scalar pieces are pglm_diag.h's; this file owns the parallel form:
//   load      thread t reads the pooled draws t, t + 256, ... (adjacent columns belong to adjacent workgroups, which run
//             together and share the lines in L2) into p[S], chain after chain; a non-finite value anywhere ends the column
//             with NaNs, max == min with the constants of the rule;
//   ranks     by counting, on the raw doubles, with the broadcast walk of k_psis_column: a thread holds four of its draws in
//             registers and walks p[0 .. S) once for them (every lane reads the same address: an LDS broadcast), counting the
//             smaller and the equal values; the score goes to y[s], and a draw whose rank interval holds one of the ten order
//             statistics the quantiles need publishes its value.  The folded ranks walk |p - median|, formed on the fly;
//   series    the five series (z, folded z, the two indicators, x) take turns in y[S].  Split-chain means: an interleaved
//             power-of-two group of threads per split chain, a tree inside the group.  The series is centred in place;
//   acov      a thread owns a (split chain, lag) pair of the current batch of L lags (L = 256 / m, even, 2 .. 128) and sums
//             over the draws ascending with one fused multiply-add per term; lane-adjacent threads hold adjacent lags of one
//             chain, so one operand is an LDS broadcast and the other a run of consecutive doubles.  The mean over the
//             chains is serial (one thread per lag).  Every thread then feeds the batch's pairs to the same Geyer state
//             (pglm_diag.h) from LDS -- uniform, no divergence -- and the next batch runs only while the sequence wants
//             more.  A value of rho depends on its lag alone, never on the batch it was computed in;
//   sums      over the pooled draws: thread t adds t, t + 256, ... ascending, the 256 partial values combine by the binary
//             tree of psis_reduce.
// All f64, no atomics, nothing depends on the launch shape or on the neighbours: a column gives the same bits alone and among
// others, run after run.
#pragma once

#include "pglm_diag.h"
#include "pglm_psis.hip.h"

#define PGL_DIAG_THREADS 256
#define PGL_DIAG_OWN 4          // draws a thread ranks per walk over the column
#define PGL_DIAG_MAX_LAGS 128   // the largest batch of lags (one chain: m = 2)

// lags per batch for m split chains: m L <= 256 while m <= 128, else L = 2
static inline __host__ __device__ int diag_batch_lags(long long m)
{
    const long long L = (PGL_DIAG_THREADS / m) & ~1LL;
    return (int)(L < 2 ? 2 : (L > PGL_DIAG_MAX_LAGS ? PGL_DIAG_MAX_LAGS : L));
}

// bytes of dynamic LDS: p[S], y[S], the m means, the m x L autocovariances of a batch
static inline size_t diag_lds_bytes(long long n, long long C)
{
    const long long m = 2 * C;
    return (size_t)(2 * n * C + m + m * diag_batch_lags(m)) * 8;
}
#define PGL_DIAG_STATIC_LDS 3168   // red, am, osq and two scalars below

template <bool FOLD>
__device__ __forceinline__ void diag_walk(const double* p, double* y, int S, double med, double* osq)
{
    const int t = threadIdx.x;
    int k0[PGL_DIAG_NQ], k1[PGL_DIAG_NQ];
#pragma unroll
    for (int q = 0; q < PGL_DIAG_NQ; ++q) {
        k0[q] = (int)pgl_diag_q_lo(q, S);
        k1[q] = (int)pgl_diag_q_hi(q, S);
    }
    for (int s0 = t; s0 < S; s0 += PGL_DIAG_OWN * PGL_DIAG_THREADS) {
        double a[PGL_DIAG_OWN];
        int lt[PGL_DIAG_OWN], eq[PGL_DIAG_OWN];
#pragma unroll
        for (int u = 0; u < PGL_DIAG_OWN; ++u) {
            const int s = s0 + u * PGL_DIAG_THREADS;
            const double v = p[s < S ? s : s0];
            a[u] = FOLD ? fabs(v - med) : v;
            lt[u] = eq[u] = 0;
        }
        for (int j = 0; j < S; ++j) {
            double v = p[j];
            if (FOLD) v = fabs(v - med);
#pragma unroll
            for (int u = 0; u < PGL_DIAG_OWN; ++u) {
                lt[u] += v < a[u];
                eq[u] += v == a[u];
            }
        }
#pragma unroll
        for (int u = 0; u < PGL_DIAG_OWN; ++u) {
            const int s = s0 + u * PGL_DIAG_THREADS;
            if (s < S) {
                y[s] = pgl_diag_score_counts(lt[u], eq[u], S);
                if (!FOLD) {
#pragma unroll
                    for (int q = 0; q < PGL_DIAG_NQ; ++q) {
                        // (tied draws all write: equal values, and + 0.0 makes a zero +0.0 whoever writes last)
                        if (lt[u] <= k0[q] && k0[q] < lt[u] + eq[u]) osq[q] = a[u] + 0.0;
                        if (lt[u] <= k1[q] && k1[q] < lt[u] + eq[u]) osq[PGL_DIAG_NQ + q] = a[u] + 0.0;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// Split-R-hat and, with want_ess, ESS and truncation lag of the series in y (centred in place).  Every thread returns the
// same values.  Ends with a barrier: y, cm, ac, am and red are free again.
__device__ __forceinline__ void diag_series(double* y, double* cm, double* ac, double* red, double* am, double* s_bh, int n,
                                            int C, int L, bool want_ess, double& rhat, double& ess, double& lag)
{
    const int t = threadIdx.x, h = n / 2, m = 2 * C;
    int G = 1;
    while (2 * G * m <= PGL_DIAG_THREADS) G *= 2;
    const int slots = PGL_DIAG_THREADS / G, jl = t / G, g = t % G;
    for (int j0 = 0; j0 < m; j0 += slots) {                    // (uniform)
        const int j = j0 + jl;
        double s = 0.0;
        if (j < m) {
            const double* c = y + pgl_diag_split_base(j, n, h);
            for (int i = g; i < h; i += G) s += c[i];
        }
        red[t] = s;
        __syncthreads();
        for (int w = G / 2; w > 0; w >>= 1) {
            if (g < w) red[t] += red[t + w];
            __syncthreads();
        }
        if (j < m && g == 0) cm[j] = red[t] / (double)h;
        __syncthreads();
    }
    for (int e = t; e < m * h; e += PGL_DIAG_THREADS) {
        const int j = e / h, i = e - j * h;
        y[pgl_diag_split_base(j, n, h) + i] -= cm[j];
    }
    if (t == 0) {
        double mm = 0.0, bh = 0.0;
        for (int j = 0; j < m; ++j) mm += cm[j];
        mm /= (double)m;
        for (int j = 0; j < m; ++j) bh += (cm[j] - mm) * (cm[j] - mm);
        *s_bh = bh / (double)(m - 1);
    }
    __syncthreads();
    const double bh = *s_bh;
    const int nl = want_ess ? L : 1;                           // lags computed per batch
    PglGeyer gy;
    double W = 0.0, vp = 0.0;
    ess = 0.0;
    lag = 0.0;
    for (int t0 = 0;; t0 += L) {                               // (every exit is uniform)
        for (int w = t; w < m * nl; w += PGL_DIAG_THREADS) {
            const int j = w / nl, tl = w - j * nl, d = t0 + tl;
            double a = 0.0;
            if (d < h) {
                const double* c = y + pgl_diag_split_base(j, n, h);
                for (int i = 0; i + d < h; ++i) a = fma(c[i], c[i + d], a);
            }
            ac[tl * m + j] = a / (double)h;
        }
        __syncthreads();
        if (t < nl) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += ac[t * m + j];
            am[t] = s / (double)m;
        }
        __syncthreads();
        bool more = false;
        if (t0 == 0) {
            W = am[0] * (double)h / (double)(h - 1);
            vp = W * (double)(h - 1) / (double)h + bh;
            rhat = pgl_diag_rhat(W, vp);
        }
        if (want_ess && vp > 0.0) {
            if (t0 == 0) pgl_geyer_init(&gy, h, pgl_diag_rho(W, am[1], vp));
            while (pgl_geyer_wants(&gy) && gy.t + 3 < t0 + L) {
                const double e = pgl_diag_rho(W, am[gy.t + 2 - t0], vp), o = pgl_diag_rho(W, am[gy.t + 3 - t0], vp);
                pgl_geyer_push(&gy, e, o);
            }
            more = pgl_geyer_wants(&gy);
            if (!more) ess = pgl_geyer_ess(&gy, (double)m * (double)h, &lag);
        }
        __syncthreads();
        if (!more) break;
    }
}

__global__ __launch_bounds__(PGL_DIAG_THREADS) void k_diag_column(const double* __restrict__ x, int n, int C, long long K,
                                                                   long long ld, double* __restrict__ out)
{
    extern __shared__ double diag_dyn[];
    __shared__ double red[PGL_DIAG_THREADS], am[PGL_DIAG_MAX_LAGS], osq[2 * PGL_DIAG_NQ];
    __shared__ double s_bh;
    __shared__ long long s_bad;
    const int S = n * C, m = 2 * C, L = diag_batch_lags(m);
    double* p = diag_dyn;
    double* y = p + S;
    double* cm = y + S;
    double* ac = cm + m;
    const int t = threadIdx.x;
    const long long k = blockIdx.x;
    const double* col = x + k;
    const double nan = __builtin_nan("");

    if (t == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    double lo = (double)INFINITY, hi = -(double)INFINITY;
    for (int s = t; s < S; s += PGL_DIAG_THREADS) {
        const int c = s / n, i = s - c * n;
        const double v = col[((size_t)i * C + c) * ld];
        p[s] = v;
        bad |= !pgl_hmc_finite(v);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                               // (uniform over the workgroup)
        if (t < PGL_DIAG_NOUT) out[(size_t)t * K + k] = nan;
        return;
    }
    lo = psis_reduce(lo, red, PsisMin());
    hi = psis_reduce(hi, red, PsisMax());
    if (lo == hi) {                                            // (uniform)
        if (t < PGL_DIAG_NOUT) {
            const bool is_c = t == PGL_DIAG_MEAN || t == PGL_DIAG_MEDIAN || t == PGL_DIAG_Q025 || t == PGL_DIAG_Q975;
            const bool is_nan = t == PGL_DIAG_RHAT_PLAIN || t == PGL_DIAG_RHAT || t == PGL_DIAG_MCSE_MEAN;
            out[(size_t)t * K + k] = is_c ? lo + 0.0 : (is_nan ? nan : 0.0);
        }
        return;
    }
    double v = 0.0;
    for (int s = t; s < S; s += PGL_DIAG_THREADS) v += p[s];
    const double mean = psis_reduce(v, red, PsisSum()) / (double)S;
    v = 0.0;
    for (int s = t; s < S; s += PGL_DIAG_THREADS) v += (p[s] - mean) * (p[s] - mean);
    const double sd = sqrt(psis_reduce(v, red, PsisSum()) / (double)(S - 1));

    diag_walk<false>(p, y, S, 0.0, osq);
    double Q[PGL_DIAG_NQ];
#pragma unroll
    for (int q = 0; q < PGL_DIAG_NQ; ++q) Q[q] = pgl_diag_lerp(osq[q], osq[PGL_DIAG_NQ + q], pgl_diag_q_frac(q, S));
    double rhat_bulk, rhat_fold, rhat_plain, ess_bulk, ess_lo, ess_hi, ess_mean, lag_bulk, lag_lo, lag_hi, lag_mean, du0, du1;
    diag_series(y, cm, ac, red, am, &s_bh, n, C, L, true, rhat_bulk, ess_bulk, lag_bulk);
    diag_walk<true>(p, y, S, Q[2], osq);
    diag_series(y, cm, ac, red, am, &s_bh, n, C, L, false, rhat_fold, du0, du1);
    for (int s = t; s < S; s += PGL_DIAG_THREADS) y[s] = p[s] <= Q[1] ? 1.0 : 0.0;
    __syncthreads();
    diag_series(y, cm, ac, red, am, &s_bh, n, C, L, true, du0, ess_lo, lag_lo);
    for (int s = t; s < S; s += PGL_DIAG_THREADS) y[s] = p[s] <= Q[3] ? 1.0 : 0.0;
    __syncthreads();
    diag_series(y, cm, ac, red, am, &s_bh, n, C, L, true, du0, ess_hi, lag_hi);
    for (int s = t; s < S; s += PGL_DIAG_THREADS) y[s] = p[s];
    __syncthreads();
    diag_series(y, cm, ac, red, am, &s_bh, n, C, L, true, rhat_plain, ess_mean, lag_mean);
    if (t == 0) {
        const size_t Ks = (size_t)K;
        out[PGL_DIAG_MEAN * Ks + k] = mean;
        out[PGL_DIAG_SD * Ks + k] = sd;
        out[PGL_DIAG_MEDIAN * Ks + k] = Q[2];
        out[PGL_DIAG_Q025 * Ks + k] = Q[0];
        out[PGL_DIAG_Q975 * Ks + k] = Q[4];
        out[PGL_DIAG_RHAT_PLAIN * Ks + k] = rhat_plain;
        out[PGL_DIAG_RHAT * Ks + k] = pgl_diag_max_nan(rhat_bulk, rhat_fold);
        out[PGL_DIAG_ESS_BULK * Ks + k] = ess_bulk;
        out[PGL_DIAG_ESS_TAIL * Ks + k] = ess_lo < ess_hi ? ess_lo : ess_hi;
        out[PGL_DIAG_ESS_MEAN * Ks + k] = ess_mean;
        out[PGL_DIAG_MCSE_MEAN * Ks + k] = sd / sqrt(ess_mean);
        out[PGL_DIAG_LAG_BULK * Ks + k] = lag_bulk;
        out[PGL_DIAG_LAG_Q05 * Ks + k] = lag_lo;
        out[PGL_DIAG_LAG_Q95 * Ks + k] = lag_hi;
        out[PGL_DIAG_LAG_MEAN * Ks + k] = lag_mean;
    }
}
