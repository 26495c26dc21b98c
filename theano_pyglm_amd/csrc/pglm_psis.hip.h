// PSIS-LOO on the device: k_psis_column, one workgroup of 256 threads per column of the (S, C) matrix of pointwise
// log-likelihoods (element [s, c] at s * ld + c), the column resident in LDS.  The rule of a column and the scalar pieces
// are pglm_psis.h's; this file owns the parallel form:
//   load      thread t reads draws t, t + 256, ... (a stride-ld read; adjacent columns belong to adjacent workgroups, which
//             run together and share the lines in L2) into l[S]; a non-finite value anywhere ends the column with NaNs;
//   order     rank by counting, on the raw doubles: pos(s) = #{j : l_j > l_s or (l_j == l_s and j < s)}.  A thread holds
//             four of its draws in registers and walks l[0 .. S) once for them (every lane reads the same address: an LDS
//             broadcast).  S^2 comparisons per column, no data movement, no barrier inside, and the order of step 2 of
//             the rule by construction;
//   tail      the thread that owns rank S - M - 1 publishes the cutoff; n = #{l_s < l_cut} by a tree; the owner of rank
//             S - n + i writes excess i;
//   fit       candidate i belongs to lanes 4 i .. 4 i + 3: lane g adds log1p(-b_i e_j) over j = g, g + 4, ... ascending, the
//             four partial sums combine as (p0 + p1) + (p2 + p3).  All m <= 64 candidates run at once.  The weights (m
//             exponentials each) are one thread per candidate, the posterior mean serial (pgl_psis_posterior_b);
//   sums      over the tail (one element per thread) and over the draws (thread t adds t, t + 256, ... ascending): 256
//             partial values, combined by a binary tree in LDS: red[t] += red[t + h], h = 128, 64, .. 1.
// No atomics, nothing depends on the launch shape or on the neighbours: a column gives the same bits alone and among
// others, run after run.
#pragma once

#include "pglm_psis.h"

#define PGL_PSIS_THREADS 256
#define PGL_PSIS_OWN 4          // draws a thread ranks per walk over the column

struct PsisSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct PsisMax { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };
struct PsisMin { __device__ double operator()(double a, double b) const { return a < b ? a : b; } };

template <class Op>
__device__ __forceinline__ double psis_reduce(double v, double* red, Op op)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = PGL_PSIS_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] = op(red[t], red[t + h]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// bytes of dynamic LDS for S draws: l[S] doubles, then pos[S] ints
static inline size_t psis_lds_bytes(long long S) { return (size_t)S * 8 + (size_t)((S + 1) & ~1LL) * 4; }

__global__ __launch_bounds__(PGL_PSIS_THREADS) void k_psis_column(const double* __restrict__ ll, long long S, long long C,
                                                                   long long ld, double* __restrict__ out,
                                                                   double* __restrict__ lw)
{
    extern __shared__ double psis_dyn[];
    __shared__ double e[PGL_PSIS_MAX_TAIL], sm[PGL_PSIS_MAX_TAIL], red[PGL_PSIS_THREADS];
    __shared__ double cb[PGL_PSIS_MAX_CAND], cL[PGL_PSIS_MAX_CAND], cw[PGL_PSIS_MAX_CAND];
    __shared__ double s_lcut;
    __shared__ int s_bad;
    double* l = psis_dyn;
    int* pos = (int*)(psis_dyn + S);
    const int t = threadIdx.x;
    const long long c = blockIdx.x;
    const double* col = ll + c;
    const int n_s = (int)S;

    if (t == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    double lmin = (double)INFINITY;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) {
        const double v = col[(size_t)s * ld];
        l[s] = v;
        bad |= !pgl_hmc_finite(v);
        lmin = v < lmin ? v : lmin;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                               // (uniform over the workgroup)
        const double nan = __builtin_nan("");
        if (t < PGL_PSIS_NOUT) out[(size_t)t * C + c] = nan;
        if (lw) for (int s = t; s < n_s; s += PGL_PSIS_THREADS) lw[(size_t)s * ld + c] = nan;
        return;
    }
    const double rmax = -psis_reduce(lmin, red, PsisMin());

    // ---- order: ranks on the raw doubles ----
    for (int s0 = t; s0 < n_s; s0 += PGL_PSIS_OWN * PGL_PSIS_THREADS) {
        double a[PGL_PSIS_OWN];
        int p[PGL_PSIS_OWN];
#pragma unroll
        for (int u = 0; u < PGL_PSIS_OWN; ++u) {
            const int s = s0 + u * PGL_PSIS_THREADS;
            a[u] = l[s < n_s ? s : s0];
            p[u] = 0;
        }
        for (int j = 0; j < n_s; ++j) {
            const double v = l[j];
#pragma unroll
            for (int u = 0; u < PGL_PSIS_OWN; ++u) p[u] += (v > a[u]) || (v == a[u] && j < s0 + u * PGL_PSIS_THREADS);
        }
#pragma unroll
        for (int u = 0; u < PGL_PSIS_OWN; ++u) {
            const int s = s0 + u * PGL_PSIS_THREADS;
            if (s < n_s) pos[s] = p[u];
        }
    }
    __syncthreads();

    // ---- tail ----
    const int M = (int)pgl_psis_tail_len(S);
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) if (pos[s] == n_s - M - 1) s_lcut = l[s];
    __syncthreads();
    const double l_cut = s_lcut;
    double cnt = 0.0;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) cnt += (l[s] < l_cut) ? 1.0 : 0.0;
    const int n = (int)psis_reduce(cnt, red, PsisSum());      // (integers in doubles: exact)
    const int t0 = n_s - n;                                    // the first rank of the tail
    const double x_cut = pgl_psis_cutoff(l_cut, rmax), exp_cut = exp(x_cut);
    double khat = (double)INFINITY;
    int smooth = 0;
    if (n >= PGL_PSIS_MIN_TAIL) {                              // (uniform)
        for (int s = t; s < n_s; s += PGL_PSIS_THREADS) if (pos[s] >= t0) e[pos[s] - t0] = exp(-l[s] - rmax) - exp_cut;
        __syncthreads();
        const int m = pgl_psis_candidates(n);
        {
            const int i = t >> 2, g = t & 3;
            double b = 0.0, k = 0.0;
            if (i < m) {
                b = pgl_psis_cand(i + 1, m, e[n - 1], e[pgl_psis_quartile(n) - 1]);
                for (int j = g; j < n; j += 4) k += log1p(-b * e[j]);
            }
            red[t] = k;
            __syncthreads();
            if (i < m && g == 0) {
                k = (red[t] + red[t + 1]) + (red[t + 2] + red[t + 3]);
                cb[i] = b;
                cL[i] = pgl_psis_profile(b, k / (double)n, n);
            }
            __syncthreads();
        }
        if (t < m) cw[t] = pgl_psis_weight(cL, m, t);
        __syncthreads();
        const double bp = pgl_psis_posterior_b(cw, cb, m);
        const double k = psis_reduce(t < n ? log1p(-bp * e[t]) : 0.0, red, PsisSum()) / (double)n;
        const double sigma = -k / bp;
        khat = pgl_psis_khat(k, n);
        smooth = pgl_hmc_finite(khat);
        if (smooth && t < n) sm[t] = pgl_psis_smoothed(t, n, khat, sigma, exp_cut);
        __syncthreads();
    }

    // ---- truncate, normalise, outputs ----
#define PSIS_X(s, x)                                                             \
    double x = (smooth && pos[s] >= t0) ? sm[pos[s] - t0] : -l[s] - rmax;       \
    x = pgl_psis_truncate(x)
    double v = -(double)INFINITY;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) { PSIS_X(s, x); v = x > v ? x : v; }
    const double mx = psis_reduce(v, red, PsisMax());
    v = 0.0;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) { PSIS_X(s, x); v += exp(x - mx); }
    const double lse = mx + log(psis_reduce(v, red, PsisSum()));
    v = -(double)INFINITY;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) { PSIS_X(s, x); const double q = x - lse + l[s]; v = q > v ? q : v; }
    const double a = psis_reduce(v, red, PsisMax());
    double se = 0.0, s2 = 0.0;
    for (int s = t; s < n_s; s += PGL_PSIS_THREADS) {
        PSIS_X(s, x);
        const double w = x - lse;
        se += exp(w + l[s] - a);
        s2 += exp(2.0 * w);
        if (lw) lw[(size_t)s * ld + c] = w;
    }
#undef PSIS_X
    se = psis_reduce(se, red, PsisSum());
    s2 = psis_reduce(s2, red, PsisSum());
    if (t == 0) {
        out[c] = a + log(se);
        out[(size_t)C + c] = khat;
        out[2 * (size_t)C + c] = 1.0 / s2;
        out[3 * (size_t)C + c] = (double)n;
    }
}
