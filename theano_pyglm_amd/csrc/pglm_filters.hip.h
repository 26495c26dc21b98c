// Posterior bands of the filters on the device: k_filter_bands<B>, one workgroup of 256 threads per (group, row) on a grid of
// (groups, rows), reading the samplers' tensor (n, C M, P) where it lies.  The rule is pglm_filters.h's; this file owns the
// parallel form:
//   load     thread t reads the B weights of the pooled draws t, t + 256, ... (B consecutive doubles of a theta row; the
//            workgroups of adjacent groups run together and share the lines in L2) and, where they fit, leaves them in LDS
//            weight-major (wl[b S + s]: consecutive lanes, consecutive doubles, no bank conflict).  "Fit": the sort buffer and
//            the weights within PGL_FILT_LDS_BUDGET = 144 KiB, S B + Spad <= 18 432 doubles -- every B at S <= 1024, B <= 3 at
//            4 x 1000 draws.  Beyond that the weights are re-read per lag from the tensor (the group's S B doubles, at most
//            512 KiB, stay in L2 between the lags; the deviation DESIGN.md section 8 states).  A non-finite weight ends the
//            group with NaNs and info = 1;
//   lag      the S values of a lag go to the sort buffer v[Spad] (Spad: the next power of two, padded with +inf); a non-
//            finite value ends the lag with NaNs;
//   sums     piece j of 256 consecutive draws is summed ascending by thread j (at most 16 threads work: the order is the
//            rule's, and it is what the two passes cost), the piece sums are added in order by every thread alike;
//   band     a thread keeps d_s of its draws in registers (16 at S = 4096) and updates them from v before the sort;
//   sort     a bitonic network on v in LDS, one barrier per stage; thread q < 3 takes quantile q from the sorted values.
//            The effective weight is one more "lag" with the contrast as its basis row; d_s itself is sorted last.
// All f64, no atomics, no scratch; nothing depends on the grid or on the neighbours.
#pragma once

#include "pglm_filters.h"

#define PGL_FILT_THREADS 256
#define PGL_FILT_OWN (PGL_FILT_MAX_DRAWS / PGL_FILT_THREADS)
#define PGL_FILT_LDS_BUDGET (144 * 1024)

struct FiltParams {
    const double* x;        // (n, C M, P)
    const double* basis;    // (R, B)
    const double* c;        // (B)
    double* out;            // (M, G, R, 5)
    double* grp;            // (M, G, 8)
    double level;
    long long P;
    int n, C, M, first, G, R, Spad, resident;
};

static inline int filt_pad(long long S)
{
    int p = 2;
    while (p < S) p <<= 1;
    return p;
}
static inline bool filt_resident(long long S, int B) { return (size_t)(filt_pad(S) + S * B) * 8 <= PGL_FILT_LDS_BUDGET; }
static inline size_t filt_lds_bytes(long long S, int B) { return (size_t)(filt_pad(S) + (filt_resident(S, B) ? S * B : 0)) * 8; }

// the sum of the rule over v[0 .. S), the same value in every thread.  Ends with a barrier: red is free again.
__device__ __forceinline__ double filt_sum(const double* v, int S, double* red, int sq, double mean)
{
    const int t = threadIdx.x, np = (S + PGL_FILT_PIECE - 1) / PGL_FILT_PIECE;
    if (t < np) {
        const int lo = t * PGL_FILT_PIECE;
        red[t] = pgl_filt_piece(v, lo, lo + PGL_FILT_PIECE < S ? lo + PGL_FILT_PIECE : S, sq, mean);
    }
    __syncthreads();
    double s = 0.0;
    for (int j = 0; j < np; ++j) s = s + red[j];
    __syncthreads();
    return s;
}

// ascending bitonic network on v[0 .. Spad), Spad a power of two >= 2.  Ends with a barrier.
__device__ __forceinline__ void filt_sort(double* v, int Spad)
{
    for (int k = 2; k <= Spad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < Spad / 2; q += PGL_FILT_THREADS) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const double a = v[i], b = v[l];
                if ((a > b) == ((i & k) == 0)) {
                    v[i] = b;
                    v[l] = a;
                }
            }
            __syncthreads();
        }
}

// mean, sd, the three quantiles of v[0 .. S) into o5; with BAND the threads' d_s take this lag's ratios.  v is left sorted.
template <bool BAND>
__device__ __forceinline__ void filt_stats(double* v, int S, int Spad, double* red, double level, double* o5,
                                           double (&d)[PGL_FILT_OWN])
{
    const int t = threadIdx.x;
    const double mean = filt_sum(v, S, red, 0, 0.0) / (double)S;
    const double sd = pgl_filt_sd(filt_sum(v, S, red, 1, mean), S);
    if (BAND && sd > 0.0) {
#pragma unroll
        for (int u = 0; u < PGL_FILT_OWN; ++u) {
            const int s = t + u * PGL_FILT_THREADS;
            if (s < S) {
                const double r = pgl_filt_ratio(v[s], mean, sd);
                d[u] = r > d[u] ? r : d[u];
            }
        }
    }
    __syncthreads();
    filt_sort(v, Spad);
    if (t < 3) o5[2 + t] = pgl_filt_quantile(v, S, pgl_filt_prob(t, level));
    if (t == 3) {
        o5[0] = mean;
        o5[1] = sd;
    }
}

template <int B>
__global__ __launch_bounds__(PGL_FILT_THREADS) void k_filter_bands(FiltParams p)
{
    extern __shared__ double filt_dyn[];
    __shared__ double red[PGL_FILT_OWN];
    __shared__ int s_first;
    const int t = threadIdx.x, g = blockIdx.x, m = blockIdx.y;
    const int S = p.n * p.C, Spad = p.Spad, R = p.R;
    double* v = filt_dyn;
    double* wl = v + Spad;
    const size_t si = (size_t)p.C * p.M * p.P, sc = (size_t)p.M * p.P;
    const double* x = p.x + (size_t)m * p.P + p.first + (size_t)g * B;
    double* out = p.out + ((size_t)m * p.G + g) * R * PGL_FILT_NLAG;
    double* grp = p.grp + ((size_t)m * p.G + g) * PGL_FILT_NGRP;
    const double nan = __builtin_nan(""), inf = (double)INFINITY;

    int bad = 0;
    for (int s = t; s < S; s += PGL_FILT_THREADS) {
        const int c = s / p.n, i = s - c * p.n;
        const double* src = x + i * si + c * sc;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const double val = src[b];
            bad |= !pgl_hmc_finite(val);
            if (p.resident) wl[(size_t)b * S + s] = val;
        }
    }
    bad = __syncthreads_or(bad);                               // (a barrier: wl is visible)
    if (bad) {                                                 // (uniform over the workgroup)
        for (int q = t; q < R * PGL_FILT_NLAG; q += PGL_FILT_THREADS) out[q] = nan;
        if (t < PGL_FILT_NGRP) grp[t] = t == PGL_FILT_NGRP - 1 ? 1.0 : nan;
        return;
    }
    double d[PGL_FILT_OWN];
#pragma unroll
    for (int u = 0; u < PGL_FILT_OWN; ++u) d[u] = 0.0;
    for (int tau = 0; tau <= R; ++tau) {                       // tau = R: the effective weight
        const double* brow = tau < R ? p.basis + (size_t)tau * B : p.c;
        double* o5 = tau < R ? out + (size_t)tau * PGL_FILT_NLAG : grp + 1;
        int nf = 0;
        for (int s = t; s < Spad; s += PGL_FILT_THREADS) {
            double h = inf;
            if (s < S) {
                if (p.resident) {
                    h = pgl_filt_dot(brow, wl + s, S, B);
                } else {
                    const int c = s / p.n, i = s - c * p.n;
                    h = pgl_filt_dot(brow, x + i * si + c * sc, 1, B);
                }
                nf |= !pgl_hmc_finite(h);
            }
            v[s] = h;
        }
        nf = __syncthreads_or(nf);                             // (a barrier: v is visible)
        if (nf) {                                              // (uniform)
            if (t < PGL_FILT_NLAG) o5[t] = nan;
            if (tau == R && t == PGL_FILT_NLAG) grp[6] = nan;
            continue;
        }
        if (tau < R) {
            filt_stats<true>(v, S, Spad, red, p.level, o5, d);
        } else {
            filt_stats<false>(v, S, Spad, red, p.level, o5, d);
            if (t == 0) s_first = S;
            __syncthreads();
            for (int s = t; s < S; s += PGL_FILT_THREADS)      // the first positive of the sorted values: one writer
                if (v[s] > 0.0 && (s == 0 || !(v[s - 1] > 0.0))) s_first = s;
            __syncthreads();
            if (t == 0) grp[6] = (double)(S - s_first) / (double)S;
        }
        __syncthreads();                                       // (the quantiles are read: v is free again)
    }
#pragma unroll
    for (int u = 0; u < PGL_FILT_OWN; ++u) {
        const int s = t + u * PGL_FILT_THREADS;
        if (s < Spad) v[s] = s < S ? d[u] : inf;
    }
    __syncthreads();
    filt_sort(v, Spad);
    if (t == 0) {
        grp[0] = v[pgl_filt_rank(p.level, S) - 1] + 0.0;
        grp[PGL_FILT_NGRP - 1] = 0.0;
    }
}
