// Goodness of fit on the device (rules: pglm_gof.h).
//   k_rcorr_chunk / k_rcorr_finish   the discrete-time corrected intervals: the CORR instantiations of the bodies of
//                     pglm_rescale.hip.h on the walk of pglm_binwalk.hip.h, around the same k_rescale_scan -- one read of the
//                     currents, no (nT, N) array; the rate is pgl_lambda_only's arithmetic, its log1p series chosen per lane for the
//                     pieces of the intervals and by the wave's vote for the chunk totals behind stats (pglm_rescale.hip.h says why);
//   k_ks_segment      the KS distance of segmented samples, one workgroup per segment: z = -expm1(-tau), the sorting
//                     network of pglm_gof.h in place on the segment's part of zs (the indices >= n of the padded index
//                     space are a virtual +inf and are never touched), D+ and D- by a fixed-order maximum.
// The network's steps of span < PGL_KS_TILE run on one tile at a time in LDS (4096 doubles, 32 KiB: no opt-in), the wider
// ones on global memory between workgroup barriers; its running time does not depend on the values.  Inside a tile the merges
// k = 2, 4 and the half-cleaners j = 2, 1 of every later merge run on the four consecutive elements a thread holds in
// registers; the half-cleaners j >= 32 read 32 consecutive doubles per half wave (one 256-byte bank row: conflict-free),
// j = 4, 8, 16 and the flip steps are two-way conflicted (docs/NOTEBOOK.md, "KS sort").
#pragma once
#include "pglm_gof.h"

#define PGL_KS_THREADS 1024
static_assert(PGL_KS_TILE == 4 * PGL_KS_THREADS, "a thread holds four consecutive elements of a tile");

template <int NLIN>
__global__ __launch_bounds__(256) void k_rcorr_chunk(const RescaleParams p)
{
    pgl_rescale_chunk_body<NLIN, true>(p);
}

__global__ __launch_bounds__(256) void k_rcorr_finish(const RescaleParams p)
{
    pgl_rescale_finish_body<true>(p);
}

struct KsParams {
    const double* tau;        // concatenated segments
    const long long* off;     // (M + 1)
    double* zs;               // the length of tau: z of every segment, sorted where the segment is valid
    double* ks;               // (M, 4): D, D+, D-, n
};

__device__ __forceinline__ void ks_cx(double& a, double& b)
{
    const bool sw = a > b;
    const double lo = sw ? b : a, hi = sw ? a : b;
    a = lo;
    b = hi;
}

// one step of the network on a tile in LDS: the flip step of merge kj (FLIP) or the half-cleaner of stride kj
template <bool FLIP>
__device__ __forceinline__ void ks_lds_step(double* s, const int kj)
{
#pragma unroll
    for (int r = 0; r < PGL_KS_TILE / 2 / PGL_KS_THREADS; ++r) {
        long long i, l;
        if (FLIP) pgl_gof_pair_flip(threadIdx.x + r * PGL_KS_THREADS, kj, &i, &l);
        else pgl_gof_pair_half(threadIdx.x + r * PGL_KS_THREADS, kj, &i, &l);
        const double a = s[i], b = s[l];
        if (a > b) {
            s[i] = b;
            s[l] = a;
        }
    }
    __syncthreads();
}

// the merges k = 2 and 4 (FIRST) or the half-cleaners j = 2, 1 of a later merge on the thread's four elements
template <bool FIRST>
__device__ __forceinline__ void ks_lds_regs(double* s)
{
    double* q = s + 4 * threadIdx.x;
    double v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    if (FIRST) {
        ks_cx(v0, v1); ks_cx(v2, v3);                 // k = 2
        ks_cx(v0, v3); ks_cx(v1, v2);                 // k = 4: flip
    } else {
        ks_cx(v0, v2); ks_cx(v1, v3);                 // j = 2
    }
    ks_cx(v0, v1); ks_cx(v2, v3);                     // j = 1
    q[0] = v0; q[1] = v1; q[2] = v2; q[3] = v3;
    __syncthreads();
}

// tile t of the segment <-> LDS, the indices >= n as +inf
__device__ __forceinline__ void ks_tile_load(double* s, const double* z, const long long n, const long long t)
{
#pragma unroll
    for (int r = 0; r < PGL_KS_TILE / PGL_KS_THREADS; ++r) {
        const int e = threadIdx.x + r * PGL_KS_THREADS;
        const long long i = t * PGL_KS_TILE + e;
        s[e] = (i < n) ? z[i] : __builtin_inf();
    }
    __syncthreads();
}
__device__ __forceinline__ void ks_tile_store(const double* s, double* z, const long long n, const long long t)
{
#pragma unroll
    for (int r = 0; r < PGL_KS_TILE / PGL_KS_THREADS; ++r) {
        const int e = threadIdx.x + r * PGL_KS_THREADS;
        const long long i = t * PGL_KS_TILE + e;
        if (i < n) z[i] = s[e];
    }
    __syncthreads();
}

// one step on global memory: pairs whose upper index is >= n hold the virtual +inf there and are in order
template <bool FLIP>
__device__ __forceinline__ void ks_global_step(double* z, const long long n, const long long P, const long long kj)
{
    for (long long p = threadIdx.x; p < P / 2; p += PGL_KS_THREADS) {
        long long i, l;
        if (FLIP) pgl_gof_pair_flip(p, kj, &i, &l);
        else pgl_gof_pair_half(p, kj, &i, &l);
        if (l < n) {
            const double a = z[i], b = z[l];
            if (a > b) {
                z[i] = b;
                z[l] = a;
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(PGL_KS_THREADS) void k_ks_segment(const KsParams p)
{
    __shared__ double s[PGL_KS_TILE];
    const long long o0 = p.off[blockIdx.x];
    const long long n = p.off[blockIdx.x + 1] - o0;
    const double* tau = p.tau + o0;
    double* z = p.zs + o0;
    double* out = p.ks + (size_t)blockIdx.x * PGL_KS_NOUT;
    int bad = 0;
    for (long long i = threadIdx.x; i < n; i += PGL_KS_THREADS) {
        const double t = tau[i];
        bad |= pgl_gof_bad(t);
        z[i] = pgl_gof_z(t);
    }
    bad = __syncthreads_or(bad);
    __syncthreads();
    if (n < 2 || bad) {                                              // (uniform over the workgroup)
        if (threadIdx.x == 0) {
            out[0] = out[1] = out[2] = __builtin_nan("");
            out[3] = (double)n;
        }
        return;
    }
    const long long P = pgl_gof_pow2(n);
    const long long ntiles = (n + PGL_KS_TILE - 1) / PGL_KS_TILE;
    // every merge up to the tile
    for (long long t = 0; t < ntiles; ++t) {
        ks_tile_load(s, z, n, t);
        ks_lds_regs<true>(s);
        for (int k = 8; k <= PGL_KS_TILE; k <<= 1) {
            ks_lds_step<true>(s, k);
            for (int j = k >> 2; j >= 4; j >>= 1) ks_lds_step<false>(s, j);
            ks_lds_regs<false>(s);
        }
        ks_tile_store(s, z, n, t);
    }
    // the wider merges: steps of span >= the tile on global memory, the rest tile by tile
    for (long long k = 2 * PGL_KS_TILE; k <= P; k <<= 1) {
        ks_global_step<true>(z, n, P, k);
        for (long long j = k >> 2; j >= PGL_KS_TILE; j >>= 1) ks_global_step<false>(z, n, P, j);
        for (long long t = 0; t < ntiles; ++t) {
            ks_tile_load(s, z, n, t);
            for (int j = PGL_KS_TILE / 2; j >= 4; j >>= 1) ks_lds_step<false>(s, j);
            ks_lds_regs<false>(s);
            ks_tile_store(s, z, n, t);
        }
    }
    // D+ and D-: thread t takes p = t, t + 1024, .. in ascending order, then a binary tree over the 1024 partial maxima
    double dp = -__builtin_inf(), dm = -__builtin_inf();
    for (long long i = threadIdx.x; i < n; i += PGL_KS_THREADS) {
        const double v = z[i];
        const double a = pgl_gof_dplus(v, i, n), b = pgl_gof_dminus(v, i, n);
        dp = a > dp ? a : dp;
        dm = b > dm ? b : dm;
    }
    s[threadIdx.x] = dp;
    s[PGL_KS_THREADS + threadIdx.x] = dm;
    __syncthreads();
    for (int w = PGL_KS_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double a = s[threadIdx.x + w], b = s[PGL_KS_THREADS + threadIdx.x + w];
            if (a > s[threadIdx.x]) s[threadIdx.x] = a;
            if (b > s[PGL_KS_THREADS + threadIdx.x]) s[PGL_KS_THREADS + threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = s[0] > s[PGL_KS_THREADS] ? s[0] : s[PGL_KS_THREADS];
        out[1] = s[0];
        out[2] = s[PGL_KS_THREADS];
        out[3] = (double)n;
    }
}
