// Wald statistics of the coupling groups on the device: k_wald_groups<B>, one wave per group, PGL_WALD_WAVES groups per
// workgroup, on a grid of (blocks of groups, rows).  The rule is pglm_wald.h's; this file owns the parallel form:
//   S       lane l of the wave walks the columns k = l, l + 64, ... <= o + B - 1.  At every column it loads the B entries
//           W[o + a][k] it may read (k <= o + a) -- one load instruction of the wave is 64 consecutive doubles of one row,
//           512 bytes -- and adds the B (B + 1) / 2 products of pairs into accumulators in registers (B is a template
//           argument: they are indexed statically).  Every entry of the group's rows is read once for S.  The lane sums are
//           combined by the tree of the rule with __shfl_down; lane 0 leaves S in the wave's part of LDS;
//   finish  lane 0 runs pgl_wald_finish on the LDS copy: var, the factor in place, y;
//   u       where d_u is given the wave walks the P columns of its row once more: the group's rows again for k < o + B (they
//           were just read by this wave) and zeros beyond.
// A row with d_info[m] != 0 gets NaN and its W and theta are not read.  No atomics; nothing depends on the grid or on the
// neighbours.
#pragma once

#include "pglm_wald.h"

#define PGL_WALD_WAVES 4
#define PGL_WALD_THREADS (PGL_WALD_WAVES * PGL_WALD_LANES)

struct WaldParams {
    const double* W;        // (M, P, ld)
    const double* theta;    // (M, P)
    const double* c;        // (B)
    const int* info;        // (M)
    double* out;            // (M, G, 4)
    double* u;              // null or (G M, P)
    long long P, ld;
    int M, first, G;
};

template <int B>
__global__ __launch_bounds__(PGL_WALD_THREADS) void k_wald_groups(WaldParams p)
{
    PGL_WALD_NOCONTRACT
    __shared__ double sS[PGL_WALD_WAVES][B * B], sy[PGL_WALD_WAVES][B];
    const int lane = threadIdx.x & (PGL_WALD_LANES - 1), wv = threadIdx.x / PGL_WALD_LANES;
    const int g = blockIdx.x * PGL_WALD_WAVES + wv, m = blockIdx.y;
    const bool live = g < p.G;
    const bool bad = p.info[m] != 0;                               // (uniform over the workgroup)
    const long long o = (long long)p.first + (long long)(live ? g : 0) * B;
    const double* W = p.W + (size_t)m * p.P * p.ld;
    double* out = p.out + ((size_t)m * p.G + (live ? g : 0)) * PGL_WALD_NOUT;
    double* u = p.u ? p.u + ((size_t)(live ? g : 0) * p.M + m) * p.P : nullptr;
    if (bad) {
        const double nan = __builtin_nan("");
        if (live) {
            if (lane < PGL_WALD_NOUT) out[lane] = nan;
            if (u) for (long long k = lane; k < p.P; k += PGL_WALD_LANES) u[k] = nan;
        }
        return;
    }
    if (live) {
        double acc[B * (B + 1) / 2];
#pragma unroll
        for (int q = 0; q < B * (B + 1) / 2; ++q) acc[q] = 0.0;
        for (long long k = lane; k < o + B; k += PGL_WALD_LANES) {
            double w[B];
#pragma unroll
            for (int a = 0; a < B; ++a) w[a] = k <= o + a ? W[(size_t)(o + a) * p.ld + k] : 0.0;
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    const double t = w[a] * w[b];
                    acc[a * (a + 1) / 2 + b] = acc[a * (a + 1) / 2 + b] + (k <= o + b ? t : 0.0);
                }
        }
#pragma unroll
        for (int a = 0; a < B; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                double v = acc[a * (a + 1) / 2 + b];
#pragma unroll
                for (int h = PGL_WALD_LANES / 2; h > 0; h >>= 1) v = v + __shfl_down(v, h);
                if (lane == 0) sS[wv][a * B + b] = v;
            }
    }
    __syncthreads();
    if (live && lane == 0) pgl_wald_finish(sS[wv], p.theta + (size_t)m * p.P + o, p.c, B, out, sy[wv]);
    __syncthreads();
    if (live && u)
        for (long long k = lane; k < p.P; k += PGL_WALD_LANES) u[k] = k < o + B ? pgl_wald_u(W, p.ld, o, B, sy[wv], k) : 0.0;
}

template <int B>
static void wald_launch_b(const WaldParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(k_wald_groups<B>, dim3((unsigned)((p.G + PGL_WALD_WAVES - 1) / PGL_WALD_WAVES), (unsigned)p.M),
                       dim3(PGL_WALD_THREADS), 0, stream, p);
}

// B in 1 .. PGL_WALD_MAX_B (the caller's check)
static void wald_launch(int B, const WaldParams& p, hipStream_t stream)
{
    switch (B) {
#define PGL_WALD_CASE(b) case b: wald_launch_b<b>(p, stream); break;
        PGL_WALD_CASE(1) PGL_WALD_CASE(2) PGL_WALD_CASE(3) PGL_WALD_CASE(4) PGL_WALD_CASE(5) PGL_WALD_CASE(6) PGL_WALD_CASE(7)
        PGL_WALD_CASE(8) PGL_WALD_CASE(9) PGL_WALD_CASE(10) PGL_WALD_CASE(11) PGL_WALD_CASE(12) PGL_WALD_CASE(13)
        PGL_WALD_CASE(14) PGL_WALD_CASE(15) PGL_WALD_CASE(16)
#undef PGL_WALD_CASE
    }
}
