// Stimulus decoding (the rules: pglm_decode.h): the objective F(u), its gradient and its Hessian-vector products with respect
// to the STIMULUS u (Tu, D) of a population with a 'basis' stimulus, the spikes and the parameters fixed.  Part of
// pglm_kernels.hip.h (included from there, in order; one translation unit).
//
// The hot path is the adjoint pair of the feature build (k_stim_conv): two convolutions over the (nT, N) plane,
//   k_dec_forward<nlin, mode>   I = K * s for 256-bin chunks x slabs of 64 neurons; a wave holds 16 bins of its 64 neurons, lane =
//                               neuron: the K slab of 32 taps and the 64 + 32 rows of s a sub-tile of 64 bins needs are staged in
//                               LDS (K conflict-free, s a broadcast), a thread keeps 16 accumulators and a window of 19 values
//                               of s in registers: 23 LDS reads per 64 FMAs.  Mode 0 adds the offset c, evaluates the rate and
//                               writes r and cc and the chunk's sum of the ll terms per neuron; the spike counts come from the
//                               event lists on the cursor of pgl_bin_walk.  Mode 1 writes cc o (K * v).
//   k_dec_backward              g_s = K^T y for tiles of 64 output bins, a gather: the same thread layout, over neuron slabs of
//                               64 (the 64 + 16 rows of y of a slab and 16 taps of K in LDS: (tile + Rt) x N would not fit), a
//                               thread's 16 partial sums of its neuron are added over the slab's lanes in lane order through
//                               LDS, the slabs in slab order.  Nothing is scattered.
// around them k_dec_filters (K), k_dec_offset (c = bias + GX0), k_dec_interp (L), k_dec_interp_t (L^T and the prior's gradient
// or product) and k_dec_sum (the chunk sums in a fixed order: chunks ascending per neuron, then neurons ascending; the prior's
// value).  All f64, no atomics, no scratch; every element has ONE thread and a fixed order of additions, so two calls give the
// same bits and a result does not depend on how many chunks or tiles a workgroup takes (DecParams::cut).
#pragma once

#include "pglm_decode.h"

#define PGL_DEC_TB 64             // bins of a sub-tile (4 waves x 16)
#define PGL_DEC_NS 64             // neurons of a slab: the lanes of a wave
#define PGL_DEC_TC 32             // taps of K staged at a time, forward
#define PGL_DEC_TCB 16            // the same, backward

struct DecParams {
    BinSource src;                // event lists (pglm_binwalk.hip.h); GX is not read
    const double* K;              // (Rt, D, N)
    const double* c;              // (nT, N) offset
    const double* s;              // (nT, D): L u (mode 0), L v (mode 1)
    const double* yin;            // (nT, N): what k_dec_backward correlates with K
    double* r;                    // (nT, N)
    double* cc;                   // (nT, N)
    double* y;                    // (nT, N) mode 1: cc o (K * v)
    double* part;                 // (nchunks, N) chunk sums of the ll terms
    double* gs;                   // (nT, D)
    long long nT;
    int N, Rt, D, cut;            // cut: chunks (forward) / tiles (backward) a workgroup takes, >= 1
    double dt;
};

template <int NLIN, int MODE>
__global__ __launch_bounds__(256) void k_dec_forward(const DecParams p)
{
    __shared__ double Ks[PGL_DEC_TC][PGL_DEC_NS];
    __shared__ double ss[PGL_DEC_TB + PGL_DEC_TC];
    __shared__ double red[4][PGL_DEC_NS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tb = w * 16;
    const int nslabs = (p.N + PGL_DEC_NS - 1) / PGL_DEC_NS;
    const int n0 = (int)(blockIdx.x % nslabs) * PGL_DEC_NS, n = n0 + lane;
    const bool has_n = n < p.N;
    const long long nchunks = (p.nT + PGL_DEC_CHUNK - 1) / PGL_DEC_CHUNK;
    for (int ic = 0; ic < p.cut; ++ic) {
        const long long chunk = (long long)(blockIdx.x / nslabs) * p.cut + ic;
        if (chunk >= nchunks) break;                                        // (the same for the whole workgroup)
        double llsum = 0.0;
        for (int sub = 0; sub < PGL_DEC_CHUNK / PGL_DEC_TB; ++sub) {
            const long long t0 = chunk * PGL_DEC_CHUNK + sub * PGL_DEC_TB;
            if (t0 >= p.nT) break;
            double acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = 0.0;
            for (int d = 0; d < p.D; ++d)
                for (int tau0 = 0; tau0 < p.Rt; tau0 += PGL_DEC_TC) {
                    __syncthreads();
                    for (int i = threadIdx.x; i < PGL_DEC_TC * PGL_DEC_NS; i += 256) {
                        const int e = i >> 6, l = i & 63;
                        Ks[e][l] = (tau0 + e < p.Rt && n0 + l < p.N) ? p.K[((size_t)(tau0 + e) * p.D + d) * p.N + n0 + l] : 0.0;
                    }
                    // ss[j] = s[t0 - tau0 - TC + j]: bin t0 + b at tap tau0 + e reads j = b - 1 - e + TC
                    for (int j = threadIdx.x; j < PGL_DEC_TB + PGL_DEC_TC; j += 256) {
                        const long long ts = t0 - tau0 - PGL_DEC_TC + j;
                        ss[j] = (ts >= 0 && ts < p.nT) ? p.s[(size_t)ts * p.D + d] : 0.0;
                    }
                    __syncthreads();
#pragma unroll 2
                    for (int e = 0; e < PGL_DEC_TC; e += 4) {
                        double W[19];
                        const int base = tb + PGL_DEC_TC - 4 - e;
#pragma unroll
                        for (int j = 0; j < 19; ++j) W[j] = ss[base + j];
#pragma unroll
                        for (int ee = 0; ee < 4; ++ee) {
                            const double kv = Ks[e + ee][lane];
#pragma unroll
                            for (int k = 0; k < 16; ++k) acc[k] = fma(kv, W[k + 3 - ee], acc[k]);
                        }
                    }
                }
            const long long tw = t0 + tb;
            if (has_n && tw < p.nT) {
                int eend = 0, ei = 0;
                int2 nx = make_int2(-1, 0);
                if (MODE == 0) {
                    ei = pgl_rs_first_event(p.src, n, tw, eend);
                    if (ei < eend) nx = p.src.spk[ei];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const long long t = tw + k;
                    if (t < p.nT) {
                        const size_t o = (size_t)t * p.N + n;
                        if (MODE == 0) {
                            int count = 0;
                            if (t == nx.x) {
                                count = nx.y;
                                ++ei;
                                nx = (ei < eend) ? p.src.spk[ei] : make_int2(-1, 0);
                            }
                            double term, r, cc;
                            pgl_dec_point(p.c[o] + acc[k], (double)count, NLIN, p.dt, &term, &r, &cc);
                            p.r[o] = r;
                            p.cc[o] = cc;
                            llsum += term;
                        } else {
                            p.y[o] = p.cc[o] * acc[k];
                        }
                    }
                }
            }
        }
        if (MODE == 0) {
            __syncthreads();
            red[w][lane] = llsum;
            __syncthreads();
            if (w == 0 && has_n) p.part[(size_t)chunk * p.N + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        }
    }
}

__global__ __launch_bounds__(256) void k_dec_backward(const DecParams p)
{
    __shared__ double Ks[PGL_DEC_TCB][PGL_DEC_NS];
    __shared__ double ys[(PGL_DEC_TB + PGL_DEC_TCB) * PGL_DEC_NS];          // rows of y; then the lanes' sums [lane][65]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tb = w * 16;
    const long long ntiles = (p.nT + PGL_DEC_TB - 1) / PGL_DEC_TB;
    for (int it = 0; it < p.cut; ++it) {
        const long long tile = (long long)blockIdx.x * p.cut + it;
        if (tile >= ntiles) break;                                          // (the same for the whole workgroup)
        const long long t0 = tile * PGL_DEC_TB;
        for (int d = 0; d < p.D; ++d) {
            double total = 0.0;                                             // of output bin t0 + threadIdx.x (threads 0 .. 63)
            for (int n0 = 0; n0 < p.N; n0 += PGL_DEC_NS) {
                double acc[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] = 0.0;
                for (int tau0 = 0; tau0 < p.Rt; tau0 += PGL_DEC_TCB) {
                    __syncthreads();
                    for (int i = threadIdx.x; i < PGL_DEC_TCB * PGL_DEC_NS; i += 256) {
                        const int e = i >> 6, l = i & 63;
                        Ks[e][l] = (tau0 + e < p.Rt && n0 + l < p.N) ? p.K[((size_t)(tau0 + e) * p.D + d) * p.N + n0 + l] : 0.0;
                    }
                    // row j = y[t0 + 1 + tau0 + j]: output bin t0 + b at tap tau0 + e reads j = b + e
                    for (int i = threadIdx.x; i < (PGL_DEC_TB + PGL_DEC_TCB) * PGL_DEC_NS; i += 256) {
                        const int j = i >> 6, l = i & 63;
                        const long long ty = t0 + 1 + tau0 + j;
                        ys[i] = (ty < p.nT && n0 + l < p.N) ? p.yin[(size_t)ty * p.N + n0 + l] : 0.0;
                    }
                    __syncthreads();
#pragma unroll 2
                    for (int e = 0; e < PGL_DEC_TCB; e += 4) {
                        double W[19];
#pragma unroll
                        for (int j = 0; j < 19; ++j) W[j] = ys[(tb + e + j) * PGL_DEC_NS + lane];
#pragma unroll
                        for (int ee = 0; ee < 4; ++ee) {
                            const double kv = Ks[e + ee][lane];
#pragma unroll
                            for (int k = 0; k < 16; ++k) acc[k] = fma(kv, W[k + ee], acc[k]);
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 16; ++k) ys[lane * 65 + tb + k] = acc[k];
                __syncthreads();
                if (threadIdx.x < PGL_DEC_TB) {
                    double sl = 0.0;
                    for (int l = 0; l < PGL_DEC_NS; ++l) sl += ys[l * 65 + threadIdx.x];
                    total += sl;
                }
            }
            if (threadIdx.x < PGL_DEC_TB && t0 + threadIdx.x < p.nT) p.gs[(size_t)(t0 + threadIdx.x) * p.D + d] = total;
        }
    }
}

// what the small kernels around the two convolutions read
struct DecAux {
    const double* a;              // k_dec_filters: basis (Rt, B); k_dec_offset: GX; k_dec_interp: u or v; k_dec_interp_t: gs; k_dec_sum: part
    const double* b;              // k_dec_filters, k_dec_offset: theta (N, P); k_dec_interp_t: u or v; k_dec_sum: u
    double* out;                  // K, c, s, the gradient or product (Tu, D), F
    double* col;                  // k_dec_sum: the neurons' sums (N)
    long long nT, Tu, nchunks;
    int N, D, B, P, Rt, q, xs;
    PglDecPrior prior;
    double center;                // k_dec_interp_t: mu for the gradient, 0 for the product
};

// K[tau, d, n] = sum_b basis[tau, b] theta[n, 1 + d B + b]
__global__ __launch_bounds__(256) void k_dec_filters(const DecAux p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (g >= (long long)p.Rt * p.D * p.N) return;
    const int n = (int)(g % p.N), d = (int)((g / p.N) % p.D), tau = (int)(g / ((long long)p.N * p.D));
    p.out[g] = pgl_dec_filter_at(p.a, p.B, p.b, p.P, tau, d, n);
}

// c[t, n] = bias_n + GX0[t, n]
__global__ __launch_bounds__(256) void k_dec_offset(const DecAux p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (g >= p.nT * p.N) return;
    const int n = (int)(g % p.N);
    p.out[g] = p.b[(size_t)n * p.P] + p.a[(size_t)(g / p.N) * p.xs + n];
}

// s = L u, (nT, D)
__global__ __launch_bounds__(256) void k_dec_interp(const DecAux p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (g >= p.nT * p.D) return;
    p.out[g] = pgl_dec_interp_at(p.a, p.Tu, p.D, p.q, g / p.D, (int)(g % p.D));
}

// out (Tu, D) = L^T gs + the prior's part: its gradient at b = u (center = mu) or its product with b = v (center = 0)
__global__ __launch_bounds__(256) void k_dec_interp_t(const DecAux p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (g >= p.Tu * p.D) return;
    const long long i = g / p.D;
    const int d = (int)(g % p.D);
    p.out[g] = pgl_dec_interp_t_at(p.a, p.nT, p.D, p.q, p.Tu, i, d) + pgl_dec_prior_lin(p.b, p.Tu, p.D, i, d, &p.prior, p.center);
}

// F[0 .. 2] = F, log likelihood, log prior.  One workgroup: a thread adds the chunk sums of its neurons in chunk order (col, N
// doubles), thread 0 the neurons in order; the prior's terms element e by thread e % 256 in order, then the 256 threads in order.
__global__ __launch_bounds__(256) void k_dec_sum(const DecAux p)
{
    __shared__ double red[256];
    for (int n = threadIdx.x; n < p.N; n += 256) {
        double a = 0.0;
        for (long long c = 0; c < p.nchunks; ++c) a += p.a[(size_t)c * p.N + n];
        p.col[n] = a;
    }
    double lp = 0.0;
    for (long long e = threadIdx.x; e < p.Tu * p.D; e += 256) lp += pgl_dec_prior_term(p.b, p.Tu, p.D, e / p.D, (int)(e % p.D), &p.prior);
    red[threadIdx.x] = lp;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ll = 0.0;
        for (int n = 0; n < p.N; ++n) ll += p.col[n];
        lp = 0.0;
        for (int j = 0; j < 256; ++j) lp += red[j];
        p.out[0] = ll + lp;
        p.out[1] = ll;
        p.out[2] = lp;
    }
}
