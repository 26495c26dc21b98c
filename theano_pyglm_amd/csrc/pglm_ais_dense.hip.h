// annealed importance sampling with a dense mass matrix: k_tri_matvec_shared, k_ais_dense_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// The AIS run of pglm_ais.hip.h with the inverse mass matrix Sigma_i = W_i W_i^T of every NEURON i, W (M, P, P) lower
// triangular, shared by the K particles of the neuron (pglm_ais_dense.h: the transition runs in the whitened momentum
// r = W^T p, as the chain of pglm_hmc_dense.hip.h does).  The rows are particle-major, row = k M + i, so the K vectors that
// meet W_i lie M rows apart: the product is a triangular product with K right-hand sides.  A workgroup owns one (tile of
// 64 outputs, neuron) and produces that tile for all K particles from ONE read of its part of W_i -- the grid of
// k_tri_matvec, (tile, row), with the particles folded into the workgroup.  The kick and the drift are the products'
// epilogues: a leapfrog step is a row kernel and two product launches whatever K is.  Only j <= i of W is read.
// A transition starts with the chain's own k_hmc_dense_draw on pgl_ais_hmc_view.
// Every output is summed in the order of k_tri_matvec, which depends on P alone: row (k, i) of a K-particle call has the
// bits of the one-row k_tri_matvec call with W_i, for any K and M -- subset = batch, repeat = same bits.
// ---------------------------------------------------------------------------
#include "pglm_ais_dense.h"

#define PGL_TRI_SHARED_KC 8                    // most particles per pass over a part of W (the launcher: 1, 2, 4 or this)

// y_r = W_{r mod M} x_r (TRANS 0) or W^T x_r (TRANS 1), r = k M + m, for the neuron m = blockIdx.y and every particle k < K,
// outputs in tiles of 64 as k_tri_matvec deals them out (TRANS 0: output i to wave i mod 4, lanes along the row, then a
// butterfly; TRANS 1: lane l owns column c0 + l, wave w the rows c0 + w, c0 + w + 4, ..., the four sums met in LDS as
// (s0 + s1) + (s2 + s3)).  Each entry of W that is loaded meets KC particles: KC partial sums per lane in registers, KC
// sets per workgroup in LDS; K > KC is a loop over chunks of KC particles inside the workgroup (W then comes from cache
// once per further chunk).  A chunk's missing particles (K not a multiple of KC) recompute the chunk's first and store
// nothing.  step (K M): one per row.  EPI as k_tri_matvec.
// GUARD (k_smc_tri_matvec_shared, pglm_smc.hip.h): done (M), one flag per neuron; the workgroups of a done neuron compute
// nothing -- KICK leaves y as it is, DRIFT leaves y as it is and copies it to Xt.
template <int TRANS, int EPI, int KC, int GUARD>
__device__ __forceinline__ void pgl_tri_matvec_shared_body(const double* __restrict__ W, const double* __restrict__ x, const int K,
                                                           const int M, const int P, double* __restrict__ y,
                                                           double* __restrict__ Xt, const double* __restrict__ step,
                                                           const double scale, const double* __restrict__ done,
                                                           double (*part)[TRANS ? 4 : 1][PGL_TRI_TILE])
{
    constexpr int NW = TRANS ? 4 : 1;
    const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (GUARD && done[m] != 0.0) {
        if (EPI == PGL_TRI_DRIFT) {
            const int ntile = (P + PGL_TRI_TILE - 1) / PGL_TRI_TILE;
            for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x)
                for (int e = tid; e < K * PGL_TRI_TILE; e += 256) {
                    const int c = tile * PGL_TRI_TILE + e % PGL_TRI_TILE;
                    if (c >= P) continue;
                    const size_t o = ((size_t)(e / PGL_TRI_TILE) * M + m) * P;
                    Xt[o + c] = y[o + c];
                }
        }
        return;
    }
    const double* Wr = W + (size_t)m * P * P;
    const int ntile = (P + PGL_TRI_TILE - 1) / PGL_TRI_TILE;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int c0 = tile * PGL_TRI_TILE;
        for (int k0 = 0; k0 < K; k0 += KC) {
            const int kn = K - k0 < KC ? K - k0 : KC;
            const double* xk[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) xk[k] = x + ((size_t)(k0 + (k < kn ? k : 0)) * M + m) * P;
            if (TRANS == 0) {
                for (int kk = 0; kk < PGL_TRI_TILE / 4; ++kk) {
                    const int i = c0 + 4 * kk + wave;                          // (the same in every lane of the wave)
                    if (i >= P) break;
                    const double* w = Wr + (size_t)i * P;
                    double a[KC];
#pragma unroll
                    for (int k = 0; k < KC; ++k) a[k] = 0.0;
#pragma unroll 4
                    for (int j = lane; j <= i; j += 64) {                      // (pgl_hmcd_row_dot's terms, in its order)
                        const double wj = w[j];
#pragma unroll
                        for (int k = 0; k < KC; ++k) a[k] += wj * xk[k][j];
                    }
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        double b = a[k];
                        for (int s = 32; s > 0; s >>= 1) b += __shfl_xor(b, s, 64);
                        if (lane == 0) part[k][0][4 * kk + wave] = b;
                    }
                }
            } else {
                const int j = c0 + lane;
                double a[KC];
#pragma unroll
                for (int k = 0; k < KC; ++k) a[k] = 0.0;
                if (j < P) {
#pragma unroll 4
                    for (int i = c0 + wave; i < P; i += 4)                     // (pgl_hmcd_col_dot's terms, in its order)
                        if (i >= j) {
                            const double wij = Wr[(size_t)i * P + j];
#pragma unroll
                            for (int k = 0; k < KC; ++k) a[k] += wij * xk[k][i];
                        }
                }
#pragma unroll
                for (int k = 0; k < KC; ++k) part[k][wave][lane] = a[k];
            }
            __syncthreads();
            for (int e = tid; e < kn * PGL_TRI_TILE; e += 256) {
                const int k = e / PGL_TRI_TILE, t = e % PGL_TRI_TILE, c = c0 + t;
                if (c >= P) continue;
                const size_t row = (size_t)(k0 + k) * M + m, o = row * P;
                double a;
                if (TRANS) a = (part[k][0][t] + part[k][NW > 1 ? 1 : 0][t]) + (part[k][NW > 2 ? 2 : 0][t] + part[k][NW > 3 ? 3 : 0][t]);
                else a = part[k][0][t];
                if (EPI == PGL_TRI_KICK) y[o + c] = pgl_hmcd_kick(y[o + c], scale, step[row], a);
                else if (EPI == PGL_TRI_DRIFT) {
                    const double qn = pgl_hmcd_drift(y[o + c], step[row], a);
                    y[o + c] = qn;
                    Xt[o + c] = qn;
                } else y[o + c] = a;
            }
            __syncthreads();                                                   // part is free for the next chunk
        }
    }
}
template <int TRANS, int EPI, int KC>
__global__ __launch_bounds__(256) void k_tri_matvec_shared(const double* __restrict__ W, const double* __restrict__ x, const int K,
                                                           const int M, const int P, double* __restrict__ y,
                                                           double* __restrict__ Xt, const double* __restrict__ step,
                                                           const double scale)
{
    __shared__ double part[KC][TRANS ? 4 : 1][PGL_TRI_TILE];
    pgl_tri_matvec_shared_body<TRANS, EPI, KC, 0>(W, x, K, M, P, y, Xt, step, scale, nullptr, part);
}

// after the evaluation of all rows at Xt = q: gu = grad U_beta along the trajectory from grad = grad ll (left as it is);
// the kick's product reads gu next
// (the row bodies of this kernel and the next are shared with their guarded forms, k_smc_dense_target / _end of
// pglm_smc.hip.h, which pass the rows of a done neuron by)
__device__ __forceinline__ void pgl_ais_dense_target_row(const AisView& v, const double* __restrict__ grad, const BfgsPrior& q,
                                                         double* red)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)r * v.P;
    pgl_ais_target_row(v.q + o, grad + o, v.gu + o, v.sc[(size_t)12 * v.R + r], q, red, tid);
}
__global__ __launch_bounds__(256) void k_ais_dense_target(const AisView v, const double* __restrict__ grad, const BfgsPrior q)
{
    __shared__ double red[12];
    pgl_ais_dense_target_row(v, grad, q, red);
}

// end of a transition, after the last half kick: H1 from ll[row], the log prior at q (summed again, as k_ais_dense_target
// summed it: gu is rewritten with the same bits) and r, then pgl_ais_finish_row as the last branch of k_ais_leap
__device__ __forceinline__ void pgl_ais_dense_end_row(const AisView& v, const double* __restrict__ ll,
                                                      const double* __restrict__ grad, const BfgsPrior& q, const int adapt,
                                                      double* __restrict__ acc_out, double* __restrict__ step_out, double* red,
                                                      int* dec)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)r * v.P;
    const double lp1 = pgl_ais_target_row(v.q + o, grad + o, v.gu + o, v.sc[(size_t)12 * v.R + r], q, red, tid);
    __syncthreads();                                                           // red is free, gu of the row is in memory
    const double ks = pgl_hmc_end_kinetic<1>(v.p + o, nullptr, nullptr, 0.0, v.P, red, tid);
    pgl_ais_finish_row(v, r, ll[r], lp1, ks, grad + o, adapt, acc_out, step_out, dec, tid);
}
__global__ __launch_bounds__(256) void k_ais_dense_end(const AisView v, const double* __restrict__ ll,
                                                       const double* __restrict__ grad, const BfgsPrior q, const int adapt,
                                                       double* __restrict__ acc_out, double* __restrict__ step_out)
{
    __shared__ double red[12];
    __shared__ int dec;
    pgl_ais_dense_end_row(v, ll, grad, q, adapt, acc_out, step_out, red, &dec);
}
