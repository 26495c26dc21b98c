// lock-step HMC with a dense mass matrix: k_tri_matvec, k_hmc_dense_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// The chain of pglm_hmc.hip.h with the inverse mass matrix Sigma_m = W_m W_m^T of every row m, W (M, P, P) lower
// triangular (pglm_hmc_dense.h: the chain runs in the whitened momentum r = W^T p, so a leapfrog step is two triangular
// matrix-vector products per row, r -= eps W^T grad U and q += eps W r, and no solve).  The products stream W once each:
// they are bandwidth-bound (C3, M = 128, P = 641: 210 MB per product) and run on a grid of their own, (output tile, row),
// so that 32 rows fill the chip as well as 128 do -- one workgroup per row would pull a row's 1.6 MB through one CU.  The
// kick and the drift are the products' epilogues: a leapfrog step is the target kernel and two product launches, and
// nothing but the state block is written.  Only j <= i of W is read.
// Every output is summed in an order that depends on P alone (k_tri_matvec): subset = batch, repeat = same bits.
// ---------------------------------------------------------------------------
#include "pglm_hmc_dense.h"

#define PGL_TRI_TILE 64                        // outputs per workgroup and step of the tile loop
enum { PGL_TRI_STORE = 0, PGL_TRI_KICK = 1, PGL_TRI_DRIFT = 2 };

// y_m = W_m x_m (TRANS 0) or W_m^T x_m (TRANS 1) for every row m = blockIdx.y, outputs in tiles of 64: the workgroup takes
// the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (gridDim.x = the number of tiles: one each; 1: the whole row).
//   TRANS 0  output i belongs to wave i mod 4; its 64 lanes run along row i of W (lane l: j = l, l + 64, ... <= i), then a
//            butterfly over the wave.
//   TRANS 1  lane l of every wave owns column c0 + l and walks down the rows (wave w: i = c0 + w, c0 + w + 4, ... < P, a
//            term where i >= j); the four waves' sums meet in LDS as (s0 + s1) + (s2 + s3).
// Either way a wave reads 512 contiguous bytes of a row of W per load.
// EPI: STORE  y[m, c] = the product;
//      KICK   y = the momentum r:  r[m, c] -= scale step[m] product       (TRANS 1, x = grad U)
//      DRIFT  y = the point q:     q[m, c] += step[m] product, Xt[m, c] = q[m, c]   (TRANS 0, x = r)
template <int TRANS, int EPI>
__global__ __launch_bounds__(256) void k_tri_matvec(const double* __restrict__ W, const double* __restrict__ x, const int P,
                                                    double* __restrict__ y, double* __restrict__ Xt,
                                                    const double* __restrict__ step, const double scale)
{
    __shared__ double part[4][PGL_TRI_TILE];
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* Wr = W + (size_t)r * P * P;
    const double* xr = x + (size_t)r * P;
    const size_t o = (size_t)r * P;
    const int ntile = (P + PGL_TRI_TILE - 1) / PGL_TRI_TILE;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int c0 = tile * PGL_TRI_TILE;
        if (TRANS == 0) {
            for (int k = 0; k < PGL_TRI_TILE / 4; ++k) {
                const int i = c0 + 4 * k + wave;                               // (the same in every lane of the wave)
                if (i >= P) break;
                double a = pgl_hmcd_row_dot(Wr, P, i, xr, lane, 64);
                for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s, 64);
                if (lane == 0) part[0][4 * k + wave] = a;
            }
        } else {
            const int j = c0 + lane;
            part[wave][lane] = j < P ? pgl_hmcd_col_dot(Wr, P, j, xr, c0 + wave, 4) : 0.0;
        }
        __syncthreads();
        const int c = c0 + tid;
        if (tid < PGL_TRI_TILE && c < P) {
            const double a = TRANS ? (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]) : part[0][tid];
            if (EPI == PGL_TRI_KICK) y[o + c] = pgl_hmcd_kick(y[o + c], scale, step[r], a);
            else if (EPI == PGL_TRI_DRIFT) {
                const double qn = pgl_hmcd_drift(y[o + c], step[r], a);
                y[o + c] = qn;
                Xt[o + c] = qn;
            } else y[o + c] = a;
        }
        __syncthreads();                                                       // part is free for the next tile
    }
}

// start of a transition: the momentum r = z (the draws of k_hmc_begin), H0, q0 = q.  The half kick and the first drift
// are the two product launches behind it.
// GUARD (k_smc_dense_draw, pglm_smc.hip.h): done (n_done), one flag per neuron, row r belongs to neuron r mod n_done; a row
// of a done neuron is passed by.
template <int GUARD>
__device__ __forceinline__ void pgl_hmc_dense_draw_row(const HmcView& v, const double* __restrict__ done, const int n_done,
                                                       double* red)
{
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    if (GUARD && done[r % n_done] != 0.0) return;
    PglHmc s;
    pgl_hmc_load(v, r, &s);
    const pgl_hmc_u64 key = pgl_hmc_row_key(&s);
    double ks = 0.0;
    for (int c = tid; c < P; c += 256) {
        const double z = pgl_hmc_normal(key, (pgl_hmc_u64)c);
        ks += pgl_hmcd_kinetic_elem(z);
        v.p[o + c] = z;
        v.q0[o + c] = v.q[o + c];
    }
    ks = pgl_blk_sum(ks, red);
    if (tid == 0) {
        pgl_hmc_begin(&s, ks);
        v.sc[(size_t)1 * v.M + r] = s.H0;
    }
}
__global__ __launch_bounds__(256) void k_hmc_dense_draw(const HmcView v)
{
    __shared__ double red[12];
    pgl_hmc_dense_draw_row<0>(v, nullptr, 1, red);
}

// after ONE evaluation of all rows at Xt = q: (ll, grad) -> U, grad U in place (the kick's product reads grad U next)
__global__ __launch_bounds__(256) void k_hmc_dense_target(const HmcView v, double* __restrict__ ll, double* __restrict__ grad,
                                                          const BfgsPrior q)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)r * v.P;
    const double U1 = pgl_hmc_target_row(v.q + o, grad + o, ll[r], q, red, tid);
    if (tid == 0) ll[r] = U1;
}

// end of a transition, after the last half kick: H1 from U1 = ll[row] and r, then pgl_hmc_finish_row as the last branch of
// k_hmc_leap
__global__ __launch_bounds__(256) void k_hmc_dense_end(const HmcView v, const double* __restrict__ ll,
                                                       const double* __restrict__ grad, const int n_warmup,
                                                       double* __restrict__ sample_out)
{
    __shared__ double red[12];
    __shared__ int dec;
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)r * v.P;
    const double ks = pgl_hmc_end_kinetic<1>(v.p + o, nullptr, nullptr, 0.0, v.P, red, tid);
    pgl_hmc_finish_row(v, r, ll[r], ks, grad + o, n_warmup, sample_out, &dec, tid);
}
