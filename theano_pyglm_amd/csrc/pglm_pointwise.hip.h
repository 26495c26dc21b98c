// Pointwise log-likelihood of a parameter draw, resolved in time: for every neuron the sums of
//     term_t = -dt * lam_t + S[t,n] * log lam_t,     lam_t = nlin(bias_n + GX[t][n]),
// over blocks of consecutive bins, from the bias-free total currents the forward-only pass leaves in GX and the per-neuron
// event lists -- the ll counterpart of pglm_rescale.hip.h, on the same chunks: PGL_RS_CHUNK bins counted from t_lo
// (pglm_binwalk.hip.h), a block = block_chunks consecutive chunks (the last block may be short), n_blocks = ceil(nchunks /
// block_chunks).  Given the spike history the conditional-intensity likelihood factorises over bins, so the block sums are
// proper pointwise terms for WAIC and their total is the ll of the range.  ONE read of GX, no (nT, N) array, two launches:
//   k_pw_chunk   time chunks x columns of GX, a thread per (chunk, neuron) on the walk of pglm_binwalk.hip.h: rate (all f64:
//                pgl_lambda_only), log lam = x for exp and pgl_log(lam) else, at the event bins only (a bin with S = 0
//                contributes -dt * lam: never a 0 * log 0), running sum, chunk total;
//   k_pw_block   one thread per (block, neuron): the block's chunk totals added in chunk order -> ll_blk[b][n], and, with an
//                accumulator, the fold of pglm_pointwise.h (running maximum, rescaled sum of exponentials, Welford mean and
//                M2 over the draws).  With long blocks this launch has few threads; it reads nchunks x N doubles.
// Every sum has a fixed order and nothing is atomic: the results are bit-reproducible from run to run.
#pragma once

#include "pglm_pointwise.h"

struct PointwiseParams {
    BinSource src;            // currents, biases, event lists, time range (pglm_binwalk.hip.h)
    double* part;             // (nchunks, xs) chunk sums
    double* ll_blk;           // (n_blocks, N) block sums, or null
    double* acc;              // (4, n_blocks, N) accumulator over draws, or null
    long long draw;
    int nchunks, block_chunks, n_blocks;
};

template <int NLIN>
__global__ __launch_bounds__(256) void k_pw_chunk(const PointwiseParams p)
{
    const BinSource& s = p.src;
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % s.xs);
    const long long c = g / s.xs;
    if (c >= p.nchunks || j >= s.N) return;
    const long long t0 = s.t_lo + c * PGL_RS_CHUNK;
    const int len = (int)((s.t_hi - t0 < PGL_RS_CHUNK) ? s.t_hi - t0 : PGL_RS_CHUNK);
    double acc = 0.0;
    pgl_bin_walk(
        s, j, t0, len, [](const double xv) { return pgl_lambda_only(xv, NLIN, PGL_C); },
        [&](int, const bool live, const double xv, const double lam, const bool event, const int count, int) {
            double term = -s.dt * lam;
            if (event) {
                const double loglam = (NLIN == 1) ? pgl_log(lam, PGL_C) : xv;
                term = fma((double)count, loglam, term);
            }
            acc += live ? term : 0.0;
        });
    p.part[(size_t)c * s.xs + j] = acc;
}

__global__ __launch_bounds__(256) void k_pw_block(const PointwiseParams p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % p.src.xs);
    const long long b = g / p.src.xs;
    if (b >= p.n_blocks || j >= p.src.N) return;
    const long long c0 = b * p.block_chunks;
    const long long c1 = (c0 + p.block_chunks < p.nchunks) ? c0 + p.block_chunks : p.nchunks;
    double l = 0.0;
    for (long long c = c0; c < c1; ++c) l += p.part[(size_t)c * p.src.xs + j];
    const size_t o = (size_t)b * p.src.N + j;
    if (p.ll_blk) p.ll_blk[o] = l;
    if (p.acc) {
        const size_t pl = (size_t)p.n_blocks * p.src.N;
        double m = p.acc[o], e = p.acc[pl + o], mean = p.acc[2 * pl + o], m2 = p.acc[3 * pl + o];
        pgl_pw_fold(l, p.draw, &m, &e, &mean, &m2);
        p.acc[o] = m; p.acc[pl + o] = e; p.acc[2 * pl + o] = mean; p.acc[3 * pl + o] = m2;
    }
}
