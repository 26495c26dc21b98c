// Independence of the rescaled intervals on the device (rules: pglm_acf.h).
//   k_acf_segment     one workgroup per segment, f64 throughout, no atomics, two passes over tiles of PGL_ACF_TILE pieces:
//     pass 1  the scores g_i = pgl_acf_score(tau_i) into d_scores (every element of the segment, void or not) and a tile of them
//             into LDS; thread j sums piece j of the tile in ascending i, thread 0 adds the piece totals in ascending piece order:
//             the mean.
//     pass 2  the work item is (piece, lag), lag 0 being c_0.  Every piece of the tile is staged with its own window of
//             PGL_ACF_PIECE + L centred scores d_i = g_i - mean (read back from d_scores: once per piece, not once per lag) and
//             the index of every element's run inside the segment (-1 behind the segment's end), found by bisection of run_off;
//             the pair (i, i + k) counts where the two run indices are equal.  An item walks its piece in ascending i, product
//             and sum rounded apart (pgl_acf_madd); thread k then adds the tile's piece totals of lag k in ascending piece order
//             to the running c_k and n_k it keeps in registers.
//   Thread 0 ends with pgl_acf_finish.  A segment may have any length: the tiles are walked in a loop.  The running time depends
//   on the offsets and on L, not on the values: a void segment is computed like any other and voided at the end.
// LDS: the windows of a tile lie at a stride of PGL_ACF_PIECE + PGL_ACF_MAX_LAG + ((L + 1) mod 32) doubles.  Consecutive items
// (piece, k) of a wave are consecutive in k and then in piece, so with that stride the item (piece, k) reads the double at
// piece (L + 1) + k + i modulo 32 in step i: the 32 lanes of a half wave read 32 consecutive doubles modulo the 256-byte bank
// row -- no 64-bit bank conflict whatever L is -- and the d_i of a piece is one broadcast address per piece.  The run indices
// (ints at the same stride) follow the same pattern at half the width.  Pass 1 stages at a stride of PGL_ACF_PIECE + 1.
// 22.0 KiB of doubles, 11.0 KiB of ints and 7.1 KiB of totals: 40.1 KiB of static LDS, no opt-in.
#pragma once
#include "pglm_acf.h"

#define PGL_ACF_THREADS 256
#define PGL_ACF_TILE 8                                                         // pieces of a tile
#define PGL_ACF_STRIDE_MAX (PGL_ACF_PIECE + PGL_ACF_MAX_LAG + 32)              // doubles between the windows of two pieces
static_assert(PGL_ACF_TILE * (PGL_ACF_PIECE + 1) <= PGL_ACF_TILE * PGL_ACF_STRIDE_MAX, "pass 1 stages into the same buffer");
static_assert(PGL_ACF_MAX_LAG + 1 <= PGL_ACF_THREADS && PGL_ACF_TILE <= PGL_ACF_THREADS, "a thread per lag, a thread per piece");

struct AcfParams {
    const double* tau;            // concatenated runs
    const long long* run_off;     // (R + 1)
    const long long* seg_run;     // (M + 1)
    double* scores;               // the length of tau
    double* out;                  // (M, PGL_ACF_NHEAD + L)
    int L;
};

__global__ __launch_bounds__(PGL_ACF_THREADS) void k_acf_segment(const AcfParams p)
{
    __shared__ double sd[PGL_ACF_TILE * PGL_ACF_STRIDE_MAX];
    __shared__ int sr[PGL_ACF_TILE * PGL_ACF_STRIDE_MAX];
    __shared__ double spt[PGL_ACF_TILE * (PGL_ACF_MAX_LAG + 1)];
    __shared__ int scn[PGL_ACF_TILE * (PGL_ACF_MAX_LAG + 1)];
    __shared__ double sacc[PGL_ACF_MAX_LAG + 1];
    __shared__ long long scnt[PGL_ACF_MAX_LAG + 1];
    __shared__ double smean;
    const int L = p.L, tid = threadIdx.x;
    const long long r0 = p.seg_run[blockIdx.x], r1 = p.seg_run[blockIdx.x + 1];
    const long long o0 = p.run_off[r0], n = p.run_off[r1] - o0;
    const long long tile_elems = (long long)PGL_ACF_TILE * PGL_ACF_PIECE;
    const long long ntile = n > 0 ? (n + tile_elems - 1) / tile_elems : 0;
    const double* tau = p.tau + o0;
    double* g = p.scores + o0;

    // ---- pass 1: scores and their mean --------------------------------------------------------------------------------------
    int bad = 0;
    double acc = 0.0;
    for (long long t = 0; t < ntile; ++t) {
        const long long base = t * tile_elems;
        for (int e = tid; e < PGL_ACF_TILE * PGL_ACF_PIECE; e += PGL_ACF_THREADS) {
            const long long i = base + e;
            double v = 0.0;
            if (i < n) {
                const double x = tau[i];
                bad |= pgl_gof_bad(x);
                v = pgl_acf_score(x);
                g[i] = v;
            }
            sd[(e / PGL_ACF_PIECE) * (PGL_ACF_PIECE + 1) + (e % PGL_ACF_PIECE)] = v;
        }
        __syncthreads();
        if (tid < PGL_ACF_TILE) {
            const long long left = n - (base + (long long)tid * PGL_ACF_PIECE);
            const int len = left < PGL_ACF_PIECE ? (left > 0 ? (int)left : 0) : PGL_ACF_PIECE;
            const double* s = sd + tid * (PGL_ACF_PIECE + 1);
            double a = 0.0;
            for (int i = 0; i < len; ++i) a = pgl_acf_add(a, s[i]);
            spt[tid] = a;
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < PGL_ACF_TILE && base + (long long)j * PGL_ACF_PIECE < n; ++j) acc = pgl_acf_add(acc, spt[j]);
    }
    if (tid == 0) smean = pgl_acf_mean(acc, n);
    bad = __syncthreads_or(bad);                       // (a barrier: the mean and every score of the segment are visible)
    const double mean = smean;

    // ---- pass 2: the lagged products ----------------------------------------------------------------------------------------
    const int PS = PGL_ACF_PIECE + PGL_ACF_MAX_LAG + ((L + 1) & 31), W = PGL_ACF_PIECE + L, nitem = PGL_ACF_TILE * (L + 1);
    long long cnt = 0;
    acc = 0.0;
    for (long long t = 0; t < ntile; ++t) {
        const long long base = t * tile_elems;
        for (int e = tid; e < PGL_ACF_TILE * W; e += PGL_ACF_THREADS) {
            const int pl = e / W, w = e - pl * W;
            const long long i = base + (long long)pl * PGL_ACF_PIECE + w;
            double d = 0.0;
            int rid = -1;
            if (i < n) {
                d = pgl_acf_centre(g[i], mean);
                long long lo = r0, hi = r1;            // the last run that starts at or before o0 + i: the one that holds it
                while (hi - lo > 1) {
                    const long long mid = lo + ((hi - lo) >> 1);
                    if (p.run_off[mid] <= o0 + i) lo = mid;
                    else hi = mid;
                }
                rid = (int)(lo - r0);
            }
            sd[pl * PS + w] = d;
            sr[pl * PS + w] = rid;
        }
        __syncthreads();
        for (int it = tid; it < nitem; it += PGL_ACF_THREADS) {
            const int pl = it / (L + 1), k = it - pl * (L + 1);
            const long long left = n - (base + (long long)pl * PGL_ACF_PIECE);
            const int len = left < PGL_ACF_PIECE ? (left > 0 ? (int)left : 0) : PGL_ACF_PIECE;
            const double* s = sd + pl * PS;
            const int* r = sr + pl * PS;
            double a = 0.0;
            int c = 0;
            for (int i = 0; i < len; ++i) {
                const bool ok = r[i] == r[i + k];
                const double a1 = pgl_acf_madd(a, s[i], s[i + k]);
                a = ok ? a1 : a;
                c += ok ? 1 : 0;
            }
            spt[pl * (PGL_ACF_MAX_LAG + 1) + k] = a;
            scn[pl * (PGL_ACF_MAX_LAG + 1) + k] = c;
        }
        __syncthreads();
        if (tid <= L)
            for (int j = 0; j < PGL_ACF_TILE && base + (long long)j * PGL_ACF_PIECE < n; ++j) {
                acc = pgl_acf_add(acc, spt[j * (PGL_ACF_MAX_LAG + 1) + tid]);
                cnt += scn[j * (PGL_ACF_MAX_LAG + 1) + tid];
            }
    }
    if (tid <= L) {
        sacc[tid] = acc;
        scnt[tid] = cnt;
    }
    __syncthreads();
    if (tid == 0) pgl_acf_finish(n, mean, sacc, scnt, L, bad, p.out + (size_t)blockIdx.x * (PGL_ACF_NHEAD + L));
}
