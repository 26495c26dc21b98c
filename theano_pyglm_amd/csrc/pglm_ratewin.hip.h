// Expected and observed spike counts over user-chosen time windows, and their fold over posterior draws: for every neuron
//     Lam[w][n] = dt * sum_{t in window w} lam_t,   lam_t = nlin(bias_n + GX[t][n]),      obs[w][n] = sum_{t in window w} S[t,n],
// from the bias-free total currents the forward-only pass leaves in GX and the per-neuron event lists -- the firing-rate
// counterpart of pglm_pointwise.hip.h.  Windows are win >= 1 consecutive bins counted from t_lo (the last one may be short) and
// have nothing to do with the 256-bin chunk grid of the rescaling kernels; the order of every sum is the one pglm_ratewin.h
// fixes (pieces of at most PGL_RW_PIECE = 256 bins counted from the window's own first bin, each summed in time order, added
// in piece order), so the bits of a window do not depend on how the work is cut.  ONE read of GX, no (nT, N) array, two launches:
//   k_rw_piece    units x columns of GX, a thread per (unit, neuron) on the walk of pglm_binwalk.hip.h.  win > 256: a unit is
//                 one piece of a window, so a long window is spread over ceil(win / 256) threads per neuron.  win <= 256: a
//                 window is one piece and a unit is floor(256 / win) consecutive windows, so a thread still owns about 256
//                 bins; it restarts its sums at every window start.  Per piece: the sum of the rate and the sum of the spike
//                 counts -> part, cnt;
//   k_rw_window   one thread per (window, neuron): the window's piece sums added in piece order -> Lam, obs, and, with an
//                 accumulator, the fold of pglm_ratewin.h (Welford mean and M2, min, max, running mean of the Poisson mid-p
//                 value of the observed count).  With win >= the range this launch has N threads and reads nT / 256 doubles each.
// Nothing is atomic and every sum has a fixed order: the results are bit-reproducible from run to run.
//
// The rate function is pgl_lambda_only's arithmetic (all f64) with ONE difference: that function picks the series of log1p by
// a vote of the wave (__all), so the last bit of a lane's rate can depend on the currents of the 63 other lanes -- other
// neurons and other windows.  Here every lane picks the series its own argument allows (pgl_rw_lambda), which is what makes a
// window's bits independent of its neighbours; each series is used inside the range it was derived for, as there.
#pragma once

#include "pglm_ratewin.h"

struct RateWinParams {
    BinSource src;            // currents, biases, event lists, time range (pglm_binwalk.hip.h)
    double* part;             // (npieces, xs) piece sums of the rate
    int* cnt;                 // (npieces, xs) piece sums of the spike counts
    double* lam;              // (n_win, N) expected counts, or null
    double* obs;              // (n_win, N) observed counts, or null
    double* acc;              // (PGL_RW_NACC, n_win, N) accumulator over draws, or null
    long long win, draw;
    long long n_win, npieces, nunits;
    int ppw;                  // pieces of a whole window: ceil(win / 256)
    int group;                // pieces (= windows) per unit where ppw = 1, else 1
};

__device__ __forceinline__ double pgl_rw_lambda(const double x, const int nlin, const double* __restrict__ C)
{
    if (nlin != 1) return pgl_exp(x, C);
    const double e = pgl_exp(-fabs(x), C);
    double l1p;
    if (e < C[23]) {                               // |x| > 9.25: alternating series, error < e^6
        l1p = e * fma(-e, fma(-e, fma(-e, fma(-e, 0.2, 0.25), C[22]), 0.5), 1.0);
    } else if (e < 0.1) {                          // |x| > 2.3: log1p(e) = 2 atanh(s), s = e/(2+e) < 0.048
        const double rc = pgl_rcp(2.0 + e);
        const double s = e * rc;
        const double z = s * s;
        const double q = fma(z, fma(z, fma(z, fma(z, fma(z, fma(z, 1.0 / 13.0, 1.0 / 11.0), 1.0 / 9.0), 1.0 / 7.0),
                                           0.2), C[22]), 1.0);
        l1p = e * ((rc + rc) * q);
    } else {                                       // (a NaN argument comes here and stays NaN)
        const double u = 1.0 + e;
        l1p = pgl_log(u, C) + (e - (u - 1.0)) * pgl_rcp(u);
    }
    return fmax(x, 0.0) + l1p;
}

template <int NLIN>
__global__ __launch_bounds__(256) void k_rw_piece(const RateWinParams p)
{
    const BinSource& s = p.src;
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % s.xs);
    const long long u = g / s.xs;
    if (u >= p.nunits || j >= s.N) return;
    const long long q0 = u * p.group;                            // the unit's first piece
    long long t0;
    int span, step;                                              // bins of the unit, bins of each of its pieces
    if (p.ppw == 1) {
        t0 = s.t_lo + q0 * p.win;
        const long long room = s.t_hi - t0, all = (long long)p.group * p.win;
        span = (int)((room < all) ? room : all);
        step = (int)p.win;
    } else {
        const long long w0 = s.t_lo + (q0 / p.ppw) * p.win;      // the window's first bin
        t0 = w0 + (q0 % p.ppw) * PGL_RW_PIECE;
        const long long wend = (w0 + p.win < s.t_hi) ? w0 + p.win : s.t_hi;
        span = (int)((wend - t0 < PGL_RW_PIECE) ? wend - t0 : PGL_RW_PIECE);
        step = span;
    }
    size_t o = (size_t)q0 * s.xs + j;
    double acc = 0.0;
    int cnt = 0, left = step;
    pgl_bin_walk(
        s, j, t0, span, [](const double xv) { return pgl_rw_lambda(xv, NLIN, PGL_C); },
        [&](const int k, const bool live, double, const double lam, bool, const int count, int) {
            if (!live) return;
            acc += lam;
            cnt += count;
            if (--left == 0 || k + 1 == span) {                  // the piece ends here
                p.part[o] = acc;
                p.cnt[o] = cnt;
                o += s.xs;
                acc = 0.0;
                cnt = 0;
                left = step;
            }
        });
}

__global__ __launch_bounds__(256) void k_rw_window(const RateWinParams p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % p.src.xs);
    const long long w = g / p.src.xs;
    if (w >= p.n_win || j >= p.src.N) return;
    const long long q0 = w * p.ppw;
    const long long q1 = (q0 + p.ppw < p.npieces) ? q0 + p.ppw : p.npieces;
    double s = 0.0;
    int c = 0;
    for (long long q = q0; q < q1; ++q) {
        s += p.part[(size_t)q * p.src.xs + j];
        c += p.cnt[(size_t)q * p.src.xs + j];
    }
    const double lam = p.src.dt * s, y = (double)c;
    const size_t o = (size_t)w * p.src.N + j;
    if (p.lam) p.lam[o] = lam;
    if (p.obs) p.obs[o] = y;
    if (p.acc) {
        const size_t pl = (size_t)p.n_win * p.src.N;
        double mean = p.acc[o], m2 = p.acc[pl + o], mn = p.acc[2 * pl + o], mx = p.acc[3 * pl + o], pit = p.acc[4 * pl + o];
        pgl_rw_fold(lam, y, p.draw, &mean, &m2, &mn, &mx, &pit);
        p.acc[o] = mean; p.acc[pl + o] = m2; p.acc[2 * pl + o] = mn; p.acc[3 * pl + o] = mx; p.acc[4 * pl + o] = pit;
    }
}
