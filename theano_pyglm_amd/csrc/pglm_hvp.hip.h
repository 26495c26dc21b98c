// Hessian-vector products of the log likelihood: the curvature pass, the row kernels of the general apply and the fused
// apply on resident feature tiles (k_hvp5).
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
//
// Reference: hessian_rop_wrt_list (pyglm/utils/grads.py:68-95) builds H.v with T.Rop.  With x_t = f_t . theta_n:
//   H_n . v = sum_t c_t f_t (f_t . v),   c_t = -dt lam''(x_t) + S[t,n] (log lam)''(x_t)
// c depends on theta only: pgl_hvp_prepare_* computes it once and keeps it on the device (same footprint and layout as the
// residual slab), pgl_hvp_apply_dev is forward contraction | one multiply per element | backward contraction.
#pragma once

// ---------------------------------------------------------------------------
// c(x, s), all f64 (pgl_exp / pgl_log / pgl_rcp).
//   exp:        c = -dt e^x, x clamped at 709 (the largest x with a finite e^x): c is always finite, a zero u = f . v
//               never meets an infinite weight; x -> -inf gives c = -0 (x clamped at -800 as well: pgl_exp(-inf) is NaN,
//               k ln2 - inf in its range reduction).
//   explinear:  lam = log(1 + e^x), sig = 1 / (1 + e^-x), with e = e^-|x| and inv = 1 / (1 + e):
//               lam'' = sig (1 - sig) = e inv^2 (both signs of x),
//               (log lam)'' = sig (1 - sig) / lam - sig^2 / lam^2 = sig / lam^2 . ((1 - sig) lam - sig)
//                 x >= 0:  inv^2 (e lam - 1) / lam^2                                    (no cancellation: e lam << 1)
//                 x <  0:  e inv^2 (lam - e) / lam^2, and for e < 1e-2 by the series of log1p (lam - e cancels and lam -> 0):
//                          lam = e l(e), lam - e = -e^2 q(e) / 2  =>  -(e / 2) inv^2 q(e) / l(e)^2
//               Limits (|x| clamped at 800 inside the exponential, see above): x -> +inf (x clamped at DBL_MAX): c = 0;
//               x -> -inf: e = 0, c = 0 (the reference's 0/0 at lam == 0 is NOT reproduced: the limit of (log lam)'' is
//               -e^x / 2 -> 0);  x = NaN: c = NaN.
// ---------------------------------------------------------------------------
template <typename CP>
__device__ __forceinline__ double pgl_curvature(const double x, const double s, const int nlin, const double dt, const CP C)
{
    double c;
    if (nlin == 1) {
        const double xc = fmin(x, 1.7976931348623157e308);
        const double e = pgl_exp(-fmin(fabs(x), 800.0), C);     // (e^-800 = 0; pgl_exp's range reduction makes inf - inf beyond)
        const double u = 1.0 + e;
        const double inv = pgl_rcp(u);
        const double i2 = inv * inv;
        c = -dt * e * i2;
        if (s > 0.0) {
            double h;
            if (xc >= 0.0) {
                const double lam = xc + (pgl_log(u, C) + (e - (u - 1.0)) * inv);
                const double rl = pgl_rcp(lam);
                h = i2 * fma(e, lam, -1.0) * rl * rl;
            } else if (e < 1.0e-2) {
                double l = 0.1, q = 2.0 / 11.0;            // l = log1p(e) / e, q = -2 (log1p(e) - e) / e^2, degree 9
#pragma unroll
                for (int k = 8; k >= 0; --k) {
                    l = fma(-e, l, 1.0 / (k + 1));
                    q = fma(-e, q, 2.0 / (k + 2));
                }
                const double rl = pgl_rcp(l);
                h = -0.5 * e * i2 * q * rl * rl;
            } else {
                const double lam = pgl_log(u, C) + (e - (u - 1.0)) * inv;
                const double rl = pgl_rcp(lam);
                h = e * i2 * (lam - e) * rl * rl;
            }
            c = fma(s, h, c);
        }
    } else {
        c = -dt * pgl_exp(fmax(fmin(x, 709.0), -800.0), C);
    }
    return (x != x) ? x : c;
}

// x -> c in place.  slab = 0: rows layout of the 3-phase path, element i = (t - row0) * xs + n.  slab = 1: the accumulator
// layout of the two-pass kernels' slab, element i = ((tile - tile0) * nPT + pt) * 256 + r * 64 + lane with
// t = 16 tile + (lane >> 4) + 4 r, n = 16 pt + (lane & 15).  X holds the currents without the bias.  Elements of padding
// neurons (n >= npost) and of bins outside [.., t_hi) get c = 0, so the apply needs no range test of its own.
__global__ __launch_bounds__(256) void k_hvp_curv(double* __restrict__ X, const double* __restrict__ bias,
                                                  const uint8_t* __restrict__ S, int Nall, int n_lo, int npost,
                                                  const int* __restrict__ pidx, int xs, long long row0, long long t_hi,
                                                  long long total, int slab, int nlin, double dt)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long t;
        int n;
        if (slab) {
            const int lane = (int)(i & 63), r = (int)((i >> 6) & 3);
            const long long blk = i >> 8;
            const int nPT = xs >> 4;
            n = 16 * (int)(blk % nPT) + (lane & 15);
            t = row0 + 16 * (blk / nPT) + (lane >> 4) + 4 * r;
        } else {
            n = (int)(i % xs);
            t = row0 + i / xs;
        }
        double c = 0.0;
        if (n < npost && t < t_hi) {
            const double s = (double)S[t * Nall + (pidx ? pidx[n] : n_lo + n)];
            c = pgl_curvature(X[i] + bias[n], s, nlin, dt, PGL_C);
        }
        X[i] = c;
    }
}

// General apply, phase 2 (rows layout): r = c * (u + v_bias) in place of u; per-block sums of r (the bias component of
// H.v) for k_rows_reduce.  Grid as k_rows_epilogue.
__global__ __launch_bounds__(256) void k_hvp_rows_mul(double* __restrict__ Xbuf, const double* __restrict__ Cbuf, int xstride,
                                                      const double* __restrict__ bias, int npost, long long t_lo,
                                                      long long t_hi, int rows, double* __restrict__ llp,
                                                      double* __restrict__ gbp)
{
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= npost) return;
    const long long t0 = t_lo + (long long)blockIdx.x * rows;
    long long t1 = t0 + rows;
    if (t1 > t_hi) t1 = t_hi;
    const double b = bias[n];
    double gb = 0.0;
    for (long long t = t0; t < t1; ++t) {
        const double r = Cbuf[t * xstride + n] * (Xbuf[t * xstride + n] + b);
        gb += r;
        Xbuf[t * xstride + n] = r;
    }
    llp[(size_t)blockIdx.x * npost + n] = 0.0;
    gbp[(size_t)blockIdx.x * npost + n] = gb;
}

// ---------------------------------------------------------------------------
// Fused apply on resident feature tiles: pass 1 of the two-pass scheme of k_fused5 (same images, same Wmat fragment
// stream, same L / H column split, one wave per post tile) with the rate epilogue replaced by one multiply:
//   per tile: [L_i | H_i in LDS] forward u = F . v over both parts | barrier | r = c * (u + v_bias), c read from the
//             curvature slab in the accumulator layout | r to the residual slab | backward for the L columns from L_i,
//             the DMA of L_{i+1} (third buffer) and H_{i+1} (over H_i) issued between its MFMAs | wait | barrier.
// Pass 2 (the H columns from the residual slab) is k_fused5<KTL, KTH, 2> itself; k_finalize reduces the partials.
// No spike counts, no transcendental, no helper waves.  FWO = 1: forward only, the raw currents go to p.Xbuf (the
// curvature pass of pgl_hvp_prepare_* on this shape class).
// ---------------------------------------------------------------------------
template <int KTL, int KTH, int FWO>
__global__ __launch_bounds__(512, 2) void k_hvp5(const FusedParams p, const double* __restrict__ cslab_g)
{
    constexpr int TT = 16, NW = 8;
    constexpr int KT_ALL = KTL + KTH;
    constexpr int KS_ALL = 4 * KT_ALL;
    constexpr int KSL = 4 * KTL;
    constexpr int RSL = pgl_img_rsh(KTL), RSH = pgl_img_rsh(KTH);
    constexpr int IMGL = pgl_img_bytes(KTL), IMGH = pgl_img_bytes(KTH);
    constexpr size_t IMGS = (size_t)IMGL + IMGH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nPB = (p.nPT + NW - 1) / NW;
    const int pb = (int)blockIdx.x % nPB;
    const int chunk = (int)blockIdx.x / nPB;
    const int pt = pb * NW + wave;
    const bool active = pt < p.nPT;

    unsigned char* buf0 = smem;                  // L buffers at 0 and IMGL, the H buffer behind them
    unsigned char* buf2 = smem + IMGL;
    unsigned char* buf1 = smem + 2 * IMGL;

    const int col = lane & 15;
    const int grp = lane >> 4;
    const int nloc = pt * 16 + col;
    const bool valid_n = active && (nloc < p.npost);

    const int tile_beg = p.tile0 + chunk * p.tilesPerChunk;
    int tile_end = tile_beg + p.tilesPerChunk;
    if (tile_end > p.tile0 + p.nTiles) tile_end = p.tile0 + p.nTiles;
    const size_t soff = ((size_t)(active ? pt : 0)) * 256 + lane;
    double* const rslab = p.Xbuf + soff;
    const double* const cslab = cslab_g + soff;
    const size_t rstride = (size_t)p.nPT * 256;
    const unsigned char* __restrict__ fimg = p.Fimg - (size_t)p.img_tile0 * IMGS;

    // backward over the L image; the DMA rounds of the next tile's L (NRL rounds) and H (NRH rounds) images go out
    // between the MFMAs (as k_fused5's bwd_part in pass 1)
    constexpr int NRL = (IMGL / 1024 + 7) / 8, NRH = (IMGH / 1024 + 7) / 8;
    auto bwd_l = [&](d4_t (&G)[KTL], const unsigned char* Fb, const double (&rq)[4], const unsigned char* g0,
                     unsigned char* l0, const unsigned char* g1, unsigned char* l1, const bool dma) {
        const double* fb = reinterpret_cast<const double*>(Fb) + pgl_img_brow(grp) * RSL + col;
        constexpr int NK = KTL, NS = 4 * NK;
        constexpr int PD = (NS < PGL_PD) ? NS : PGL_PD;
        constexpr int NRT = NRL + NRH;
        constexpr int DSFULL = NS / NRT;
        constexpr int DSCAP = (PGL_DS1 > 0) ? PGL_DS1 : NS;
        constexpr int DSTEP = (NS >= 2 * NRT) ? ((DSFULL < DSCAP) ? DSFULL : DSCAP) : 0;   // MFMAs between rounds
        double ar[PD];
#pragma unroll
        for (int s = 0; s < PD; ++s) ar[s] = pgl_lds_f64(fb + (2 * (s / NK)) * RSL + 16 * (s % NK));
        auto round = [&](const int j) {
            if (j < NRL) pgl_dma_round<KTL>(g0, l0, j, wave, lane);
            else pgl_dma_round<KTH>(g1, l1, j - NRL, wave, lane);
        };
        if (DSTEP == 0 && dma) {
#pragma unroll
            for (int j = 0; j < NRT; ++j) round(j);
        }
        const int phase = (wave < 4) ? ((DSTEP > 1) ? DSTEP / 2 - 1 : 0) : DSTEP - 1;
        if (PGL_PRIO && wave >= 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (PGL_PRIO && s == NS / 2 && wave >= 4) __builtin_amdgcn_s_setprio(0);
            const double a = ar[s % PD];
            if (s + PD < NS) ar[s % PD] = pgl_lds_f64(fb + (2 * ((s + PD) / NK)) * RSL + 16 * ((s + PD) % NK));
            G[s % NK] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rq[s / NK], G[s % NK], 0, 0, 0);
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            if (DSTEP > 0) {
                constexpr int DS = (DSTEP > 0) ? DSTEP : 1;
                const int j = s / DS;
                const int ph = s % DS;
                if ((ph == DS - 1 || (DS > 1 && ph == DS / 2 - 1)) && j < NRT) {
                    if (ph == phase && dma) round(j);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };

    d4_t G[KTL];
#pragma unroll
    for (int kt = 0; kt < KTL; ++kt) G[kt] = (d4_t){0.0, 0.0, 0.0, 0.0};
    double gb_acc = 0.0;
    const double bias_l = valid_n ? p.bias[nloc] : 0.0;
    const double* __restrict__ wrow = p.Wfrag + (size_t)(active ? pt : 0) * KS_ALL * 64;
    if (tile_beg < tile_end) {
        pgl_dma_half<KTL>(fimg + (size_t)tile_beg * IMGS, buf0, wave, lane);
        pgl_dma_half<KTH>(fimg + (size_t)tile_beg * IMGS + IMGL, buf1, wave, lane);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);              // vmcnt(0): the DMAs have landed
    __syncthreads();
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int par = (tile - tile_beg) & 1;
        const unsigned char* Lb = par ? buf2 : buf0;     // L alternates buf0 / buf2, H lives in buf1
        unsigned char* Ln = par ? buf0 : buf2;
        const bool more = tile + 1 < tile_end;
        // ---- forward over both parts ----
        d4_t acc0 = (d4_t){0.0, 0.0, 0.0, 0.0};
        d4_t acc1 = (d4_t){0.0, 0.0, 0.0, 0.0};
        if (active) {
            constexpr int PW2 = (KS_ALL / 2 < PGL_PW / 2) ? KS_ALL / 2 : PGL_PW / 2;
            const double* faL = reinterpret_cast<const double*>(Lb) + pgl_img_row(col) * RSL + grp;
            const double* faH = reinterpret_cast<const double*>(buf1) + pgl_img_row(col) * RSH + grp;
            const double* wr_s = wrow;
            asm volatile("" : "+s"(wr_s));
            constexpr int PA = 4;
            pgl_d2 wr[PW2];
            double ar[PA];
            auto afrag = [&](const int s) -> double {
                return (s < KSL) ? pgl_lds_f64(faL + 4 * s) : pgl_lds_f64(faH + 4 * (s - KSL));
            };
            // scalar bases of the Wmat fragment stream, one per 4 KB (four pairs of k-steps)
            pgl_glb_cd2p wr_base[KS_ALL / 8 + 1];
#pragma unroll
            for (int b4 = 0; b4 < (KS_ALL + 7) / 8; ++b4) {
                const double* bs = wr_s + (size_t)b4 * 512;
                asm volatile("" : "+s"(bs));
                wr_base[b4] = (pgl_glb_cd2p)bs;
            }
#pragma unroll
            for (int q = 0; q < PW2; ++q) wr[q] = wr_base[q / 4][(q % 4) * 64 + lane];
#pragma unroll
            for (int q = 0; q < PA; ++q) ar[q] = afrag(q);
            if (PGL_PRIO && wave >= 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int q = 0; q < KS_ALL; ++q) {
                if (PGL_PRIO && q == KS_ALL / 2 && wave >= 4) __builtin_amdgcn_s_setprio(0);
                const double a = ar[q % PA];
                const double b = (q & 1) ? wr[(q / 2) % PW2].y : wr[(q / 2) % PW2].x;
                if (q + PA < KS_ALL) ar[q % PA] = afrag(q + PA);
                if ((q & 1) && (q / 2 + PW2 < KS_ALL / 2)) {
                    const int pair = q / 2 + PW2;      // compile-time (unrolled)
                    wr[(q / 2) % PW2] = wr_base[pair / 4][(pair % 4) * 64 + lane];
                }
                if (q & 1)
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc1, 0, 0, 0);
                else
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc0, 0, 0, 0);
                if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        const size_t so = (size_t)(tile - p.tile0) * rstride;
        double cv[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (!FWO) {                         // requested in front of the barrier: its wait hides the latency
            if (active) {
#pragma unroll
                for (int r = 0; r < 4; ++r) cv[r] = cslab[so + r * 64];
            }
        }
        // every wave is done with H_i (buf1): the next tile's DMA may overwrite it
        __syncthreads();
        if constexpr (FWO) {
            if (active) {
#pragma unroll
                for (int r = 0; r < 4; ++r) rslab[so + r * 64] = acc0[r] + acc1[r];
            }
            if (more) {
                pgl_dma_half<KTL>(fimg + (size_t)(tile + 1) * IMGS, Ln, wave, lane);
                pgl_dma_half<KTH>(fimg + (size_t)(tile + 1) * IMGS + IMGL, buf1, wave, lane);
            }
        } else if (active) {
            // c = 0 for padding neurons and for bins outside the evaluated range (k_hvp_curv)
            double rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rr[r] = cv[r] * (bias_l + (acc0[r] + acc1[r]));
                gb_acc += rr[r];
                rslab[so + r * 64] = rr[r];
            }
            bwd_l(G, Lb, rr, fimg + (size_t)(tile + 1) * IMGS, Ln, fimg + (size_t)(tile + 1) * IMGS + IMGL, buf1, more);
        } else if (more) {
            pgl_dma_half<KTL>(fimg + (size_t)(tile + 1) * IMGS, Ln, wave, lane);
            pgl_dma_half<KTH>(fimg + (size_t)(tile + 1) * IMGS + IMGL, buf1, wave, lane);
        }
        __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0): L_{i+1}, H_{i+1} landed, r stored
        __syncthreads();
    }
    if constexpr (!FWO) {
        if (active) {
            pgl_store_ll(p, chunk, pt, 0, 1, lane, 0.0, gb_acc);
            double* gp = pgl_gpart(p.Gpart, pt, KT_ALL, 0, p.nChunks, chunk, lane);
            const size_t gcs = (size_t)p.nChunks * 64;
#pragma unroll
            for (int kt = 0; kt < KTL; ++kt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(kt * 4 + r) * gcs] = G[kt][r];
            }
        }
    }
}
