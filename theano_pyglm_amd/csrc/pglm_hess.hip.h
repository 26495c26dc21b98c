// Dense per-neuron Hessians of the log likelihood: the weighted Gram contraction k_hess and the reduction of its partials.
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
//
// Reference: hessian_wrt_list (pyglm/utils/grads.py:30-66), the default of the parallel driver
// (parallel_coord_descent.py:62 use_hessian=True).  With the curvature c[t, n] of pgl_hvp_prepare_* (pglm_hvp.hip.h):
//   H_n = sum_t c[t, n] f_t f_t^T,   f_t = [1, fstim[t,:], Weff[n',n] fS[t,n',b]]
// The feature row without Weff, phi_t = [fS[t,n',b] | fstim[t,:] | 1] (the kernel's own column order), is shared by every
// post-synaptic neuron:  G_n = Phi^T . diag(c_n) . Phi  on v_mfma_f64_16x16x4_f64, A = a block of Phi^T (16 columns x 4 bins),
// B = c o Phi (4 bins x 16 columns), and Weff enters in the reduction, on both sides.
//
// Blocking: the columns are cut into blocks of 64.  A workgroup (8 waves) owns one block pair (I, J <= I), eight prepared
// rows (one per wave: c differs by row, Phi does not) and one chunk of 16-bin time tiles.  Per tile the 512 threads build the
// two 16 x 64 blocks of Phi in LDS from the event lists (gen_items, as k_fused2; dense stimulus columns and the constant
// column are copied in), then every wave runs 4 k-steps x (4 A fragments, 4 B fragments, 16 MFMAs) into its 4 x 4 output
// tiles (128 accumulator registers); on the diagonal pair (I == J) only the 10 tiles on and below the diagonal.
// The chunk partials leave in the accumulator layout; k_hess_reduce sums them in chunk order (deterministic), applies Weff,
// permutes to the theta layout and stores every element j <= i to H[i][j] AND H[j][i] from the same register: both triangles
// hold the same bits.
#pragma once

struct HessParams {
    long long nT, t_hi;
    int N, B, R, RP, Dstim, Kimp, K;     // K = Kimp + Dstim + 1 columns (= P)
    const int2* __restrict__ spk;
    const int* __restrict__ wlo;
    const int* __restrict__ whi;
    const double* __restrict__ fstim;
    const double* __restrict__ phi;
    const double* __restrict__ C;        // curvature of the last prepare (rows layout or accumulator-layout slab, k_hvp_curv)
    int cxs;                             // 16 * post tiles of the prepare: row stride of the rows layout
    int r0, count;                       // prepared rows [r0, r0 + count) of this launch
    int tile0, nTiles, nChunks, tilesPerChunk;
    int nPairs, nGroups;
    double* __restrict__ part;           // [chunk][row][pair][4 x 4 tiles][4][64]
};

constexpr int PGL_HESS_CB = 64;          // columns per block
constexpr int PGL_HESS_LD = 144;         // LDS row stride of the two blocks (16 mod 32 doubles: the four bins of an MFMA
                                         // fragment read fall into different bank halves)
constexpr int PGL_HESS_NPB = 66;         // presynaptic neurons a block of 64 impulse columns can touch (B = 1: 64)

__device__ __forceinline__ void pgl_hess_pair(const int pair, int& I, int& J)
{
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= pair) ++i;
    I = i;
    J = pair - i * (i + 1) / 2;
}

template <int SLAB>
__global__ __launch_bounds__(512, 2) void k_hess(const HessParams p)
{
    constexpr int TT = 16, CB = PGL_HESS_CB, LD = PGL_HESS_LD, NPB = PGL_HESS_NPB, CAP = PGL_CAP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int nthr = 512;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, grp = lane >> 4;

    const int pair = (int)blockIdx.x % p.nPairs;
    const int g = ((int)blockIdx.x / p.nPairs) % p.nGroups;
    const int chunk = (int)blockIdx.x / (p.nPairs * p.nGroups);
    int I, J;
    pgl_hess_pair(pair, I, J);
    const bool diag = I == J;
    const int row = g * 8 + wave;                 // prepared row of this wave (relative to r0)
    const bool active = row < p.count;

    const int B = p.B, RP = p.RP, N = p.N, R = p.R;
    double* Fs = reinterpret_cast<double*>(smem);
    size_t off = (size_t)TT * LD * 8;
    double* phiE = reinterpret_cast<double*>(smem + off);
    double* phiO = phiE + (size_t)B * RP;
    off += (((size_t)2 * B * RP * 8) + 15) & ~(size_t)15;
    int2* s_dec = reinterpret_cast<int2*>(smem + off);         // [2][NPB][CAP]
    off += (size_t)2 * NPB * CAP * 8;
    int* s_lo = reinterpret_cast<int*>(smem + off);            // [2][NPB]
    off += (size_t)2 * NPB * 4;
    int* s_cnt = reinterpret_cast<int*>(smem + off);           // [2][NPB]

    for (int i = tid; i < B * RP; i += nthr) {
        const int b = i / RP, k = i - b * RP;
        phiE[i] = (k >= 16 && k < 16 + R) ? p.phi[b * R + k - 16] : 0.0;
        phiO[i] = (k + 1 >= 16 && k + 1 < 16 + R) ? p.phi[b * R + k + 1 - 16] : 0.0;
    }

    // the two column blocks of this workgroup: region 0 = block I (A operand), region 1 = block J (B operand; I itself on
    // the diagonal pair) -- first column, presynaptic neurons with impulse columns inside
    const int nreg = diag ? 1 : 2;
    int c0[2], npLo[2], nnp[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        c0[q] = CB * (q == 0 ? I : J);
        npLo[q] = c0[q] / B;
        const int last = (c0[q] + CB - 1 < p.Kimp) ? c0[q] + CB - 1 : p.Kimp - 1;
        nnp[q] = (c0[q] < p.Kimp) ? last / B - npLo[q] + 1 : 0;
    }

    d4_t acc[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = (d4_t){0.0, 0.0, 0.0, 0.0};

    const int tile_beg = p.tile0 + chunk * p.tilesPerChunk;
    int tile_end = tile_beg + p.tilesPerChunk;
    if (tile_end > p.tile0 + p.nTiles) tile_end = p.tile0 + p.nTiles;
    const int nrow = p.r0 + row;                  // row of the prepare
    const int joff = diag ? 0 : CB;

    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int t0 = tile * TT;
        // c of this wave's row: bin 4 s + grp of the tile rides in k-step s, lane group grp (requested here, used behind
        // three barriers).  Bins outside [.., t_hi) and padding rows hold c = 0 (k_hvp_curv); the rows layout ends at nT.
        double cs[4] = {0.0, 0.0, 0.0, 0.0};
        if (active) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long long t = (long long)t0 + 4 * s + grp;
                if (t < p.t_hi) {
                    if (SLAB)
                        cs[s] = p.C[((size_t)(tile - p.tile0) * (p.cxs >> 4) + (nrow >> 4)) * 256 + s * 64 + grp * 16 + (nrow & 15)];
                    else
                        cs[s] = p.C[(size_t)t * p.cxs + nrow];
                }
            }
        }
        __syncthreads();                           // every wave is done with the previous tile's blocks
        // ---- event windows of the blocks' presynaptic neurons, decoded for this tile ----
        for (int q = 0; q < nreg; ++q) {
            for (int id = tid; id < nnp[q] * CAP; id += nthr) {
                const int np = id / CAP, sl = id % CAP;
                const size_t wi = (size_t)tile * N + npLo[q] + np;
                const int lo = p.wlo[wi];
                const int cnt = p.whi[wi] - lo;
                if (sl == 0) {
                    s_lo[q * NPB + np] = lo;
                    s_cnt[q * NPB + np] = cnt;
                }
                if (cnt <= CAP && sl < cnt)
                    s_dec[(q * NPB + np) * CAP + ((lo + sl) & (CAP - 1))] = pgl_decode_event<8>(p.spk[lo + sl], t0, B * RP * 8);
            }
            // ---- dense stimulus columns, the constant column, zero padding ----
            if (c0[q] + CB > p.Kimp) {
                for (int id = tid; id < TT * CB; id += nthr) {
                    const int r = id / CB, c = id % CB;
                    const int gc = c0[q] + c;
                    if (gc >= p.Kimp) {
                        const long long tg = (long long)t0 + r;
                        double v = 0.0;
                        if (gc < p.Kimp + p.Dstim)
                            v = (tg < p.nT) ? p.fstim[tg * p.Dstim + (gc - p.Kimp)] : 0.0;
                        else if (gc == p.Kimp + p.Dstim)
                            v = 1.0;
                        Fs[r * LD + q * CB + c] = v;
                    }
                }
            }
        }
        __syncthreads();
        // ---- impulse columns from the staged events ----
        for (int q = 0; q < nreg; ++q) {
            const int kend = (c0[q] + CB < p.Kimp) ? c0[q] + CB : p.Kimp;
            gen_items<0, CAP, double>(Fs + q * CB - c0[q], LD, reinterpret_cast<const unsigned char*>(phiE), RP,
                                      s_dec + (q * NPB - npLo[q]) * CAP, s_lo + q * NPB - npLo[q], s_cnt + q * NPB - npLo[q],
                                      p.spk, t0, B, kend, tid, nthr, 0, 4 * c0[q]);
        }
        __syncthreads();
        // ---- G += Phi_I^T . (c o Phi_J) ----
        // (on the diagonal pair the tiles above the diagonal are skipped: wave-uniform branches around single MFMAs -- two
        // copies of the loop, one per kind of pair, made the compiler spill the accumulators)
        if (active) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double* fr = Fs + (4 * s + grp) * LD + col;
                double a[4], b[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) a[x] = pgl_lds_f64(fr + 16 * x);
#pragma unroll
                for (int y = 0; y < 4; ++y) b[y] = cs[s] * pgl_lds_f64(fr + joff + 16 * y);
#pragma unroll
                for (int x = 0; x < 4; ++x) {
#pragma unroll
                    for (int y = 0; y < 4; ++y) {
                        if (y > x && diag) continue;
                        acc[4 * x + y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[4 * x + y], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (active) {
        double* out = p.part + (((size_t)chunk * p.count + row) * p.nPairs + pair) * 4096 + lane;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[x * 256 + r * 64] = acc[x][r];
        }
    }
}

// H of one (block pair, row): the chunk partials summed in chunk order, Weff on both sides, columns permuted from
// [impulse | stimulus | 1] to the theta layout [bias, stimulus, impulse], both triangles from one value.
__global__ __launch_bounds__(256) void k_hess_reduce(const HessParams p, const double* __restrict__ Weff, const int* __restrict__ pidx,
                                                     int n_lo, double* __restrict__ H, int ld)
{
    const int pair = blockIdx.x, row = blockIdx.y;
    int I, J;
    pgl_hess_pair(pair, I, J);
    const int nrow = p.r0 + row;
    const int nglob = pidx ? pidx[nrow] : n_lo + nrow;
    const size_t cstride = (size_t)p.count * p.nPairs * 4096;
    const double* src = p.part + ((size_t)row * p.nPairs + pair) * 4096;
    double* Hn = H + (size_t)nrow * p.K * ld;
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int x = e >> 10, y = (e >> 8) & 3, r = (e >> 6) & 3, lane = e & 63;
        const int i = PGL_HESS_CB * I + 16 * x + (lane >> 4) + 4 * r;
        const int j = PGL_HESS_CB * J + 16 * y + (lane & 15);
        if (i >= p.K || j > i) continue;           // (the tiles above the diagonal of a diagonal pair are never written)
        double v = 0.0;
        for (int c = 0; c < p.nChunks; ++c) v += src[(size_t)c * cstride + e];
        const double wi = (i < p.Kimp) ? Weff[(size_t)(i / p.B) * p.N + nglob] : 1.0;
        const double wj = (j < p.Kimp) ? Weff[(size_t)(j / p.B) * p.N + nglob] : 1.0;
        const int ti = (i < p.Kimp) ? 1 + p.Dstim + i : (i < p.Kimp + p.Dstim ? 1 + i - p.Kimp : 0);
        const int tj = (j < p.Kimp) ? 1 + p.Dstim + j : (j < p.Kimp + p.Dstim ? 1 + j - p.Kimp : 0);
        v = v * wi * wj;
        Hn[(size_t)ti * ld + tj] = v;
        Hn[(size_t)tj * ld + ti] = v;
    }
}
