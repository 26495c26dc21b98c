// Launch plans of the fused kernels (host side; included by pglm_capi.hip after the context struct): column slices, the
// k-tile lists, make_plan, and the choice of path of an evaluation (select_plans) / of a Hessian-vector product (hvp_select).
// The lists below are the ONE statement of which tile counts exist: make_plan picks from them, the dispatchers of
// pglm_launch.h instantiate the kernels over them.
#pragma once

struct Plan {
    int npost, nPT, wpb, nPB, KT, KS, rsf, RP, nTiles, nChunks, tilesPerChunk, blocks, threads;
    int tile0;
    int version, PTW, KTW, KSPLIT, cap; // version 2/3: K split over KSPLIT waves per post tile
    int ktl, kth;                       // version 5: k-tiles of the L / H column parts
    int hlp = 0;                        // version 5: 1 = idle waves of a 5- or 6-tile block help (k_fused5<.., HLP = 1>)
    int pb_major = 0;                   // version 5, wide: post-block-major grid of one chunk per CU and post block
    int mt;                             // version 6: 16-bin tiles per step
    int nw6;                            // version 6: waves per workgroup (8, or 4 with two workgroups per CU)
    int sb6 = 0;                        // version 6: 1 = one image buffer per workgroup (k_fused6 DB = 0), 2 = per-wave block
                                        // rings on block-form images (k_fused8)
    int img32 = 0;                      // ... whose blocks are stored as f32 (PGL_OPT_FEATURE_F32 = 2)
    int nw7, wg7;                       // version 7: waves per workgroup (1, 2, 4), workgroups per CU
    size_t lds7x = 0;                   // version 7: extra LDS of the separable-stimulus forms
    size_t lds;
    bool f32;
};

// A launch covers a slice of the feature columns: presynaptic neurons [np0, np0+Ns) and dense
// stimulus columns [ds0, ds0+Ds).  One slice = everything when N <= 128 and N*B + Dstim <= 640
// (the fused path); otherwise the 3-phase path runs forward / backward launches per slice.
struct Slice {
    int np0, Ns, ds0, Ds;
};

static std::vector<Slice> make_slices(const pgl_context* h, bool balanced = false)
{
    std::vector<Slice> out;
    int maxNs = std::min(128, (h->opt_slice_cols > 0 ? h->opt_slice_cols : 640) / h->B);
    // balanced: slices of equal width (N = 160: 80 + 80, not 128 + 32) -- every slice then has a long enough feature row for
    // the two-pass kernel on resident tiles (the wide-population path).  The K-split kernel of the other sliced paths pads
    // its rows to 5 / 10 / 20 / 40 k-tiles and is better off with full 640-column slices and a short last one.
    if (balanced && h->N > maxNs) maxNs = (h->N + (h->N + maxNs - 1) / maxNs - 1) / ((h->N + maxNs - 1) / maxNs);
    int ds_left = h->sep ? 0 : h->Dstim, ds0 = 0;      // a separable stimulus is not a set of feature columns
    for (int np0 = 0; np0 < h->N; np0 += maxNs) {
        Slice sl{np0, std::min(maxNs, h->N - np0), 0, 0};
        if (np0 + sl.Ns >= h->N && ds_left > 0 && sl.Ns * h->B + ds_left <= 640) {
            sl.ds0 = ds0; sl.Ds = ds_left; ds0 += ds_left; ds_left = 0;     // stimulus rides along
        }
        out.push_back(sl);
    }
    while (ds_left > 0) {
        const int d = std::min(640, ds_left);
        out.push_back(Slice{0, 0, ds0, d});
        ds0 += d; ds_left -= d;
    }
    return out;
}

// A compile-time list of ints: `values` for the planner's loops, the pack for the dispatchers (dispatch, pglm_launch.h).
template <int... Vs>
struct IntList {
    static constexpr int values[sizeof...(Vs)] = {Vs...};
};
using KTilesSplit = IntList<1, 2, 3, 5, 7, 10, 20>;             // k-tiles per wave, K-split kernels (k_fused2 / 6)
using KTilesHalf = IntList<1, 2, 3, 5, 7, 10, 13, 16>;          // k-tiles per half, two-pass kernel (on the fly, k_fused3)
using KTilesRow = IntList<1, 2, 3, 5, 7, 10, 12, 13, 16>;       // k-tiles of the whole row, one wave per post tile (k_fused7)
// resident-tile kernel: (L, H) k-tile pairs; pass 1 (forward + L columns of G) gets the smaller share
#ifndef PGL_SPLIT_L
#define PGL_SPLIT_L 18       // L / H k-tiles of the 40-k-tile (K = 640) split; measured: 18/22 (see docs/NOTEBOOK.md §4.1)
#endif
constexpr int col_pair(int ktl, int kth) { return ktl << 8 | kth; }
constexpr int pair_l(int pr) { return pr >> 8; }
constexpr int pair_h(int pr) { return pr & 255; }
using ColPairs = IntList<col_pair(1, 1), col_pair(2, 2), col_pair(3, 3), col_pair(5, 5), col_pair(7, 7), col_pair(9, 11),
                         col_pair(12, 14), col_pair(14, 18), col_pair(PGL_SPLIT_L, 40 - PGL_SPLIT_L)>;
static bool pick_pair(int need, int& ktl, int& kth)
{
    for (int pr : ColPairs::values)
        if (pair_l(pr) + pair_h(pr) >= need) {
            ktl = pair_l(pr);
            kth = pair_h(pr);
            return true;
        }
    return false;
}
// Which instantiations of the fused kernels the library holds, beyond the lists above: the dispatchers of pglm_launch.h
// instantiate a kernel only where its predicate holds.  Instantiations that no plan of make_plan selects
// (tools/reachable_kernels.py: dry run of the dispatch over a grid of shapes, with and without forcing options) are not built;
// tests/test_capi_symbols.py fails when a reachable instantiation is missing from the library and when one is built that no
// plan reaches, so a change of make_plan shows up here.
constexpr bool fused2_built(int KTW, int KSPLIT) { return KTW * KSPLIT <= 40; }      // rows of up to 640 columns
// the plain two-pass form takes every column pair; the slab-input (XIN), L-part (PART), helper (HLP) forms and with them the
// wide-population path start at 5|5 (make_plan: helpers from ktl >= 5; select_plans: wide rows >= 7 k-tiles, sepf >= 5|5)
constexpr bool fused5_built(int KTL, int XIN, int PART, int HLP) { return (XIN == 0 && PART == 0 && HLP == 0) || KTL >= 5; }
constexpr bool hvp5_built(int KTL) { return KTL >= 3; }          // (hvp_select: the fused product from 3|3 on)
constexpr bool fused6_built(int KTW, int PTW, int MT, int NW)
{
    if (NW == 4) return MT == 1 && ((PTW == 1 && KTW <= 3) || (PTW == 2 && KTW <= 7));
    if (MT == 2) return PTW == 4 && KTW >= 2 && KTW <= 7;
    // (four post tiles, one tile per step: the long-row form, and every row length on recordings of fewer than four tiles)
    return (PTW == 1 && (KTW == 2 || KTW == 3)) || (PTW == 2 && (KTW == 5 || KTW == 7)) || (PTW == 4 && KTW >= 2);
}
// XIO = 0: workgroups of 1, 2, 4 waves; the slab-input forms of a separable stimulus (XIO 1 .. 3) exist for 4 waves only,
// with the stimulus current inside the forward contraction (2) up to 13 k-tiles and its backward too (3) up to 12: beyond,
// the extra k-steps no longer fit the registers (k_fused7<16, 4, 2> spills)
constexpr bool fused7_built(int KT, int NWV, int XIO)
{
    if (XIO == 0) return !((KT == 1 && NWV >= 2) || (KT == 2 && NWV == 4));
    return NWV == 4 && KT <= (XIO == 3 ? 12 : XIO == 2 ? 13 : 16);
}

static size_t img_pair_bytes(int ktl, int kth) { return (size_t)pgl_img_bytes(ktl) + pgl_img_bytes(kth); }
// one-part images (k_fused6 / 7), padded rows or the block form of k_fused8: slot key and bytes per tile
// (blk: 0 padded rows, 1 blocks of 2 KB, 2 the same blocks stored as f32)
static int img_key6(int kt, int blk) { return (blk ? 0x8000 : 0) | (blk == 2 ? 0x4000 : 0) | kt << 8; }
static size_t img_bytes6(int kt, int blk) { return blk ? (size_t)kt * (blk == 2 ? 1024 : 2048) : (size_t)pgl_img_bytes(kt); }
static constexpr int kRing8 = 8;            // k_fused8<5, kRing8>: blocks per wave
static size_t lds_fused8(int slots) { return (size_t)8 * slots * 2048 + (size_t)(8 * 256 + 256 + 32 + 8 * 48) * 8; }

static int fused6_wg_per_cu(const Plan& pl);        // (pglm_launch.h: an occupancy query of the instantiation the plan selects)

static int make_plan(const pgl_context* h, int n_lo, int n_hi, const Slice& sl, Plan& pl,
                     bool single_slice = true, bool force7 = false, bool wide = false)
{
    const bool hlp_ok = (single_slice || wide) && !force7;      // (the slab-input form of a separable stimulus has no helper variant)
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    pl.npost = n_hi - n_lo;
    pl.nPT = (pl.npost + 15) / 16;
    const int ktot_s = sl.Ns * h->B + sl.Ds;
    const int need = std::max(1, (ktot_s + 15) / 16);
    pl.f32 = h->opt_f32 != 0;
    // version 2: f64 features, 8 waves (2 per SIMD), one workgroup per CU
    // version 3: the same kernel with f32 features / basis taps (PGL_OPT_FEATURE_F32)
    // version 1: the 4-wave kernel of the first round (PGL_OPT_KERNEL = 1)
    // version 4: the two-pass kernel (one workgroup = 8 post tiles, no K split; PGL_OPT_KERNEL 0 = auto
    //            for >= 5 post tiles, 3 = force, 2 = force version 2); f64 features, one slice only
    pl.version = pl.f32 ? 3 : 2;
    if (pl.version == 2 && single_slice && need >= 2) {
        if (h->opt_kernel == 3) pl.version = 4;
        // two-pass kernel on resident tiles from 5 post tiles on; from 3 when the feature row is too long for
        // the resident K-split kernel (measured at K = 640: 64 neurons 2.05 ms against 2.33 ms of k_fused2; a 48-neuron
        // list of a lock-step sweep at C3: 2.36 ms on k_fused2)
        // (force7 with a feature row too long for k_fused7 (> 16 k-tiles: its G no longer fits the registers beside the
        // epilogue) -- e.g. a short neuron list of a wide separable-stimulus population: the slab-input form of the two-pass
        // kernel, whatever the number of post tiles)
        else if (h->opt_kernel == 4 || (h->opt_kernel == 0 && (pl.nPT >= 5 || (pl.nPT >= 3 && need > 20))) ||
                 (force7 && need > 16 && (h->opt_kernel == 0 || h->opt_kernel == 7)))
            pl.version = 5;
    }
    // wide: one column slice of a wide population on the resident-tile two-pass kernel (select_plans has checked the
    // row lengths and the memory)
    if (wide) pl.version = 5;
    pl.tile0 = (int)(h->t_lo / 16);
    pl.nTiles = (int)((h->t_hi + 15) / 16) - pl.tile0;
    pl.ktl = pl.kth = 0;
    if (pl.version == 5 && !pick_pair(need, pl.ktl, pl.kth)) pl.version = 4;
    if (pl.version == 5 && !wide && h->opt_kernel == 0 && find_img(h, pl.ktl << 8 | pl.kth, pl.tile0, pl.nTiles) < 0) {
        // resident feature tiles need nTiles * (L + H image bytes) of HBM (3.1 GB at C3); in auto mode
        // fall back to on-the-fly generation (version 4) when the device cannot spare them
        if (!img_room(h, (size_t)pl.nTiles * img_pair_bytes(pl.ktl, pl.kth))) pl.version = 4;
    }
    // the in-kernel-feature two-pass kernel carries at most 16 k-tiles per half in its registers (k_fused3<20, ..> spilled
    // 22 VGPRs): rows of 33-40 k-tiles go to the K-split kernel, which is as fast there (2.20 against 2.16 ms at N = 128)
    if (pl.version == 4 && (need + 1) / 2 > 16) pl.version = 2;
    pl.RP = h->Rk + 32;
    if (pl.version == 3) {
        while (pl.RP % 64 != 8) ++pl.RP;  // f32 table rows one 32-byte span apart (mod 256 B)
    } else {
        // bank spread of the per-basis table rows for ds_read_b128: the row-interleaved items of
        // gen_items want the rows of b = 0..3 four 16-byte slots (64 B) apart
        while (pl.RP % 32 != 8) ++pl.RP;
    }
    pl.cap = PGL_CAP;
    if (pl.version == 5) {
        pl.PTW = 8; pl.KSPLIT = 1; pl.KTW = pl.kth; pl.KT = pl.ktl + pl.kth; pl.wpb = 8;
        pl.nPB = (pl.nPT + 7) / 8;
    } else if (pl.version == 4) {
        const int needh = (need + 1) / 2;
        int kth = 0;
        for (int k : KTilesHalf::values)
            if (k >= needh) {
                kth = k;
                break;
            }
        if (kth == 0) return fail(PGL_ERR_UNSUPPORTED, "slice exceeds 640 feature columns");
        pl.PTW = 8; pl.KSPLIT = 1; pl.KTW = kth; pl.KT = 2 * kth; pl.wpb = 8;
        pl.nPB = (pl.nPT + 7) / 8;
    } else {
        const int nw = 8;
        const int maxptw = 4;
        pl.PTW = (pl.nPT >= 3) ? 4 : pl.nPT;
        pl.PTW = std::min(pl.PTW, maxptw);
        if (h->opt_ptw == 1 || h->opt_ptw == 2 || h->opt_ptw == 4) pl.PTW = std::min(h->opt_ptw, pl.PTW);
        pl.KSPLIT = nw / pl.PTW;
        const int needw = (need + pl.KSPLIT - 1) / pl.KSPLIT;
        pl.KTW = 0;
        for (int k : KTilesSplit::values)
            if (k >= needw) {
                pl.KTW = k;
                break;
            }
        if (pl.KTW == 0 || pl.KTW * pl.KSPLIT > 40)
            return fail(PGL_ERR_UNSUPPORTED,
                        "slice of " + std::to_string(ktot_s) + " feature columns exceeds 640");
        pl.KT = pl.KTW * pl.KSPLIT;
        pl.wpb = nw;
        pl.nPB = (pl.nPT + pl.PTW - 1) / pl.PTW;
        // version 6: the K-split scheme on resident feature tiles (k_fused6) when two step buffers of
        // whole-row images fit the LDS: short feature rows (C1, C2, C5).  Post blocks of one or two tiles
        // run as 4-wave workgroups, two per CU (less padding of K, barrier waits overlap).
        pl.mt = 0;
        pl.nw6 = 8;
        if (pl.version == 2 && single_slice && (h->opt_kernel == 0 || h->opt_kernel == 6) && h->opt_ptw == 0) {
            int ptw6 = pl.PTW, nw6 = 8, ktw6 = pl.KTW;
            if (pl.nPT <= 2) {
                nw6 = 4;
                ptw6 = pl.nPT;
                const int needw6 = (need + nw6 / ptw6 - 1) / (nw6 / ptw6);
                ktw6 = 0;
                for (int k : KTilesSplit::values)
                    if (k >= needw6 && k <= 10) {
                        ktw6 = k;
                        break;
                    }
                if (ktw6 == 0) { nw6 = 8; ptw6 = pl.PTW; ktw6 = pl.KTW; }
            }
            const int kt6 = ktw6 * (nw6 / ptw6);
            int mt6 = 0;
            for (int mt = (nw6 == 4 ? 1 : 2); mt >= 1 && mt6 == 0; --mt) {
                const size_t lds6 = (size_t)2 * mt * pgl_img_bytes(kt6) + (size_t)mt * nw6 * 2048 + 256 + (size_t)nw6 * 384;
                const size_t cap = (nw6 == 4) ? 80 * 1024 : 160 * 1024;      // two 4-wave workgroups per CU
                if (lds6 <= cap && (mt == 1 || pl.nTiles >= 4)) mt6 = mt;
            }
            if (mt6 == 0 && nw6 == 4) {                                      // does not fit twice: 8-wave form
                nw6 = 8; ptw6 = pl.PTW; ktw6 = pl.KTW;
                const int kt8 = ktw6 * (8 / ptw6);
                for (int mt = 2; mt >= 1 && mt6 == 0; --mt) {
                    const size_t lds6 = (size_t)2 * mt * pgl_img_bytes(kt8) + (size_t)mt * 8 * 2048 + 256 + (size_t)8 * 384;
                    if (lds6 <= 160 * 1024 && (mt == 1 || pl.nTiles >= 4)) mt6 = mt;
                }
            }
            pl.sb6 = 0;
            if (mt6 == 0 && pl.nPT <= 2 && h->opt_sb6 != 2) {
                // the row does not fit twice (K = 640: 81 KB per tile): two post tiles -> 8-wave form with ONE image buffer
                // (<10,2>: 4-way K split); one post tile -> 8-way K split with a private block ring per wave (k_fused8<5, 8>)
                nw6 = 8; ptw6 = pl.nPT;
                const int needw8 = (need + 8 / ptw6 - 1) / (8 / ptw6);
                ktw6 = (ptw6 == 1) ? 5 : 10;
                const size_t lds1 = (size_t)pgl_img_bytes(ktw6 * (8 / ptw6)) + (size_t)8 * 2048 + 256 + (size_t)8 * 384;
                if (needw8 <= ktw6 && needw8 > ktw6 / 2 && lds1 <= 160 * 1024) {
                    mt6 = 1;
                    // one post tile: every wave streams its own K slice through a private block ring (k_fused8) -- the
                    // HBM stream never stops for the fragment read-out (0.615 against 0.665 ms for a 16-neuron shard of C3)
                    pl.sb6 = (ptw6 == 1) ? 2 : 1;
                }
            }
            if (mt6 > 0) {
                const int ktall = ktw6 * (nw6 / ptw6);
                bool ok = true;
                pl.img32 = (pl.sb6 == 2 && h->opt_img32) ? 1 : 0;
                const int blk6 = (pl.sb6 == 2) ? 1 + pl.img32 : 0;
                if (h->opt_kernel == 0 && find_img(h, img_key6(ktall, blk6), pl.tile0, pl.nTiles) < 0)
                    ok = img_room(h, (size_t)pl.nTiles * img_bytes6(ktall, blk6));
                if (!ok) pl.sb6 = pl.img32 = 0;
                if (ok) {
                    pl.version = 6;
                    pl.mt = mt6; pl.nw6 = nw6; pl.PTW = ptw6; pl.KTW = ktw6; pl.KSPLIT = nw6 / ptw6;
                    pl.KT = ktall; pl.wpb = nw6;
                    pl.nPB = (pl.nPT + pl.PTW - 1) / pl.PTW;
                }
            }
        }
    }
    // version 7: no K split at all -- one wave per post tile carries the whole feature row (<= 20 k-tiles)
    // through forward, epilogue and backward; small workgroups, several per CU (k_fused7)
    pl.nw7 = 0;
    pl.wg7 = 1;
    // (measured, tools/small_shape_scan.py / config_table.py: 3-4 post tiles 46 TFLOP/s against 39 of the
    // K-split kernel at C5; with 1-2 post tiles only 2-6 waves fit a CU and the 4-wave K-split form wins -- except one
    // post tile of 4-5 k-tiles (N = 16 at B = 5: 0.065 against 0.083 ms, tools/shape_sweep.py).  Rows of 17-20 k-tiles
    // (N = 52..64 at B = 5) stay with the K-split kernel: 160 registers of G beside the epilogue spill (9-108 VGPRs
    // by variant) and k_fused6 is the faster one there anyway, 0.49 against 0.57 ms at N = 64)
    if ((pl.version == 2 || pl.version == 6) && !pl.f32 && single_slice && pl.nPT <= 4 && need <= 16 &&
        ((h->opt_kernel == 0 && (pl.nPT >= 3 || (pl.nPT == 1 && need >= 4 && need <= 5))) || h->opt_kernel == 7 || force7) &&
        h->opt_ptw == 0) {
        int kt7 = 0;
        for (int k : KTilesRow::values)
            if (k >= need) {
                kt7 = k;
                break;
            }
        const int nw7 = (pl.nPT >= 3 || force7) ? 4 : pl.nPT;       // force7: the slab-input form exists for 4 waves only
        // (force7 = separable stimulus: + the per-wave accumulators of the fused stimulus backward, k_fused7<.., 3>)
        const size_t lds7 = (size_t)2 * pgl_img_bytes(kt7) + 256 + (size_t)nw7 * 192 * 8 + (force7 ? (size_t)nw7 * 320 * 8 : 0);
        bool ok = kt7 > 0 && lds7 <= 160 * 1024;
        if (ok && h->opt_kernel == 0 && find_img(h, kt7 << 8, pl.tile0, pl.nTiles) < 0)
            ok = img_room(h, (size_t)pl.nTiles * pgl_img_bytes(kt7));
        if (ok) {
            pl.version = 7;
            pl.nw7 = nw7;
            pl.wg7 = (int)std::max<size_t>(1, std::min<size_t>((size_t)160 * 1024 / lds7, (size_t)(8 / nw7)));
            // one-wave workgroups: five to seven per CU put two waves on some SIMDs and one on the others -- the kernel ends
            // with the doubly loaded SIMDs while the others idle (N = 16: exits spread over 28 .. 67 us); one wave per SIMD
            // and longer chunks: 0.0876 -> 0.0828 ms per evaluation (tools/shape_sweep.py, chunk-count scan of round 6)
            if (nw7 == 1 && pl.wg7 > 4 && pl.wg7 < 8) pl.wg7 = 4;
            pl.PTW = nw7; pl.KSPLIT = 1; pl.KTW = kt7; pl.KT = kt7; pl.wpb = nw7;
            pl.nPB = (pl.nPT + nw7 - 1) / nw7;
            pl.mt = 0;
            pl.lds7x = force7 ? (size_t)nw7 * 320 * 8 : 0;
        }
    }
    pl.KS = pl.KT * 4;
    const int kpad = pl.KT * 16;
    pl.rsf = pl.f32 ? kpad + 4 : kpad + 2;
    int wgPerCU = (pl.version == 7) ? pl.wg7 : 1;
    if (pl.version == 6) {
        // as many workgroups per CU as registers and LDS allow (4-wave form at C2: three)
        pl.lds = (size_t)(pl.sb6 ? 1 : 2) * pl.mt * pgl_img_bytes(pl.KT) + (size_t)pl.mt * pl.nw6 * 2048 + 256 + (size_t)pl.nw6 * 384;
        if (pl.sb6 == 2) pl.lds = lds_fused8(pl.img32 ? 5 : kRing8);
        wgPerCU = (pl.sb6 == 2) ? 1 : fused6_wg_per_cu(pl);
    }
    int target = h->opt_nchunks > 0 ? h->opt_nchunks : std::max(1, wgPerCU * h->numCU / pl.nPB);
    // a wide population whose last post block holds one to six tiles (N = 144, 160, 192, 200, 320 ..): with the post blocks of a
    // chunk side by side, half the CUs (a third, ..) carry the light blocks and idle behind them (N = 160: 0.45 of the
    // peak).  One chunk per CU and post block, post-block-major: the dispatcher hands every CU a full block first and a
    // light one behind it -- balanced whatever the cost ratio (dev option 91 = 1: the chunk-major grid)
    pl.pb_major = (wide && pl.version == 5 && pl.nPB > 1 && pl.nPT % 8 >= 1 && pl.nPT % 8 <= 6 && h->opt_nchunks == 0 &&
                   h->opt_pbmajor != 1) ? 1 : 0;
    if (pl.pb_major) target = h->numCU;
    target = std::min(target, pl.nTiles);
    if (h->opt_nchunks == 0 && wgPerCU > 1) {
        // short recordings: a chunk keeps >= 8 tiles as long as every CU still gets a workgroup (per-chunk
        // prologue, partial write-out and the reduction over chunks are paid per chunk)
        // (one-wave workgroups -- a single post tile on k_fused7 -- have a light prologue and fill a SIMD each: chunks from
        //  four tiles on, every SIMD a wave; N = 16, T = 60 s: 0.047 -> 0.042 ms per evaluation, T = 20 s: 0.035 -> 0.033)
        const bool one_wave = pl.version == 7 && pl.nw7 == 1;
        const int floor_t = std::min(std::max(1, (one_wave ? 4 : 1) * h->numCU / pl.nPB), pl.nTiles);
        target = std::min(target, std::max(floor_t, pl.nTiles / (one_wave ? 4 : 8)));
    }
    pl.tilesPerChunk = (pl.nTiles + target - 1) / target;
    pl.nChunks = (pl.nTiles + pl.tilesPerChunk - 1) / pl.tilesPerChunk;
    pl.blocks = pl.nChunks * pl.nPB;
    pl.threads = 64 * pl.wpb;
    const size_t esz = pl.f32 ? 4 : 8;
    size_t off = ((size_t)16 * pl.rsf * esz + 15) & ~(size_t)15;
    if (pl.version == 5) {
        pl.lds = (size_t)2 * pgl_img_bytes(pl.ktl) + pgl_img_bytes(pl.kth) + 256 + 8 * 192 * 8;   // + per-wave spike scratch
        // the last block leaves waves without a post tile: they help (rows from 10 k-tiles on; dev option 92 = 1: never)
        const int nb = pl.nPT % 8;
        // (measured, r06_shape_sweep*.md / r06_shard_steps.txt: five or six tiles +7 .. 12 %; a light block of one or two tiles
        //  at the end of a wide population +4 .. 5 %; three tiles of a single slice (a 48-neuron range of C3) +5 %, but -2 % as the
        //  last block of a wide population, whose full blocks pay for the helper form; four tiles: the helpers share their
        //  tile's SIMD, +-0)
        const bool nb_ok = nb == 5 || nb == 6 || (wide ? (nb == 1 || nb == 2) : nb == 3);
        pl.hlp = (hlp_ok && nb_ok && pl.ktl >= 5 && h->opt_hlp != 1) ? 1 : 0;
        if (pl.hlp) pl.lds += 4 * 256 * 8;                                                         // + the helpers' partial currents
        if (pl.lds > 160 * 1024) return fail(PGL_ERR_UNSUPPORTED, "LDS budget exceeded");
        return PGL_OK;
    }
    if (pl.version == 7) {
        pl.lds = (size_t)2 * pgl_img_bytes(pl.KT) + 256 + (size_t)pl.nw7 * 192 * 8 + pl.lds7x;
        return PGL_OK;
    }
    if (pl.version == 6) {
        pl.lds = (size_t)(pl.sb6 ? 1 : 2) * pl.mt * pgl_img_bytes(pl.KT) + (size_t)pl.mt * pl.nw6 * 2048 + 256 + (size_t)pl.nw6 * 384;
        if (pl.sb6 == 2) pl.lds = lds_fused8(pl.img32 ? 5 : kRing8);
        // chunks are whole steps of mt tiles
        pl.tilesPerChunk = (pl.tilesPerChunk + pl.mt - 1) / pl.mt * pl.mt;
        pl.nChunks = (pl.nTiles + pl.tilesPerChunk - 1) / pl.tilesPerChunk;
        pl.blocks = pl.nChunks * pl.nPB;
        return PGL_OK;
    }
    if (pl.version == 4) {
        const int c0 = pl.KTW * 16;
        const int rsfh = c0 + ((c0 % 32 == 0) ? 16 : 32);
        off = std::max(off, (((size_t)2 * 16 * rsfh * 8) + 15) & ~(size_t)15);
        off += (((size_t)2 * h->B * pl.RP * 8) + 15) & ~(size_t)15;
        off += (size_t)sl.Ns * pl.cap * 8;
        off += 2 * ((((size_t)2 * sl.Ns * 4) + 15) & ~(size_t)15);
        off += (((size_t)sl.Ns * 4) + 15) & ~(size_t)15;
        off += 256;
        pl.lds = off;
        if (pl.lds > 160 * 1024) return fail(PGL_ERR_UNSUPPORTED, "LDS budget exceeded");
        return PGL_OK;
    }
    off += (((size_t)2 * h->B * pl.RP * esz) + 15) & ~(size_t)15;
    off += (size_t)sl.Ns * pl.cap * 8;
    off += 2 * ((((size_t)2 * sl.Ns * 4) + 15) & ~(size_t)15);
    off += (((size_t)sl.Ns * 4) + 15) & ~(size_t)15;                       // ring-valid flags
    off += (size_t)pl.wpb * 256 * 8 + (size_t)pl.PTW * 256 * 8 + 256;
    pl.lds = off;
    if (pl.lds > 160 * 1024) return fail(PGL_ERR_UNSUPPORTED, "LDS budget exceeded");
    return PGL_OK;
}

// The path an evaluation of neurons [n_lo, n_hi) (or of a list of n_hi - n_lo neurons) takes and its launch plans:
//   sepf   -- separable stimulus at the frame rate: impulse columns on resident tiles (k_fused7 with the slab-input form up to
//             four post tiles, the two-pass kernel from five on or when the feature row is too long for k_fused7), the
//             stimulus current / its gradients by k_sepf_*; neuron lists are fine there (the stimulus kernels work on the
//             listed rows, the fused kernel maps rows to neurons).  A kernel forced by PGL_OPT_KERNEL other than 7 / 4 keeps
//             the stimulus on the 3-phase path it asks for;
//   sliced -- the 3-phase path (more than one slice of feature columns, or a separable stimulus by the tap-rate kernels).
// One function for enqueue_ll_grad, pgl_info and the dry run of the dispatch (pgl_plan_kernels).
static int select_plans(const pgl_context* h, int n_lo, int n_hi, std::vector<Slice>& slices, std::vector<Plan>& plans,
                        bool& sepf, bool& sliced, bool* wide_out = nullptr)
{
    slices = make_slices(h, wide_out != nullptr);
    plans.assign(slices.size(), Plan());
    if (wide_out) *wide_out = false;
    // wide -- more than one slice of feature columns (N > 128 or more than 640 columns) with every slice on the resident-tile
    //         two-pass kernel: forward-only passes of the first slices add their currents in the slab, the last slice runs
    //         pass 1 from the slab, then the pass-2 kernels take the gradients of all column parts from the residuals.
    //         Needs rows of 7 .. 40 k-tiles in every slice (equal-width slices see to that from B = 2 on), no separable
    //         stimulus, f64 features, and the memory for one image set per slice; else the in-kernel-feature path below.
    if (wide_out && slices.size() > 1 && slices.size() <= (size_t)pgl_context::NIMG && !h->sep && !h->opt_f32 &&
        (h->opt_kernel == 0 || h->opt_kernel == 4)) {
        bool ok = true;
        size_t bytes = 0;
        for (const Slice& sl : slices) {
            const int need = (sl.Ns * h->B + sl.Ds + 15) / 16;
            int ktl = 0, kth = 0;
            if (sl.Ns <= 0 || need < 7 || need > 40 || !pick_pair(need, ktl, kth)) { ok = false; break; }
            const int tile0 = (int)(h->t_lo / 16), nTiles = (int)((h->t_hi + 15) / 16) - tile0;
            bytes += (size_t)nTiles * img_pair_bytes(ktl, kth);
        }
        if (ok && h->opt_kernel == 0) {
            // the image sets that are not resident yet must fit (with the residual slab) into 90 % of the free memory
            size_t free_b = 0, total_b = 0, have = 0;
            for (int i = 0; i < pgl_context::NIMG; ++i)
                if (h->imgs[i].key >> 16) have += h->imgs[i].buf.cap;
            if (bytes > have && hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes - have > free_b / 10 * 9) ok = false;
        }
        if (ok) {
            for (size_t i = 0; i < slices.size(); ++i) {
                int rc = make_plan(h, n_lo, n_hi, slices[i], plans[i], false, false, true);
                if (rc) return rc;
                if (plans[i].version != 5) ok = false;
            }
        }
        if (ok) {
            sepf = false;
            sliced = true;
            *wide_out = true;
            return PGL_OK;
        }
    }
    if (wide_out) {
        slices = make_slices(h);
        plans.assign(slices.size(), Plan());
    }
    sepf = h->sep && h->sepf && h->opt_sepf != 2 && slices.size() == 1 && !h->opt_f32 &&
           (h->opt_kernel == 0 || h->opt_kernel == 7 || h->opt_kernel == 4);
    if (sepf) {
        int rc = make_plan(h, n_lo, n_hi, slices[0], plans[0], true, true);
        if (rc) return rc;
        sepf = (plans[0].version == 7 && plans[0].nw7 == 4) || (plans[0].version == 5 && fused5_built(plans[0].ktl, 1, 0, 0));
    }
    for (size_t i = 0; i < slices.size() && !sepf; ++i) {
        int rc = make_plan(h, n_lo, n_hi, slices[i], plans[i], slices.size() == 1 && !h->sep);
        if (rc) return rc;
    }
    sliced = !sepf && (slices.size() > 1 || h->sep);     // else the separable stimulus rides on the 3-phase path
    return PGL_OK;
}

// The path of a Hessian-vector product over the prepared rows: `fused` -- one column slice on the resident-tile two-pass plan
// (the class of k_fused5: >= 5 post tiles, or >= 3 against a long row): k_hvp5 + pass 2 of k_fused5; else the 3-phase path on
// the K-split kernel's forward-only / backward-only launches, one set per column slice, around the row kernels of
// pglm_hvp.hip.h.
static int hvp_select(const pgl_context* h, int n_lo, int n_hi, std::vector<Slice>& slices, std::vector<Plan>& plans, bool& fused)
{
    slices = make_slices(h);
    plans.assign(slices.size(), Plan());
    fused = slices.size() == 1 && !h->opt_f32 && (h->opt_kernel == 0 || h->opt_kernel == 4);
    if (fused) {
        int rc = make_plan(h, n_lo, n_hi, slices[0], plans[0], true);
        if (rc) return rc;
        fused = plans[0].version == 5 && hvp5_built(plans[0].ktl);
    }
    for (size_t i = 0; i < slices.size() && !fused; ++i) {
        int rc = make_plan(h, n_lo, n_hi, slices[i], plans[i], false);
        if (rc) return rc;
    }
    return PGL_OK;
}

// Geometry of the dense Hessian (k_hess, pglm_hess.hip.h) of `count` prepared rows: column blocks of 64 and their pairs
// j <= i, the rows of one launch (eight per workgroup; the chunk partials of a launch, 32 KB per row and pair, stay within
// a fixed budget -- more rows than that run as several launches over the same buffer), time chunks so that a launch has about
// eight workgroups per CU when the pairs and rows alone do not give them.  Shape only: the dry run needs no device.
struct HessPlan {
    int nCB, nPairs, rowsPerLaunch, nChunks, tilesPerChunk, RP;
    size_t lds, partBytes;
};
static int hess_plan(const pgl_context* h, int count, HessPlan& hp)
{
    const int K = h->Kimp + h->Dstim + 1;
    hp.nCB = (K + PGL_HESS_CB - 1) / PGL_HESS_CB;
    hp.nPairs = hp.nCB * (hp.nCB + 1) / 2;
    hp.RP = h->Rk + 32;
    while (hp.RP % 32 != 8) ++hp.RP;
    hp.lds = (size_t)16 * PGL_HESS_LD * 8 + ((((size_t)2 * h->B * hp.RP * 8) + 15) & ~(size_t)15) +
             (size_t)2 * PGL_HESS_NPB * PGL_CAP * 8 + (size_t)4 * PGL_HESS_NPB * 4;
    if (hp.lds > 160 * 1024) return fail(PGL_ERR_UNSUPPORTED, "dense Hessian: the basis tables do not fit the LDS");
    const size_t per = (size_t)hp.nPairs * 4096 * 8;           // partial bytes per row and chunk
    const size_t budget = (size_t)512 << 20;
    long long rows = std::max<long long>(1, (long long)(budget / per));
    if (rows >= count) rows = count;
    else if (rows >= 8) rows &= ~7LL;
    hp.rowsPerLaunch = (int)rows;
    const int tile0 = (int)(h->t_lo / 16), nTiles = (int)((h->t_hi + 15) / 16) - tile0;
    const long long wgs = (long long)hp.nPairs * ((rows + 7) / 8);
    long long chunks = (8LL * h->numCU + wgs - 1) / wgs;
    chunks = std::min<long long>(chunks, std::max(1, nTiles / 8));
    chunks = std::min<long long>(chunks, std::max<long long>(1, (long long)(budget / (per * rows))));
    chunks = std::max<long long>(chunks, 1);
    hp.tilesPerChunk = (int)((nTiles + chunks - 1) / chunks);
    hp.nChunks = (nTiles + hp.tilesPerChunk - 1) / hp.tilesPerChunk;
    hp.partBytes = per * (size_t)rows * hp.nChunks;
    return PGL_OK;
}
