// Launch geometry of the batched collapsed-Gibbs columns (pgl_gibbs_ll_cols, pgl_gibbs_update_cols), in the style of
// pglm_ratewin.h: the rule and nothing else.  Plain integers in, one struct out, no HIP call: the host (pglm_capi.hip) owns the
// buffers and the launches, tests/csrc/gibbs_plan_host.c compiles this file with gcc, and tests/gibbs_reference.py::geometry is
// the independent statement it is compared with.  The constants the geometry depends on live here; the kernels
// (pglm_gibbs.hip.h, pglm_direct.hip.h) read them from this file.
//
// Two paths of pgl_gibbs_ll_cols:
//   regime  k_gibbs_cols_setup [+ k_gibbs_pre_features] + k_gibbs_rate_cols + k_gibbs_reduce_cols2: rate terms in sub-blocks of
//           PGL_GRB bins (single precision for the log1p term where |x| >= 12, compacted f64 elsewhere), spike terms from the
//           event lists by extra workgroups of the same 1-D launch.  explinear only, and only while a window's event count fits
//           16 bits (R + PGL_GRB + 32 < 65535).
//   f64     k_gibbs_ll_cols + k_gibbs_reduce_cols: everything in double (the exp nonlinearity, or PGL_OPT_GIBBS_KERNEL = 1).
// The regime path is planned in two steps because its loop length depends on the kernel's occupancy at the launch's LDS size,
// which only the runtime knows: pgl_gibbs_plan_shape gives the LDS bytes, the host asks for the workgroups per CU at that size
// and hands slots = workgroups per CU x CUs to pgl_gibbs_plan_loop.  The f64 path is complete after the first step.
//
// Plain C subset, host only.
#ifndef PGLM_GIBBS_PLAN_H
#define PGLM_GIBBS_PLAN_H

#include <stddef.h>

#define PGL_KMAX 16           // candidate weights per launch (pgl_gibbs_ll_cols: K <= PGL_KMAX; pgl_gibbs_ll loops over chunks)
#ifndef PGL_GRB
#define PGL_GRB 256           // bins per sub-block of k_gibbs_rate_cols (a multiple of 64)
#endif
#ifndef PGL_GQ
#define PGL_GQ PGL_GRB        // band-queue entries per wave (the band elements of one weight: <= PGL_GRB)
#endif
#define PGL_GNL 16            // at most this many sub-blocks per workgroup
#define PGL_GECAP 24          // staged presynaptic events per column and block (k_gibbs_ll_cols)
#define PGL_GECAP_R 20        // staged presynaptic events per column and sub-block (~9 at 20 Hz; more: read from HBM)
#ifdef PGL_SPT_GLOBAL
#define PGL_SPT_N 2
#else
#define PGL_SPT_N 196         // doubles of the softplus-tail table in LDS (97 x 2, padded)
#endif

// ---- the debug option (99) as the Gibbs path reads it ----
#define PGL_GDBG_ABLATE 0xff                  // bits 0..7: the kernels' ablation byte (GibbsColsParams::dbg)
#define PGL_GDBG_NLOOP4_SHIFT 8               // bits 8..11: the older forced sub-block loop, 1 .. 15
#define PGL_GDBG_NLOOP4_MASK 0xf
#define PGL_GDBG_NO_SAME_PRE 0x1000           // bit 12: never build the shared presynaptic features
#define PGL_GDBG_NLOOP5_SHIFT 16              // bits 16..20: the forced sub-block loop, 1 .. 31 (capped at PGL_GNL)
#define PGL_GDBG_NLOOP5_MASK 0x1f

typedef struct {
    int ablate;               // handed to the kernels
    int no_same_pre;          // 1: the same_pre switch is off
    int nloop;                // forced sub-block loop, 0 = the host's choice: the 5-bit field when it is non-zero, else the 4-bit
                              // one (16 << 8 is bit 12 and forces nothing)
} PglGibbsDbg;

static inline PglGibbsDbg pgl_gibbs_dbg(int opt_dbg)
{
    PglGibbsDbg d;
    const int n5 = (opt_dbg >> PGL_GDBG_NLOOP5_SHIFT) & PGL_GDBG_NLOOP5_MASK;
    d.ablate = opt_dbg & PGL_GDBG_ABLATE;
    d.no_same_pre = (opt_dbg & PGL_GDBG_NO_SAME_PRE) != 0;
    d.nloop = n5 ? n5 : (opt_dbg >> PGL_GDBG_NLOOP4_SHIFT) & PGL_GDBG_NLOOP4_MASK;
    return d;
}

// ---- the plan ----
#define PGL_GIBBS_REGIME 0
#define PGL_GIBBS_F64 1

typedef struct {
    int path;                 // PGL_GIBBS_REGIME / PGL_GIBBS_F64
    int CP;                   // columns per workgroup
    int ygroups;              // groups of CP columns
    int nblk;                 // time blocks: of nloop sub-blocks (regime), of `rows` bins (f64, update)
    // regime
    int nsplit;               // time splits of a sub-block over the waves (narrow launches); (PGL_GRB / 64) % nsplit == 0
    long long nsub;           // sub-blocks of PGL_GRB bins
    int same_pre;             // every column has the same presynaptic neuron: its filtered spike train once per launch
    int hs_region;            // doubles of the first LDS region
    long long fs_stride;      // row stride of the filtered spike train (0 unless same_pre)
    int nloop;                // sub-blocks per workgroup
    int sblk;                 // spike workgroups per column, 256 events each
    unsigned grid;            // 1-D grid of k_gibbs_rate_cols: nblk x ygroups rate workgroups, then sblk x ncols spike workgroups
    int dbg;                  // the kernels' ablation byte
    // f64 and update
    int gtb;                  // bins per sub-block (multiple of 32, gtb * CP >= 256)
    int rows;                 // bins per block
    size_t lds;               // dynamic LDS bytes of k_gibbs_rate_cols / k_gibbs_ll_cols / k_gibbs_update_cols
} PglGibbsPlan;

static inline long long pgl_gibbs_ceil(long long a, long long b) { return (a + b - 1) / b; }

// what a path does not use: zero, and one split / one sub-block per workgroup
static inline void pgl_gibbs_plan_clear(PglGibbsPlan* pl)
{
    pl->path = 0; pl->CP = 0; pl->ygroups = 0; pl->nblk = 0;
    pl->nsplit = 1; pl->nsub = 0; pl->same_pre = 0; pl->hs_region = 0; pl->fs_stride = 0;
    pl->nloop = 1; pl->sblk = 0; pl->grid = 0; pl->dbg = 0; pl->gtb = 0; pl->rows = 0; pl->lds = 0;
}

// columns per workgroup where a thread is one (column, weight) pair: k_gibbs_ll_cols, and k_gibbs_update_cols with nw = 1
static inline int pgl_gibbs_cp(int ncols, int nw)
{
    const int fit = 256 / (nw > 1 ? nw : 1);
    const int cp = ncols < fit ? ncols : fit;
    return cp > 1 ? cp : 1;
}

// the regime-split path serves explinear unless PGL_OPT_GIBBS_KERNEL = 1, while the event count of a window fits 16 bits
static inline int pgl_gibbs_path(int explinear, int opt_gibbs, int Rk)
{
    return (explinear && opt_gibbs != 1 && Rk + PGL_GRB + 32 < 65535) ? PGL_GIBBS_REGIME : PGL_GIBBS_F64;
}

// Step 1.  ncols columns of K weights over nrows bins; pre_equal: all n_pre are the same neuron; max_ev: the largest number of
// post-synaptic events of a listed column inside the range; explinear: nlin == PGL_NLIN_EXPLINEAR; B basis functions of Rk taps.
// Fills everything but nloop, nblk and grid of the regime path (pgl_gibbs_plan_loop), and all of the f64 path.
static inline void pgl_gibbs_plan_shape(PglGibbsPlan* pl, int ncols, int K, int pre_equal, long long nrows, int max_ev,
                                        int explinear, int opt_gibbs, int opt_dbg, int B, int Rk, int numCU)
{
    const PglGibbsDbg d = pgl_gibbs_dbg(opt_dbg);
    pgl_gibbs_plan_clear(pl);
    pl->path = pgl_gibbs_path(explinear, opt_gibbs, Rk);
    if (pl->path == PGL_GIBBS_REGIME) {
        pl->CP = ncols < 8 ? ncols : 8;
        pl->nsplit = (pl->CP >= 3) ? 1 : (pl->CP == 2) ? 2 : ((PGL_GRB / 64) % 4 == 0 ? 4 : 3);
        pl->ygroups = (ncols + pl->CP - 1) / pl->CP;
        pl->nsub = pgl_gibbs_ceil(nrows, PGL_GRB);
        pl->same_pre = ncols >= 2 && !d.no_same_pre && pre_equal;
        pl->hs_region = pl->CP * Rk;
        if (pl->same_pre) {
            const int feat = B * (PGL_GRB + 2) + pl->CP * 8;
            if (feat > pl->hs_region) pl->hs_region = feat;
            pl->fs_stride = pgl_gibbs_ceil(nrows, 64) * 64;
        }
        // x0 / ic rows, the weights, the band queue of each wave, the softplus-tail table, max |w|; then the staged events,
        // and per (column, sub-block of the loop) a 4-byte first event and a 2-byte count
        pl->lds = ((size_t)pl->hs_region + (size_t)pl->CP * (PGL_GRB + 2) + (size_t)pl->CP * PGL_KMAX + (size_t)4 * PGL_GQ +
                   (size_t)PGL_SPT_N + (size_t)pl->CP) * 8 +
                  (size_t)pl->CP * PGL_GECAP_R * 8 + (size_t)pl->CP * PGL_GNL * 6 + 16;
        pl->sblk = (max_ev + 255) / 256 > 1 ? (max_ev + 255) / 256 : 1;
        pl->dbg = d.ablate;
        return;
    }
    // enough blocks for a few per CU, at most 384 bins each (the block's presynaptic events -- window of rows + R bins, ~11 at
    // 20 Hz -- are staged in LDS, PGL_GECAP per column), whole sub-blocks
    pl->CP = pgl_gibbs_cp(ncols, K);
    pl->ygroups = (ncols + pl->CP - 1) / pl->CP;
    pl->gtb = 32;
    while (pl->gtb * pl->CP < 256) pl->gtb += 32;         // narrow launches: longer sub-blocks keep 256 threads busy
    long long rows = pgl_gibbs_ceil(nrows * pl->ygroups, 4LL * numCU);
    rows = rows < 384 ? rows : 384;
    rows = rows > pl->gtb ? rows : pl->gtb;
    pl->rows = (int)(pgl_gibbs_ceil(rows, pl->gtb) * pl->gtb);
    pl->nblk = (int)pgl_gibbs_ceil(nrows, pl->rows);
    pl->lds = ((size_t)B * Rk + (size_t)3 * pl->gtb * pl->CP) * 8 + (size_t)pl->CP * PGL_GECAP * 8 + (size_t)pl->CP * 4;
}

// Step 2, regime path.  slots: workgroups of k_gibbs_rate_cols the device holds at pl->lds bytes (per CU x CUs).
// Sub-blocks per workgroup: short loops.  The columns differ in how many of their elements fall into the f64 band, so
// workgroups differ in run time and the dispatcher's dynamic placement has to even that out.  Measured at C4 (37 504 sub-block
// units on 1 024 slots: four workgroups per CU at <= 40 KB of LDS and 128 VGPRs): loops of 3..10 sub-blocks run within 1 % of
// each other (1.14 ms per launch), 13 = three well-filled rounds 1.19 ms, 16 1.25 ms, 37 = ONE round filled to 99 % 1.23 ms.
// So: at least six rounds of workgroups, loops of at most eight sub-blocks (the per-workgroup setup is amortised from ~4).
// The debug option forces a loop of 1 .. PGL_GNL (tests).
static inline void pgl_gibbs_plan_loop(PglGibbsPlan* pl, int ncols, int opt_dbg, long long slots)
{
    const int forced = pgl_gibbs_dbg(opt_dbg).nloop;
    long long nloop = pl->nsub * pl->ygroups / (6 * slots);
    nloop = nloop < 8 ? nloop : 8;
    nloop = nloop > 1 ? nloop : 1;
    if (forced) nloop = forced < PGL_GNL ? forced : PGL_GNL;
    pl->nloop = (int)nloop;
    pl->nblk = (int)pgl_gibbs_ceil(pl->nsub, pl->nloop);
    pl->grid = (unsigned)(pl->nblk * pl->ygroups + pl->sblk * ncols);
}

// the ten integers of pgl_gibbs_last_geometry: path, CP, nsplit, ygroups, nloop, nblk, sblk, same_pre, gtb, rows
static inline void pgl_gibbs_plan_report(const PglGibbsPlan* pl, int out[10])
{
    out[0] = pl->path; out[1] = pl->CP; out[2] = pl->nsplit; out[3] = pl->ygroups; out[4] = pl->nloop;
    out[5] = pl->nblk; out[6] = pl->sblk; out[7] = pl->same_pre; out[8] = pl->gtb; out[9] = pl->rows;
}

// pgl_gibbs_update_cols: one delta per column (a thread is a column), blocks of 1024 bins, the basis in LDS
static inline void pgl_gibbs_plan_update(PglGibbsPlan* pl, int ncols, long long nrows, int B, int Rk)
{
    pgl_gibbs_plan_clear(pl);
    pl->path = PGL_GIBBS_F64;
    pl->CP = pgl_gibbs_cp(ncols, 1);
    pl->ygroups = (ncols + pl->CP - 1) / pl->CP;
    pl->rows = 1024;
    pl->nblk = (int)pgl_gibbs_ceil(nrows, pl->rows);
    pl->lds = (size_t)B * Rk * 8;
}

#endif
