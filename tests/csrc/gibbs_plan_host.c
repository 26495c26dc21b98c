/* Host build of the collapsed-Gibbs launch plan (theano_pyglm_amd/csrc/pglm_gibbs_plan.h) for the CPU tests:
 *   gp_consts   PGL_KMAX, PGL_GRB, PGL_GQ, PGL_GNL, PGL_GECAP, PGL_GECAP_R, PGL_SPT_N (7 ints);
 *   gp_dbg      the decoded debug option: ablation byte, same_pre switch off, forced loop (3 ints);
 *   gp_plan     pgl_gibbs_plan_shape, then for the regime path pgl_gibbs_plan_loop with `slots`, as the host chains them; out:
 *               the ten integers of pgl_gibbs_last_geometry, then nsub, grid, hs_region, fs_stride, lds, dbg (16 long longs);
 *   gp_update   the geometry of pgl_gibbs_update_cols: CP, ygroups, rows, nblk, lds (5 long longs). */
#include "../../theano_pyglm_amd/csrc/pglm_gibbs_plan.h"

void gp_consts(int* out)
{
    out[0] = PGL_KMAX; out[1] = PGL_GRB; out[2] = PGL_GQ; out[3] = PGL_GNL; out[4] = PGL_GECAP; out[5] = PGL_GECAP_R;
    out[6] = PGL_SPT_N;
}

void gp_dbg(int opt_dbg, int* out)
{
    const PglGibbsDbg d = pgl_gibbs_dbg(opt_dbg);
    out[0] = d.ablate; out[1] = d.no_same_pre; out[2] = d.nloop;
}

void gp_plan(int ncols, int K, int pre_equal, long long nrows, int max_ev, int explinear, int opt_gibbs, int opt_dbg, int B,
             int Rk, int numCU, long long slots, long long* out)
{
    PglGibbsPlan pl;
    int geo[10];
    pgl_gibbs_plan_shape(&pl, ncols, K, pre_equal, nrows, max_ev, explinear, opt_gibbs, opt_dbg, B, Rk, numCU);
    if (pl.path == PGL_GIBBS_REGIME) pgl_gibbs_plan_loop(&pl, ncols, opt_dbg, slots);
    pgl_gibbs_plan_report(&pl, geo);
    for (int i = 0; i < 10; ++i) out[i] = geo[i];
    out[10] = pl.nsub; out[11] = pl.grid; out[12] = pl.hs_region; out[13] = pl.fs_stride; out[14] = (long long)pl.lds;
    out[15] = pl.dbg;
}

void gp_update(int ncols, long long nrows, int B, int Rk, long long* out)
{
    PglGibbsPlan pl;
    pgl_gibbs_plan_update(&pl, ncols, nrows, B, Rk);
    out[0] = pl.CP; out[1] = pl.ygroups; out[2] = pl.rows; out[3] = pl.nblk; out[4] = (long long)pl.lds;
}
