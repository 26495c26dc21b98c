// NUTS row kernels: k_nuts_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// The No-U-Turn sampler (inference/batched_nuts.py) for the chains of all M neurons of a range -- one workgroup per neuron
// row -- around the one launch that does the work: a fused ll+grad evaluation of all rows per leapfrog step
// (pgl_ll_grad_dev).  The transition, its random numbers and its decisions are pglm_nuts.h (compiled for the host by
// tests/csrc/nuts_host.c); these kernels own the vectors, the fixed-order reductions (pgl_blk_sum), the priors' part of U
// and its gradient (pgl_hmc_target_row).  All state lives in ONE device block of doubles laid out by pgl_nuts_view.
// Rows do not wait for each other: a row that ends a transition writes its kept point, draws the next momentum and starts
// the next tree in the same launch; after its last transition it sets its done flag and returns at once from then on,
// its Xt row left at its current point.
// The inverse mass matrix W W^T: diagonal (minv, W = diag(sqrt(minv)), or none) -- everything is ONE launch of k_nuts_step
// per leapfrog step;  dense (W (M, P, P)) -- k_nuts_target, the product W^T grad U (k_tri_matvec, stored), k_nuts_step,
// and the product W r with the drift as its epilogue (k_tri_matvec<0, DRIFT> with the row's signed step).
// ---------------------------------------------------------------------------
#include "pglm_adapt.h"                         // (pglm_nuts.h, and the mass adaptation's rules)
#include <cstddef>

struct NutsView {
    int M, P, D;
    double* vec;                              // (PGL_NUTS_NVEC + 2 D, M, P)
    double* sc;                               // (PGL_NUTS_NSCAL, M): PglNuts, field-major
};
__host__ __device__ inline size_t pgl_nuts_doubles(int M, int P, int D)
{
    return (size_t)M * P * (PGL_NUTS_NVEC + 2 * D) + (size_t)M * PGL_NUTS_NSCAL;
}
__host__ __device__ inline NutsView pgl_nuts_view(double* st, int M, int P, int D)
{
    NutsView v;
    v.M = M; v.P = P; v.D = D;
    v.vec = st;
    v.sc = st + (size_t)M * P * (PGL_NUTS_NVEC + 2 * D);
    return v;
}
// row r of vector k
__device__ __forceinline__ double* pgl_nuts_row(const NutsView& v, int k, int r)
{
    return v.vec + ((size_t)k * v.M + r) * v.P;
}
#define PGL_NUTS_FIELDS(F) F(Uc, 0) F(H0, 1) F(step, 2) F(t, 3) F(neuron, 4) F(seed_lo, 5) F(seed_hi, 6) F(done, 7) \
    F(depth, 8) F(v, 9) F(i, 10) F(lw_tree, 11) F(lw_sub, 12) F(Us, 13) F(sum_acc, 14) F(n_leaf, 15) F(sel, 16) \
    F(sel_sub, 17) F(hbar, 18) F(logeps_bar, 19) F(mu, 20) F(n_leapfrog, 21) F(n_div, 22) F(acc_post, 23) \
    F(last_depth, 24) F(last_nleaf, 25) F(last_stop, 26) F(last_sel, 27) F(last_acc, 28) F(ve, 29)
enum { PGL_NUTS_F_H0 = 1, PGL_NUTS_F_DONE = 7, PGL_NUTS_F_DEPTH = 8, PGL_NUTS_F_V = 9, PGL_NUTS_F_I = 10, PGL_NUTS_F_VE = 29 };
// the table above and the constants are the struct's order: a reordered field does not compile
static_assert(sizeof(PglNuts) == PGL_NUTS_NSCAL * sizeof(double), "PglNuts: PGL_NUTS_NSCAL doubles");
#define PGL_NUTS_CHK(name, k) static_assert(offsetof(PglNuts, name) == (k) * sizeof(double), "PGL_NUTS_FIELDS: " #name);
PGL_NUTS_FIELDS(PGL_NUTS_CHK)
#undef PGL_NUTS_CHK
static_assert(offsetof(PglNuts, H0) == PGL_NUTS_F_H0 * sizeof(double) && offsetof(PglNuts, done) == PGL_NUTS_F_DONE * sizeof(double) &&
              offsetof(PglNuts, depth) == PGL_NUTS_F_DEPTH * sizeof(double) && offsetof(PglNuts, v) == PGL_NUTS_F_V * sizeof(double) &&
              offsetof(PglNuts, i) == PGL_NUTS_F_I * sizeof(double) && offsetof(PglNuts, ve) == PGL_NUTS_F_VE * sizeof(double),
              "PGL_NUTS_F_*");
__device__ __forceinline__ void pgl_nuts_load(const NutsView& v, int r, PglNuts* s)
{
#define PGL_NUTS_LD(name, k) s->name = v.sc[(size_t)k * v.M + r];
    PGL_NUTS_FIELDS(PGL_NUTS_LD)
#undef PGL_NUTS_LD
}
__device__ __forceinline__ void pgl_nuts_store(const NutsView& v, int r, const PglNuts* s)
{
#define PGL_NUTS_ST(name, k) v.sc[(size_t)k * v.M + r] = s->name;
    PGL_NUTS_FIELDS(PGL_NUTS_ST)
#undef PGL_NUTS_ST
}

// dense mass: (ll, grad) -> U, grad U in place at the rows' points x = vector `which` of the state (QC at the start of a
// chain, QW in it); the product W^T grad U reads grad next
__global__ __launch_bounds__(256) void k_nuts_target(const NutsView v, const int which, double* __restrict__ ll,
                                                     double* __restrict__ grad, const BfgsPrior q)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x;
    const double U = pgl_hmc_target_row(pgl_nuts_row(v, which, r), grad + (size_t)r * v.P, ll[r], q, red, tid);
    if (tid == 0) ll[r] = U;
}

// What follows a decision, per element c of the row: fresh momentum at the candidate (act & END), the first half kick of
// the next leaf from the leaf itself (CONT) or from the edge on side vnew (NEWSUB), and -- diagonal mass -- the drift.
// Returns z^2 of a fresh momentum, else 0.
__device__ __forceinline__ double pgl_nuts_advance_elem(const NutsView& v, const int r, const int c, const int act,
                                                        const double vnew, const double ve, const pgl_hmc_u64 key,
                                                        const bool dense, const double* __restrict__ minv,
                                                        double* __restrict__ Xt)
{
    const size_t o = (size_t)r * v.P + c;
    double* qw = pgl_nuts_row(v, PGL_NUTS_QW, r) + c;
    double* rw = pgl_nuts_row(v, PGL_NUTS_RW, r) + c;
    double zz = 0.0;
    if (act & PGL_NUTS_DONE) {
        const double qc = pgl_nuts_row(v, PGL_NUTS_QC, r)[c];
        *qw = qc; *rw = 0.0;
        Xt[o] = qc;
        return 0.0;
    }
    if (act & PGL_NUTS_END) {
        const double z = pgl_hmc_normal(key, (pgl_hmc_u64)c);
        const double qc = pgl_nuts_row(v, PGL_NUTS_QC, r)[c], hc = pgl_nuts_row(v, PGL_NUTS_HC, r)[c];
        pgl_nuts_row(v, PGL_NUTS_QL, r)[c] = qc; pgl_nuts_row(v, PGL_NUTS_QR, r)[c] = qc;
        pgl_nuts_row(v, PGL_NUTS_HL, r)[c] = hc; pgl_nuts_row(v, PGL_NUTS_HR, r)[c] = hc;
        pgl_nuts_row(v, PGL_NUTS_RL, r)[c] = z; pgl_nuts_row(v, PGL_NUTS_RR, r)[c] = z;
        pgl_nuts_row(v, PGL_NUTS_RHO, r)[c] = z;
        zz = z * z;
    }
    double base, rn;
    if (act & PGL_NUTS_NEWSUB) {
        const bool right = vnew > 0.0;
        base = pgl_nuts_row(v, right ? PGL_NUTS_QR : PGL_NUTS_QL, r)[c];
        rn = pgl_nuts_half_kick(pgl_nuts_row(v, right ? PGL_NUTS_RR : PGL_NUTS_RL, r)[c], ve,
                                pgl_nuts_row(v, right ? PGL_NUTS_HR : PGL_NUTS_HL, r)[c]);
        pgl_nuts_row(v, PGL_NUTS_RHOS, r)[c] = 0.0;
    } else {
        base = *qw;
        rn = pgl_nuts_half_kick(*rw, ve, pgl_nuts_row(v, PGL_NUTS_HB, r)[c]);
    }
    *rw = rn;
    if (dense) *qw = base;                                                     // (the drift is the product's epilogue)
    else {
        const double qn = pgl_nuts_drift(base, ve, (minv ? sqrt(minv[o]) : 1.0) * rn);
        *qw = qn;
        Xt[o] = qn;
    }
    return zz;
}

// start of a chain: the rows' points are in QC.  Diagonal mass: (ll, grad) hold ll and its gradient there (overwritten
// with U and grad U); dense: U and grad U already (k_nuts_target) and HB = W^T grad U.  Draws the first momentum and
// takes the first half kick (and, diagonal, the first drift: Xt[row] = the point to evaluate).  chain_rows: k_hmc_init's.
__global__ __launch_bounds__(256) void k_nuts_init(const NutsView v, double* __restrict__ ll, double* __restrict__ grad,
                                                   const BfgsPrior q, const int dense, const double* __restrict__ minv,
                                                   const int n_lo, const double* __restrict__ step0,
                                                   const unsigned long long seed, const int n_total, double* __restrict__ Xt,
                                                   const int chain_rows)
{
    __shared__ double red[12];
    __shared__ PglNuts sh;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    double U = ll[r];
    if (!dense) {
        U = pgl_hmc_target_row(pgl_nuts_row(v, PGL_NUTS_QC, r), grad + o, ll[r], q, red, tid);
        __syncthreads();                                                       // grad U of the row is in memory
    }
    for (int c = tid; c < P; c += 256) {
        const double g = grad[o + c];
        pgl_nuts_row(v, PGL_NUTS_GC, r)[c] = g;
        pgl_nuts_row(v, PGL_NUTS_HC, r)[c] = dense ? pgl_nuts_row(v, PGL_NUTS_HB, r)[c] : (minv ? sqrt(minv[o + c]) : 1.0) * g;
    }
    if (tid == 0) {
        pgl_nuts_init(&sh, P, U, step0[r], n_lo + r % chain_rows, pgl_chain_seed(seed, (pgl_hmc_u64)(r / chain_rows)), n_total);
        ll[r] = U;
    }
    __syncthreads();
    const int act = sh.done != 0.0 ? PGL_NUTS_DONE : (PGL_NUTS_END | PGL_NUTS_NEWSUB);
    const pgl_hmc_u64 key = pgl_nuts_row_key(&sh);
    double ks = 0.0;
    for (int c = tid; c < P; c += 256) ks += pgl_nuts_advance_elem(v, r, c, act, sh.v, sh.ve, key, dense != 0, minv, Xt);
    ks = pgl_blk_sum(ks, red);
    if (tid == 0) {
        pgl_nuts_energy0(&sh, ks);
        pgl_nuts_store(v, r, &sh);
    }
}

// One leapfrog step of every row that is not done, after ONE evaluation of all rows at Xt = QW.  Diagonal mass: (ll, grad)
// come in and are turned into U, grad U in place; dense: they are U and grad U (k_nuts_target) and HB = W^T grad U.
// Completes the leaf, takes the decisions of pgl_nuts_leaf, moves the vectors, writes a kept point into
// samples[slot, row] and (depth, leaves) into stats[slot, :, row], and prepares the next leaf.
// ADAPT (k_nuts_adapt_step; diagonal mass only): the row's mass adaptation of pglm_adapt.h at the row's own transition
// boundary -- after the candidate of the ended transition is in QC and before the next momentum and edge are formed: the
// Welford update of the window with QC, and at a window's end the new row of minv (this launch's leaf was still formed
// with the old one), HC = sqrt(minv) o GC with it, and the restart of the dual averaging.
template <int ADAPT>
__device__ __forceinline__ void pgl_nuts_step_row(const NutsView v, double* __restrict__ ll, double* __restrict__ grad,
                                                  const BfgsPrior q, const int dense, const double* minv,
                                                  const double delta, const int n_warmup, const int thin, const int n_keep,
                                                  double* __restrict__ Xt, double* __restrict__ samples,
                                                  double* __restrict__ stats, const AdaptView a, const int* __restrict__ sched,
                                                  double* minv_out)
{
    __shared__ double red[12];
    __shared__ double sdots[2 * PGL_NUTS_MAX_DEPTH + 2];
    __shared__ PglNuts sh;
    __shared__ int sact, sslot, sadapt;
    __shared__ double sn;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P, M = v.M, D = v.D;
    const size_t o = (size_t)r * P;
    if (v.sc[(size_t)PGL_NUTS_F_DONE * M + r] != 0.0) return;                  // (the whole workgroup)
    double* qw = pgl_nuts_row(v, PGL_NUTS_QW, r);
    double* rw = pgl_nuts_row(v, PGL_NUTS_RW, r);
    double* hb = pgl_nuts_row(v, PGL_NUTS_HB, r);
    double* rhos = pgl_nuts_row(v, PGL_NUTS_RHOS, r);
    double U1 = ll[r];
    if (!dense) {
        U1 = pgl_hmc_target_row(qw, grad + o, ll[r], q, red, tid);
        __syncthreads();                                                       // grad U of the row is in memory
    }
    const double ve = v.sc[(size_t)PGL_NUTS_F_VE * M + r], vold = v.sc[(size_t)PGL_NUTS_F_V * M + r];
    const int i = (int)v.sc[(size_t)PGL_NUTS_F_I * M + r], size = 1 << ((int)v.sc[(size_t)PGL_NUTS_F_DEPTH * M + r] - 1);
    const int nb = pgl_nuts_trailing_ones(i), pc = pgl_nuts_popcount(i);
    const bool right = vold > 0.0;
    // ---- the leaf's momentum, the checkpoint of an even leaf, the subtree's rho ----
    double ks = 0.0;
    for (int c = tid; c < P; c += 256) {
        double h = hb[c];
        if (!dense) {
            h = (minv ? sqrt(minv[o + c]) : 1.0) * grad[o + c];
            hb[c] = h;
        }
        const double rl = pgl_nuts_half_kick(rw[c], ve, h);
        rw[c] = rl;
        ks += rl * rl;
        const double rs = rhos[c];
        if (!(i & 1)) {
            pgl_nuts_row(v, PGL_NUTS_NVEC + pc, r)[c] = rl;
            pgl_nuts_row(v, PGL_NUTS_NVEC + D + pc, r)[c] = rs;
        }
        rhos[c] = rs + rl;
    }
    ks = pgl_blk_sum(ks, red);
    // ---- the U-turn products of the blocks that end at this leaf, and of the tree a merge would make ----
    for (int k = 1; k <= nb; ++k) {
        const double* cr = pgl_nuts_row(v, PGL_NUTS_NVEC + pc - k, r);
        const double* crho = pgl_nuts_row(v, PGL_NUTS_NVEC + D + pc - k, r);
        double a = 0.0, b = 0.0;
        for (int c = tid; c < P; c += 256) {
            const double rb = rhos[c] - crho[c];
            a += rb * cr[c];
            b += rb * rw[c];
        }
        a = pgl_blk_sum(a, red);
        b = pgl_blk_sum(b, red);
        if (tid == 0) {
            sdots[2 * (k - 1)] = a;
            sdots[2 * (k - 1) + 1] = b;
        }
    }
    double dl = 0.0, dr = 0.0;
    if (i == size - 1) {
        const double* el = right ? pgl_nuts_row(v, PGL_NUTS_RL, r) : rw;
        const double* er = right ? rw : pgl_nuts_row(v, PGL_NUTS_RR, r);
        const double* rho = pgl_nuts_row(v, PGL_NUTS_RHO, r);
        for (int c = tid; c < P; c += 256) {
            const double rt = rho[c] + rhos[c];
            dl += rt * el[c];
            dr += rt * er[c];
        }
        dl = pgl_blk_sum(dl, red);
        dr = pgl_blk_sum(dr, red);
    }
    // ---- the decisions ----
    if (tid == 0) {
        pgl_nuts_load(v, r, &sh);
        int slot = -1;
        if (ADAPT) {
            PglAdapt ad;
            ad.count = a.count[r]; ad.widx = a.widx[r];
            sact = pgl_nuts_leaf_from(&sh, P, D, U1, ks, sdots, dl, dr, delta, n_warmup, thin, n_keep, &slot, (double*)0,
                                      pgl_adapt_restart_t(&ad, sched));
            int aa = 0;
            double n = 0.0;
            if (sact & PGL_NUTS_END) aa = pgl_adapt_row(&ad, sched, (int)sh.t - 1, &n);
            if (aa) {
                a.count[r] = ad.count; a.widx[r] = ad.widx;
            }
            if (aa & PGL_ADAPT_SWITCH) pgl_adapt_restart_nuts(&sh);
            sadapt = aa; sn = n;
        } else
            sact = pgl_nuts_leaf(&sh, P, D, U1, ks, sdots, dl, dr, delta, n_warmup, thin, n_keep, &slot, (double*)0);
        sslot = slot;
        ll[r] = U1;
        if ((sact & PGL_NUTS_END) && slot >= 0 && stats) {
            stats[((size_t)slot * 2 + 0) * M + r] = sh.last_depth;
            stats[((size_t)slot * 2 + 1) * M + r] = sh.last_nleaf;
        }
    }
    __syncthreads();
    const int act = sact, slot = sslot;
    const pgl_hmc_u64 key = pgl_nuts_row_key(&sh);                              // (of the NEXT transition after END)
    // ---- the vectors ----
    double ks0 = 0.0;
    for (int c = tid; c < P; c += 256) {
        if (act & PGL_NUTS_TAKE_LEAF) {
            pgl_nuts_row(v, PGL_NUTS_QS, r)[c] = qw[c];
            pgl_nuts_row(v, PGL_NUTS_GS, r)[c] = grad[o + c];
            pgl_nuts_row(v, PGL_NUTS_HS, r)[c] = hb[c];
        }
        if (act & PGL_NUTS_MERGE) {
            pgl_nuts_row(v, right ? PGL_NUTS_QR : PGL_NUTS_QL, r)[c] = qw[c];
            pgl_nuts_row(v, right ? PGL_NUTS_RR : PGL_NUTS_RL, r)[c] = rw[c];
            pgl_nuts_row(v, right ? PGL_NUTS_HR : PGL_NUTS_HL, r)[c] = hb[c];
            pgl_nuts_row(v, PGL_NUTS_RHO, r)[c] += rhos[c];
        }
        if (act & PGL_NUTS_TAKE_SUB) {
            pgl_nuts_row(v, PGL_NUTS_QC, r)[c] = pgl_nuts_row(v, PGL_NUTS_QS, r)[c];
            pgl_nuts_row(v, PGL_NUTS_GC, r)[c] = pgl_nuts_row(v, PGL_NUTS_GS, r)[c];
            pgl_nuts_row(v, PGL_NUTS_HC, r)[c] = pgl_nuts_row(v, PGL_NUTS_HS, r)[c];
        }
        if ((act & PGL_NUTS_END) && slot >= 0 && samples)
            samples[((size_t)slot * M + r) * P + c] = pgl_nuts_row(v, PGL_NUTS_QC, r)[c];
        if (ADAPT && sadapt) {
            double mean = a.mean[o + c], m2 = a.m2[o + c];
            pgl_adapt_welford(pgl_nuts_row(v, PGL_NUTS_QC, r)[c], sn, &mean, &m2);
            if (sadapt & PGL_ADAPT_SWITCH) {
                const double mi = pgl_adapt_minv(m2, sn);
                minv_out[o + c] = mi;
                pgl_nuts_row(v, PGL_NUTS_HC, r)[c] = sqrt(mi) * pgl_nuts_row(v, PGL_NUTS_GC, r)[c];
                mean = 0.0; m2 = 0.0;
            }
            a.mean[o + c] = mean; a.m2[o + c] = m2;
        }
        ks0 += pgl_nuts_advance_elem(v, r, c, act, sh.v, sh.ve, key, dense != 0, minv, Xt);
    }
    if (act & PGL_NUTS_END) {                                                  // (uniform over the workgroup)
        ks0 = pgl_blk_sum(ks0, red);
        if (tid == 0 && !(act & PGL_NUTS_DONE)) pgl_nuts_energy0(&sh, ks0);
    }
    if (tid == 0) pgl_nuts_store(v, r, &sh);
}

__global__ __launch_bounds__(256) void k_nuts_step(const NutsView v, double* __restrict__ ll, double* __restrict__ grad,
                                                   const BfgsPrior q, const int dense, const double* __restrict__ minv,
                                                   const double delta, const int n_warmup, const int thin, const int n_keep,
                                                   double* __restrict__ Xt, double* __restrict__ samples,
                                                   double* __restrict__ stats)
{
    AdaptView a;
    a.R = 0; a.P = 0; a.mean = a.m2 = a.count = a.widx = nullptr;
    pgl_nuts_step_row<0>(v, ll, grad, q, dense, minv, delta, n_warmup, thin, n_keep, Xt, samples, stats, a, nullptr, nullptr);
}
// the diagonal chain under mass='adapt': minv (M, P) is read and, at a row's window ends, rewritten
__global__ __launch_bounds__(256) void k_nuts_adapt_step(const NutsView v, double* __restrict__ ll, double* __restrict__ grad,
                                                         const BfgsPrior q, double* minv, const double delta,
                                                         const int n_warmup, const int thin, const int n_keep,
                                                         double* __restrict__ Xt, double* __restrict__ samples,
                                                         double* __restrict__ stats, const AdaptView a,
                                                         const int* __restrict__ sched)
{
    pgl_nuts_step_row<1>(v, ll, grad, q, 0, minv, delta, n_warmup, thin, n_keep, Xt, samples, stats, a, sched, minv);
}
