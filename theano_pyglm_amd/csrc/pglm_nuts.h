// The No-U-Turn sampler on one row (one neuron's parameter vector) as a reverse-communication state machine, in the style
// of pglm_hmc.h: the random numbers, the scalar decisions and the per-element updates, no loops over the row and no
// callbacks -- the caller (the k_nuts_* row kernels of pglm_nuts.hip.h, one workgroup per neuron; tests/csrc/nuts_host.c on
// the host) owns the vectors, computes the reductions and supplies ll and its gradient, ONE evaluation per leapfrog step.
// Rows do not wait for each other: a row that ends a transition starts the next one in the same call and counts its own t.
//
// Multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017, "A conceptual introduction to HMC", app. A) in the whitened
// momentum r = W^T p of pglm_hmc_dense.h, K = 1/2 sum_j r_j^2, the inverse mass matrix being W W^T (diagonal: W =
// diag(sqrt(minv))).  inference/nuts.py: nuts_transition states the same transition with the leaves kept in a list.
//   target        U, grad U, the priors and the non-finite rules of pglm_hmc.h.
//   leapfrog      from an edge (q, r, h), h = W^T grad U(q), in direction v = +-1:  r' = r - v eps/2 h;  q' = q + v eps W r';
//                 evaluate;  h' = W^T grad U(q');  r'' = r' - v eps/2 h'.  The leaf is (q', r'', h'), H = U(q') + K(r'').
//   tree          transition t draws r = z at the current point (leaf -1), H0 = U + K.  Doubling d = 0, 1, ...: a direction
//                 v_d, then a subtree of 2^d leaves i = 0 .. 2^d - 1 from the edge on that side.  A leaf is DIVERGENT if H is
//                 not finite or H - H0 > 1000: weight 0, counted, the subtree is discarded and the transition ends.  After
//                 leaf i (odd) every aligned block of 2^k leaves that ends at i (k = 1 .. number of trailing one bits of i;
//                 the whole subtree is the last of them) is tested:  rho . r_first > 0 and rho . r_last > 0, rho the sum
//                 of r over the block (Euclidean in these coordinates; symmetric in the direction).  A failure discards the
//                 subtree and ends the transition.  A complete subtree is merged: the candidate step below, the edge on
//                 side v becomes its last leaf, rho_tree += rho_subtree, and the same test on the whole tree (rho_tree,
//                 r_left, r_right); a failure ends the transition, as does d + 1 = max_depth.  No other cross checks.
//                 'depth' counts the doublings begun, a discarded one included.
//   storage       O(max_depth): an even leaf i stores (r_i, the subtree's rho BEFORE leaf i) in slot popcount(i); the
//                 block of 2^k leaves that ends at the odd leaf i starts at leaf i - 2^k + 1, slot popcount(i) - k, which
//                 no later even leaf has overwritten (they all have more bits set).
//   proposal      log weights lw = H0 - H.  In a subtree leaf i replaces the subtree's candidate iff i = 0 or
//                 log u < lw_i - log sum_{k <= i} w_k;  at a merge the subtree's candidate replaces the tree's iff
//                 log u < log w_subtree - log w_tree (w_tree before the merge; the start point has w = 1).
//   statistic     alpha = the mean over all leaves built in the transition, discarded ones included, of
//                 min(1, exp(H0 - H)); a divergent leaf gives 0.
//   step size     dual averaging (Hoffman & Gelman 2014, alg. 5) per row, m = t + 1 <= n_warmup:
//                 Hbar = (1 - 1/(m + t0)) Hbar + (delta - alpha)/(m + t0);  log eps = mu - sqrt(m)/gamma Hbar;
//                 log ebar = m^-kappa log eps + (1 - m^-kappa) log ebar;  gamma = 0.05, t0 = 10, kappa = 0.75,
//                 mu = log(10 step0);  eps = clip(exp(log eps), 1e-4, 10), and at m = n_warmup eps = clip(exp(log ebar)),
//                 frozen from then on.
//   random numbers  the key and uniforms of pglm_hmc.h, key = (seed, neuron, t):  z_j from counters 2 j + 1, 2 j + 2;
//                 direction of doubling d: counter 2 P + 1 + d (v = +1 iff u < 1/2);  merge uniform of doubling d:
//                 2 P + 17 + d;  selection uniform of leaf i of doubling d: 2 P + 33 + (2^d - 1 + i).
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_NUTS_H
#define PGLM_NUTS_H

#include "pglm_hmc.h"

#define PGL_NUTS_FN PGL_HMC_FN
#define PGL_NUTS_MAX_DEPTH 10
#define PGL_NUTS_GAMMA 0.05
#define PGL_NUTS_T0 10.0
#define PGL_NUTS_KAPPA 0.75
#define PGL_NUTS_MIN_STEP 1e-4
#define PGL_NUTS_MAX_STEP 10.0
#define PGL_NUTS_DIVERGE 1000.0

// The state of M rows of P parameters is ONE block of doubles: PGL_NUTS_NVEC + 2 max_depth (M, P) arrays -- the enum
// below, then the checkpoints r[0..max_depth), rho[0..max_depth) -- then PGL_NUTS_NSCAL (M) arrays, field-major, the
// fields of PglNuts in order.
enum { PGL_NUTS_QC = 0, PGL_NUTS_GC, PGL_NUTS_HC,          // the tree's candidate (the current point between transitions)
       PGL_NUTS_QL, PGL_NUTS_RL, PGL_NUTS_HL,              // left edge
       PGL_NUTS_QR, PGL_NUTS_RR, PGL_NUTS_HR,              // right edge
       PGL_NUTS_RHO,                                       // sum of r over the tree
       PGL_NUTS_QW, PGL_NUTS_RW,                           // the point under evaluation and the half-kicked momentum there
       PGL_NUTS_RHOS,                                      // sum of r over the running subtree
       PGL_NUTS_QS, PGL_NUTS_GS, PGL_NUTS_HS,              // the subtree's candidate
       PGL_NUTS_HB,                                        // W^T grad U at the point under evaluation (dense mass)
       PGL_NUTS_NVEC };
#define PGL_NUTS_NSCAL 30

enum { PGL_NUTS_STOP_SUB = 1, PGL_NUTS_STOP_TREE = 2, PGL_NUTS_STOP_DEPTH = 3, PGL_NUTS_STOP_DIVERGENT = 4 };
enum { PGL_NUTS_TAKE_LEAF = 1, PGL_NUTS_MERGE = 2, PGL_NUTS_TAKE_SUB = 4, PGL_NUTS_END = 8, PGL_NUTS_NEWSUB = 16,
       PGL_NUTS_CONT = 32, PGL_NUTS_DONE = 64 };

typedef struct {
    double Uc, H0;              // U at the tree's candidate, total energy at the start of the running transition
    double step, t;             // step size, completed transitions
    double neuron, seed_lo, seed_hi;
    double done;                // 1 after the row's last transition
    double depth, v, i;         // running transition: doublings begun, direction of the running subtree, its next leaf
    double lw_tree, lw_sub, Us; // log sum of weights of the tree and of the running subtree, U at the subtree's candidate
    double sum_acc, n_leaf;     // running transition: sum of min(1, exp(H0 - H)) and number of leaves
    double sel, sel_sub;        // leaf number (2^d - 1 + i; -1: the start point) of the tree's / the subtree's candidate
    double hbar, logeps_bar, mu;    // dual averaging
    double n_leapfrog, n_div, acc_post;     // totals: leapfrog steps; divergent transitions and sum of alpha with t >= n_warmup
    double last_depth, last_nleaf, last_stop, last_sel, last_acc;  // the last completed transition
    double ve;                  // v * step of the running subtree (0 once done)
} PglNuts;

PGL_NUTS_FN double pgl_nuts_uniform_dir(pgl_hmc_u64 key, int P, int d) { return pgl_hmc_uniform(key, 2 * (pgl_hmc_u64)P + 1 + d); }
PGL_NUTS_FN double pgl_nuts_uniform_merge(pgl_hmc_u64 key, int P, int d) { return pgl_hmc_uniform(key, 2 * (pgl_hmc_u64)P + 17 + d); }
PGL_NUTS_FN double pgl_nuts_uniform_leaf(pgl_hmc_u64 key, int P, int leafno)
{
    return pgl_hmc_uniform(key, 2 * (pgl_hmc_u64)P + 33 + (pgl_hmc_u64)leafno);
}
PGL_NUTS_FN pgl_hmc_u64 pgl_nuts_row_key(const PglNuts* s)
{
    const pgl_hmc_u64 seed = ((pgl_hmc_u64)s->seed_hi << 32) | (pgl_hmc_u64)s->seed_lo;
    return pgl_hmc_key(seed, (pgl_hmc_u64)s->neuron, (pgl_hmc_u64)s->t);
}
PGL_NUTS_FN double pgl_nuts_logaddexp(double a, double b)
{
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (!(lo > -(double)INFINITY)) return hi;
    return hi + log(1.0 + exp(lo - hi));
}
PGL_NUTS_FN double pgl_nuts_clip_step(double e)
{
    return e < PGL_NUTS_MIN_STEP ? PGL_NUTS_MIN_STEP : (e > PGL_NUTS_MAX_STEP ? PGL_NUTS_MAX_STEP : e);
}
PGL_NUTS_FN int pgl_nuts_trailing_ones(int i)
{
    int n = 0;
    while (i & 1) { ++n; i >>= 1; }
    return n;
}
PGL_NUTS_FN int pgl_nuts_popcount(int i)
{
    int n = 0;
    while (i) { n += i & 1; i >>= 1; }
    return n;
}

// ---- dynamics, per element ----
PGL_NUTS_FN double pgl_nuts_half_kick(double r, double ve, double h) { return r - 0.5 * ve * h; }
PGL_NUTS_FN double pgl_nuts_drift(double q, double ve, double wr) { return q + ve * wr; }      // wr = (W r)_j

// ---- the scalar state ----
// start of transition s->t (t < n_total), or the end of the chain: the caller draws r = z at the candidate, makes both
// edges (qc, z, hc), rho = z, and reports sum z^2 to pgl_nuts_energy0
PGL_NUTS_FN void pgl_nuts_start(PglNuts* s, int P, int n_total)
{
    s->depth = 1.0; s->i = 0.0;
    s->lw_tree = 0.0; s->lw_sub = -(double)INFINITY;
    s->sum_acc = 0.0; s->n_leaf = 0.0; s->sel = -1.0; s->sel_sub = -1.0;
    if (s->t >= (double)n_total) {
        s->done = 1.0; s->v = 0.0; s->ve = 0.0;
        return;
    }
    s->v = pgl_nuts_uniform_dir(pgl_nuts_row_key(s), P, 0) < 0.5 ? 1.0 : -1.0;
    s->ve = s->v * s->step;
}
PGL_NUTS_FN void pgl_nuts_energy0(PglNuts* s, double ksum) { s->H0 = s->Uc + 0.5 * ksum; }

PGL_NUTS_FN void pgl_nuts_init(PglNuts* s, int P, double U0, double step0, int neuron, pgl_hmc_u64 seed, int n_total)
{
    s->Uc = U0; s->H0 = U0; s->step = step0; s->t = 0.0;
    s->neuron = (double)neuron;
    s->seed_lo = (double)(seed & 0xffffffffULL); s->seed_hi = (double)(seed >> 32);
    s->done = 0.0; s->Us = U0;
    s->hbar = 0.0; s->logeps_bar = 0.0; s->mu = log(10.0 * step0);
    s->n_leapfrog = 0.0; s->n_div = 0.0; s->acc_post = 0.0;
    s->last_depth = 0.0; s->last_nleaf = 0.0; s->last_stop = 0.0; s->last_sel = -1.0; s->last_acc = 0.0;
    pgl_nuts_start(s, P, n_total);
}

// dual averaging after transition t with statistic alpha (t < n_warmup).  m0: the transitions completed when the dual
// averaging was last restarted (pglm_adapt.h restarts it at the end of a mass window; 0: never), so the iterate is
// m = t + 1 - m0; the averaged step is taken at t + 1 = n_warmup whatever m0.
PGL_NUTS_FN void pgl_nuts_adapt_from(PglNuts* s, double alpha, double delta, int n_warmup, double m0)
{
    const double m = s->t + 1.0 - m0;
    s->hbar = (1.0 - 1.0 / (m + PGL_NUTS_T0)) * s->hbar + (delta - alpha) / (m + PGL_NUTS_T0);
    const double le = s->mu - sqrt(m) / PGL_NUTS_GAMMA * s->hbar;
    const double eta = exp(-PGL_NUTS_KAPPA * log(m));
    s->logeps_bar = eta * le + (1.0 - eta) * s->logeps_bar;
    s->step = pgl_nuts_clip_step(exp(s->t + 1.0 == (double)n_warmup ? s->logeps_bar : le));
}
PGL_NUTS_FN void pgl_nuts_adapt(PglNuts* s, double alpha, double delta, int n_warmup)
{
    pgl_nuts_adapt_from(s, alpha, delta, n_warmup, 0.0);
}

// The leaf s->i of the running subtree is complete: U1 at it, ksum = sum r^2 of its momentum.  dots[2 (k - 1)], [2 (k - 1)
// + 1] = rho . r_first, rho . r_last of the block of 2^k leaves that ends at it, k = 1 .. trailing ones of i; dot_l, dot_r =
// (rho_tree + rho_subtree) . r_left, . r_right of the tree the merge would make (read only after the subtree's last leaf).
// Returns the action bits for the caller's vectors:
//   TAKE_LEAF  subtree candidate = the leaf            MERGE  edge on side v = the leaf, rho_tree += rho_subtree
//   TAKE_SUB   tree candidate = subtree candidate (after TAKE_LEAF)
//   CONT       next leaf from the leaf itself          NEWSUB  next subtree from the edge on side s->v (new), rho_subtree = 0
//   END        the transition ended, t += 1, *keep_slot = the row of the kept-sample tensor the candidate goes to or -1;
//              then a new transition starts (pgl_nuts_start) unless DONE.
// mg (host tests; null on the device): mg[0] = min over selection decisions of |log u - log ratio|, mg[1] = min over
// leaves of |H - H0 - 1000|; both only ever lowered.
// da_m0: pgl_nuts_adapt_from's m0 (pgl_nuts_leaf: 0).
PGL_NUTS_FN int pgl_nuts_leaf_from(PglNuts* s, int P, int max_depth, double U1, double ksum, const double* dots, double dot_l,
                                   double dot_r, double delta, int n_warmup, int thin, int n_keep, int* keep_slot, double* mg,
                                   double da_m0)
{
    const pgl_hmc_u64 key = pgl_nuts_row_key(s);
    const int d = (int)s->depth - 1, size = 1 << d, i = (int)s->i, leafno = size - 1 + i;
    const double H = U1 + 0.5 * ksum, dH = H - s->H0;
    const int div = !pgl_hmc_finite(H) || dH > PGL_NUTS_DIVERGE;
    int act = 0, stop = 0;
    s->sum_acc += div ? 0.0 : (dH <= 0.0 ? 1.0 : exp(-dH));
    s->n_leaf += 1.0;
    s->n_leapfrog += 1.0;
    if (mg && pgl_hmc_finite(H)) {
        const double m = pgl_ls_abs(dH - PGL_NUTS_DIVERGE);
        if (m < mg[1]) mg[1] = m;
    }
    if (div) stop = PGL_NUTS_STOP_DIVERGENT;
    else {
        const double lw = -dH;
        s->lw_sub = pgl_nuts_logaddexp(s->lw_sub, lw);
        int take = i == 0;
        if (!take) {
            const double lu = log(pgl_nuts_uniform_leaf(key, P, leafno)), lr = lw - s->lw_sub;
            take = lu < lr;
            if (mg && pgl_ls_abs(lu - lr) < mg[0]) mg[0] = pgl_ls_abs(lu - lr);
        }
        if (take) {
            s->Us = U1; s->sel_sub = (double)leafno;
            act |= PGL_NUTS_TAKE_LEAF;
        }
        const int nb = pgl_nuts_trailing_ones(i);
        for (int k = 0; k < nb; ++k)
            if (!(dots[2 * k] > 0.0 && dots[2 * k + 1] > 0.0)) stop = PGL_NUTS_STOP_SUB;
        if (stop) act = 0;
        else if (i == size - 1) {
            act |= PGL_NUTS_MERGE;
            const double lu = log(pgl_nuts_uniform_merge(key, P, d)), lr = s->lw_sub - s->lw_tree;
            if (mg && pgl_ls_abs(lu - lr) < mg[0]) mg[0] = pgl_ls_abs(lu - lr);
            if (lu < lr) {
                s->Uc = s->Us; s->sel = s->sel_sub;
                act |= PGL_NUTS_TAKE_SUB;
            }
            s->lw_tree = pgl_nuts_logaddexp(s->lw_tree, s->lw_sub);
            if (!(dot_l > 0.0 && dot_r > 0.0)) stop = PGL_NUTS_STOP_TREE;
            else if (d + 1 >= max_depth) stop = PGL_NUTS_STOP_DEPTH;
            else {
                s->depth += 1.0; s->i = 0.0;
                s->lw_sub = -(double)INFINITY; s->sel_sub = -1.0;
                s->v = pgl_nuts_uniform_dir(key, P, d + 1) < 0.5 ? 1.0 : -1.0;
                s->ve = s->v * s->step;
                act |= PGL_NUTS_NEWSUB;
            }
        } else {
            s->i += 1.0;
            act |= PGL_NUTS_CONT;
        }
    }
    if (!stop) return act;
    // ---- the transition ends ----
    const double alpha = s->sum_acc / s->n_leaf;
    s->last_depth = s->depth; s->last_nleaf = s->n_leaf; s->last_stop = (double)stop; s->last_sel = s->sel;
    s->last_acc = alpha;
    if (s->t < (double)n_warmup) pgl_nuts_adapt_from(s, alpha, delta, n_warmup, da_m0);
    else {
        s->acc_post += alpha;
        if (stop == PGL_NUTS_STOP_DIVERGENT) s->n_div += 1.0;
    }
    const int k = (int)s->t - n_warmup;
    *keep_slot = (k >= 0 && (k + 1) % thin == 0 && (k + 1) / thin <= n_keep) ? (k + 1) / thin - 1 : -1;
    s->t += 1.0;
    pgl_nuts_start(s, P, n_warmup + n_keep * thin);
    act |= PGL_NUTS_END | PGL_NUTS_NEWSUB;
    if (s->done != 0.0) act = (act & ~PGL_NUTS_NEWSUB) | PGL_NUTS_DONE;
    return act;
}
PGL_NUTS_FN int pgl_nuts_leaf(PglNuts* s, int P, int max_depth, double U1, double ksum, const double* dots, double dot_l,
                              double dot_r, double delta, int n_warmup, int thin, int n_keep, int* keep_slot, double* mg)
{
    return pgl_nuts_leaf_from(s, P, max_depth, U1, ksum, dots, dot_l, dot_r, delta, n_warmup, thin, n_keep, keep_slot, mg, 0.0);
}

#endif
