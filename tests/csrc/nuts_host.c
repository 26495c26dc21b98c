/* Host build of the product's NUTS row state machine (theano_pyglm_amd/csrc/pglm_nuts.h) for the CPU tests and as the
 * mirror of the device chain: M rows, driven by reverse communication the way the k_nuts_* row kernels drive it -- the
 * caller supplies ll and its gradient at the points Xt the machine asks for, one call per leapfrog step.  The state block
 * has the device's layout (pglm_nuts.h).  The inverse mass matrix of a row is W W^T: W (M, P, P) lower triangular, or
 * minv (M, P) (W = diag(sqrt(minv))), or neither (identity).  prior_kind < 0: no prior (ll is the whole log density).
 * Sums run in index order.  mg (M, 4): three margins, only ever lowered: the smallest margins of the row's decisions -- selection
 * |log u - log ratio|, divergence |H - H0 - 1000|, U-turn |rho . r| / (|rho| |r|) -- and mg[., 3], the number of leaves whose H was not finite (they
 * leave no divergence margin). */
#include "../../theano_pyglm_amd/csrc/pglm_nuts.h"
#include "../../theano_pyglm_amd/csrc/pglm_hmc_dense.h"

typedef struct {
    int kind, N, B, Dstim;
    double mu_b, sg_b, stim_sigma, mu, sigma, lam;
} Prior;

static void load(const double* sc, int M, int r, PglNuts* s)
{
    double* f = (double*)s;
    for (int k = 0; k < PGL_NUTS_NSCAL; ++k) f[k] = sc[(long)k * M + r];
}
static void store(double* sc, int M, int r, const PglNuts* s)
{
    const double* f = (const double*)s;
    for (int k = 0; k < PGL_NUTS_NSCAL; ++k) sc[(long)k * M + r] = f[k];
}

static double target(const Prior* q, int P, const double* x, double* g, double ll)
{
    double lp = 0.0;
    if (q->kind < 0) {
        for (int c = 0; c < P; ++c) g[c] = pgl_hmc_grad_elem(g[c], 0.0);
        return pgl_hmc_energy(ll, 0.0);
    }
    double d;
    lp += pgl_hmc_prior_bias(x[0], q->mu_b, q->sg_b, &d);
    g[0] = pgl_hmc_grad_elem(g[0], d);
    for (int c = 1; c < 1 + q->Dstim; ++c) {
        lp += pgl_hmc_prior_stim(x[c], q->stim_sigma, &d);
        g[c] = pgl_hmc_grad_elem(g[c], d);
    }
    const int o = 1 + q->Dstim;
    for (int n = 0; n < q->N; ++n)
        lp += pgl_hmc_prior_group(q->kind, x + o + n * q->B, q->B, q->mu, q->sigma, q->lam, g + o + n * q->B);
    return pgl_hmc_energy(ll, lp);
}

static Prior prior(int kind, int N, int B, int Dstim, const double* prm)
{
    Prior q = {kind, N, B, Dstim, prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
    return q;
}

/* y = W x (trans 0) or W^T x (trans 1) for one row */
static void apply(const double* W, const double* minv, int P, int trans, const double* x, double* y)
{
    for (int c = 0; c < P; ++c) {
        if (W) y[c] = trans ? pgl_hmcd_col_dot(W, P, c, x, 0, 1) : pgl_hmcd_row_dot(W, P, c, x, 0, 1);
        else y[c] = (minv ? sqrt(minv[c]) : 1.0) * x[c];
    }
}

#define VEC(k) (st + (long)(k) * MP + o)

/* fresh momentum at the candidate: both edges, rho, H0 */
static void draw(double* st, long MP, long o, int P, PglNuts* s)
{
    const pgl_hmc_u64 key = pgl_nuts_row_key(s);
    double ks = 0.0;
    for (int c = 0; c < P; ++c) {
        const double z = pgl_hmc_normal(key, (pgl_hmc_u64)c);
        VEC(PGL_NUTS_QL)[c] = VEC(PGL_NUTS_QR)[c] = VEC(PGL_NUTS_QC)[c];
        VEC(PGL_NUTS_HL)[c] = VEC(PGL_NUTS_HR)[c] = VEC(PGL_NUTS_HC)[c];
        VEC(PGL_NUTS_RL)[c] = VEC(PGL_NUTS_RR)[c] = VEC(PGL_NUTS_RHO)[c] = z;
        ks += z * z;
    }
    pgl_nuts_energy0(s, ks);
}

/* first leaf of a subtree from the edge on side s->v */
static void from_edge(double* st, long MP, long o, int P, const PglNuts* s)
{
    const int right = s->v > 0.0;
    const double *qe = VEC(right ? PGL_NUTS_QR : PGL_NUTS_QL), *re = VEC(right ? PGL_NUTS_RR : PGL_NUTS_RL),
                 *he = VEC(right ? PGL_NUTS_HR : PGL_NUTS_HL);
    for (int c = 0; c < P; ++c) {
        VEC(PGL_NUTS_RW)[c] = pgl_nuts_half_kick(re[c], s->ve, he[c]);
        VEC(PGL_NUTS_QW)[c] = qe[c];
        VEC(PGL_NUTS_RHOS)[c] = 0.0;
    }
}

/* qw += ve W rw -> Xt */
static void drift(double* st, long MP, long o, int P, const double* W, const double* minv, const PglNuts* s, double* Xt,
                  double* tmp)
{
    apply(W, minv, P, 0, VEC(PGL_NUTS_RW), tmp);
    for (int c = 0; c < P; ++c) Xt[c] = VEC(PGL_NUTS_QW)[c] = pgl_nuts_drift(VEC(PGL_NUTS_QW)[c], s->ve, tmp[c]);
}

long long nuts_state_doubles(int M, int P, int D)
{
    return (long long)M * P * (PGL_NUTS_NVEC + 2 * D) + (long long)M * PGL_NUTS_NSCAL;
}
int nuts_nscal(void) { return (int)(sizeof(PglNuts) / sizeof(double)); }
int nuts_nvec(void) { return PGL_NUTS_NVEC; }

/* prm: mu_b, sg_b, stim_sigma, mu, sigma, lam.  The rows' start points are in the QC array; (ll, grad) at them. */
void nuts_init(double* st, int M, int P, int D, int n_lo, double* ll, double* grad, int kind, int N, int B, int Dstim,
               const double* prm, const double* W, const double* minv, const double* step0, unsigned long long seed,
               int n_total, double* Xt, double* tmp)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double* sc = st + (long)(PGL_NUTS_NVEC + 2 * D) * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        const double* Wr = W ? W + (long)r * P * P : 0;
        const double* mr = minv ? minv + o : 0;
        const double U = target(&q, P, VEC(PGL_NUTS_QC), grad + o, ll[r]);
        for (int c = 0; c < P; ++c) VEC(PGL_NUTS_GC)[c] = grad[o + c];
        apply(Wr, mr, P, 1, grad + o, VEC(PGL_NUTS_HC));
        PglNuts s;
        pgl_nuts_init(&s, P, U, step0[r], n_lo + r, seed, n_total);
        if (s.done != 0.0) {
            for (int c = 0; c < P; ++c) Xt[o + c] = VEC(PGL_NUTS_QW)[c] = VEC(PGL_NUTS_QC)[c];
        } else {
            draw(st, MP, o, P, &s);
            from_edge(st, MP, o, P, &s);
            drift(st, MP, o, P, Wr, mr, &s, Xt + o, tmp);
        }
        store(sc, M, r, &s);
    }
}

/* one leapfrog step of every row that is not done, after ONE evaluation of all rows at Xt.  samples (n_keep, M, P);
 * stats (n_keep, 2, M): depth and leaves of the kept transitions; acts (M): the action bits of this call (0: idle) */
void nuts_step(double* st, int M, int P, int D, double* ll, double* grad, int kind, int N, int B, int Dstim,
               const double* prm, const double* W, const double* minv, double delta, int n_warmup, int thin, int n_keep,
               double* Xt, double* samples, double* stats, double* mg, int* acts, double* tmp)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double* sc = st + (long)(PGL_NUTS_NVEC + 2 * D) * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        const double* Wr = W ? W + (long)r * P * P : 0;
        const double* mr = minv ? minv + o : 0;
        PglNuts s;
        load(sc, M, r, &s);
        acts[r] = 0;
        if (s.done != 0.0) continue;
        double *qw = VEC(PGL_NUTS_QW), *rw = VEC(PGL_NUTS_RW), *hb = VEC(PGL_NUTS_HB), *rhos = VEC(PGL_NUTS_RHOS);
        double* g = grad + o;
        const double U1 = target(&q, P, qw, g, ll[r]);
        apply(Wr, mr, P, 1, g, hb);
        const int i = (int)s.i, size = 1 << ((int)s.depth - 1), right = s.v > 0.0;
        const int nb = pgl_nuts_trailing_ones(i), pc = pgl_nuts_popcount(i);
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            rw[c] = pgl_nuts_half_kick(rw[c], s.ve, hb[c]);                    /* the leaf's momentum */
            ks += rw[c] * rw[c];
            if (!(i & 1)) {
                VEC(PGL_NUTS_NVEC + pc)[c] = rw[c];
                VEC(PGL_NUTS_NVEC + D + pc)[c] = rhos[c];
            }
            rhos[c] += rw[c];
        }
        if (mg && !pgl_hmc_finite(U1 + 0.5 * ks)) mg[4 * r + 3] += 1.0;
        double dots[2 * PGL_NUTS_MAX_DEPTH], dot_l = 0.0, dot_r = 0.0;
        for (int k = 1; k <= nb; ++k) {
            const double *cr = VEC(PGL_NUTS_NVEC + pc - k), *crho = VEC(PGL_NUTS_NVEC + D + pc - k);
            double a = 0.0, b = 0.0, nr = 0.0, n1 = 0.0;
            for (int c = 0; c < P; ++c) {
                const double rb = rhos[c] - crho[c];
                a += rb * cr[c]; b += rb * rw[c];
                nr += rb * rb; n1 += cr[c] * cr[c];
            }
            dots[2 * (k - 1)] = a; dots[2 * (k - 1) + 1] = b;
            if (mg) {
                const double ma = pgl_ls_abs(a) / sqrt(nr * n1), mb = pgl_ls_abs(b) / sqrt(nr * ks);
                if (ma < mg[4 * r + 2]) mg[4 * r + 2] = ma;
                if (mb < mg[4 * r + 2]) mg[4 * r + 2] = mb;
            }
        }
        if (i == size - 1) {
            const double *el = right ? VEC(PGL_NUTS_RL) : rw, *er = right ? rw : VEC(PGL_NUTS_RR);
            double nr = 0.0, nl = 0.0, nn = 0.0;
            for (int c = 0; c < P; ++c) {
                const double rt = VEC(PGL_NUTS_RHO)[c] + rhos[c];
                dot_l += rt * el[c]; dot_r += rt * er[c];
                nr += rt * rt; nl += el[c] * el[c]; nn += er[c] * er[c];
            }
            /* (the margin counts only where the merge is reached: a discarded subtree never reads these) */
            int ok = pgl_hmc_finite(U1 + 0.5 * ks) && U1 + 0.5 * ks - s.H0 <= PGL_NUTS_DIVERGE;
            for (int k = 0; k < nb; ++k) ok = ok && dots[2 * k] > 0.0 && dots[2 * k + 1] > 0.0;
            if (mg && ok) {
                const double ma = pgl_ls_abs(dot_l) / sqrt(nr * nl), mb = pgl_ls_abs(dot_r) / sqrt(nr * nn);
                if (ma < mg[4 * r + 2]) mg[4 * r + 2] = ma;
                if (mb < mg[4 * r + 2]) mg[4 * r + 2] = mb;
            }
        }
        int slot = -1;
        const int act = pgl_nuts_leaf(&s, P, D, U1, ks, dots, dot_l, dot_r, delta, n_warmup, thin, n_keep, &slot,
                                      mg ? mg + 4 * r : 0);
        acts[r] = act;
        for (int c = 0; c < P; ++c) {
            if (act & PGL_NUTS_TAKE_LEAF) {
                VEC(PGL_NUTS_QS)[c] = qw[c]; VEC(PGL_NUTS_GS)[c] = g[c]; VEC(PGL_NUTS_HS)[c] = hb[c];
            }
            if (act & PGL_NUTS_MERGE) {
                VEC(right ? PGL_NUTS_QR : PGL_NUTS_QL)[c] = qw[c];
                VEC(right ? PGL_NUTS_RR : PGL_NUTS_RL)[c] = rw[c];
                VEC(right ? PGL_NUTS_HR : PGL_NUTS_HL)[c] = hb[c];
                VEC(PGL_NUTS_RHO)[c] += rhos[c];
            }
            if (act & PGL_NUTS_TAKE_SUB) {
                VEC(PGL_NUTS_QC)[c] = VEC(PGL_NUTS_QS)[c]; VEC(PGL_NUTS_GC)[c] = VEC(PGL_NUTS_GS)[c];
                VEC(PGL_NUTS_HC)[c] = VEC(PGL_NUTS_HS)[c];
            }
            if ((act & PGL_NUTS_END) && slot >= 0 && samples) samples[((long)slot * M + r) * P + c] = VEC(PGL_NUTS_QC)[c];
            if (act & PGL_NUTS_CONT) rw[c] = pgl_nuts_half_kick(rw[c], s.ve, hb[c]);
        }
        if ((act & PGL_NUTS_END) && slot >= 0 && stats) {
            stats[((long)slot * 2 + 0) * M + r] = s.last_depth;
            stats[((long)slot * 2 + 1) * M + r] = s.last_nleaf;
        }
        if (act & PGL_NUTS_DONE) {
            for (int c = 0; c < P; ++c) {
                Xt[o + c] = qw[c] = VEC(PGL_NUTS_QC)[c];
                rw[c] = 0.0;
            }
        } else {
            if (act & PGL_NUTS_END) draw(st, MP, o, P, &s);
            if (act & PGL_NUTS_NEWSUB) from_edge(st, MP, o, P, &s);
            drift(st, MP, o, P, Wr, mr, &s, Xt + o, tmp);
        }
        store(sc, M, r, &s);
    }
}

double nuts_uniform(unsigned long long seed, unsigned long long n, unsigned long long t, unsigned long long k)
{
    return pgl_hmc_uniform(pgl_hmc_key(seed, n, t), k);
}
double nuts_normal(unsigned long long seed, unsigned long long n, unsigned long long t, unsigned long long j)
{
    return pgl_hmc_normal(pgl_hmc_key(seed, n, t), j);
}
