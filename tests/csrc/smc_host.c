/* Host build of the product's adaptive sequential Monte Carlo state machine (theano_pyglm_amd/csrc/pglm_smc.h over
 * pglm_ais.h) for the CPU tests and as the mirror of the device run.  The rows are the AIS rows of ais_host.c (included:
 * ais_init and ais_start are used as they are); the per-neuron block has the device's layout (include/pyglm_hip.h):
 *   smc: (PGL_SMC_NSCAL, M) the fields of PglSmc, (PGL_SMC_NREC, S, M) records, (R) anc, (R) w, (R) acc, (1) n_active,
 *        (R, P), (R, P), (2, R) scratch.
 * The calls are pgl_smc_init_dev's second half / _stage_dev / _begin_dev / _leap_dev with host pointers.  Sums run in index
 * order. */
#include "../../theano_pyglm_amd/csrc/pglm_smc.h"
#include "ais_host.c"

typedef struct {
    int K, M, P, S;
    double *sc, *rec, *anc, *w, *acc, *nact, *tq, *tg, *ts;
} Smc;

static Smc smc_view(double* st, int K, int M, int P, int S)
{
    Smc v;
    const long R = (long)K * M;
    v.K = K; v.M = M; v.P = P; v.S = S;
    v.sc = st;
    v.rec = v.sc + (long)PGL_SMC_NSCAL * M;
    v.anc = v.rec + (long)PGL_SMC_NREC * S * M;
    v.w = v.anc + R; v.acc = v.w + R; v.nact = v.acc + R;
    v.tq = v.nact + 1; v.tg = v.tq + R * P; v.ts = v.tg + R * P;
    return v;
}
static void smc_load(const Smc* v, int i, PglSmc* s)
{
    double* f = (double*)s;
    for (int k = 0; k < PGL_SMC_NSCAL; ++k) f[k] = v->sc[(long)k * v->M + i];
}
static void smc_store(const Smc* v, int i, const PglSmc* s)
{
    const double* f = (const double*)s;
    for (int k = 0; k < PGL_SMC_NSCAL; ++k) v->sc[(long)k * v->M + i] = f[k];
}
static void smc_record(const Smc* v, int i, int stage, double beta, double ess, double cess, double rs, double step)
{
    if (stage >= v->S) return;
    const long SM = (long)v->S * v->M, o = (long)stage * v->M + i;
    v->rec[PGL_SMC_R_BETA * SM + o] = beta;
    v->rec[PGL_SMC_R_ESS * SM + o] = ess;
    v->rec[PGL_SMC_R_CESS * SM + o] = cess;
    v->rec[PGL_SMC_R_RS * SM + o] = rs;
    v->rec[PGL_SMC_R_ACC * SM + o] = (double)NAN;
    v->rec[PGL_SMC_R_STEP * SM + o] = step;
}

long long smc_state_doubles(int K, int M, int P, int S)
{
    const long long R = (long long)K * M;
    return (long long)PGL_SMC_NSCAL * M + (long long)PGL_SMC_NREC * S * M + 3 * R + 1 + 2 * R * P + 2 * R;
}
int smc_nscal(void) { return (int)(sizeof(PglSmc) / sizeof(double)); }
double smc_uniform(unsigned long long seed, unsigned long long neuron, unsigned long long stage)
{
    return pgl_smc_uniform(seed, neuron, stage);
}

void smc_init(double* smc, int K, int M, int P, int S, double step0)
{
    const Smc m = smc_view(smc, K, M, P, S);
    for (long e = 0; e < (long)PGL_SMC_NREC * S * M; ++e) m.rec[e] = (double)NAN;
    for (int i = 0; i < M; ++i) {
        PglSmc s;
        pgl_smc_init(&s, step0);
        smc_store(&m, i, &s);
        for (int k = 0; k < K; ++k) {
            const long r = (long)k * M + i;
            m.anc[r] = (double)k; m.w[r] = 1.0 / (double)K; m.acc[r] = 0.0;
        }
    }
    m.nact[0] = (double)M;
}

static void cess_sums(const Smc* m, const double* ll0, int i, double d, double ll_max, double* s1, double* s2)
{
    *s1 = 0.0; *s2 = 0.0;
    for (int k = 0; k < m->K; ++k) {
        const long r = (long)k * m->M + i;
        const double W = m->w[r];
        if (W > 0.0) {
            const double vv = pgl_smc_v(d, ll0[r], ll_max);
            *s1 += W * vv;
            *s2 += W * vv * vv;
        }
    }
}

/* steps 0 to 3 of one neuron; margins (2, M) or NULL: [0] min over k, j of |c_j - position_k| where the stage resampled
 * (else +inf), [1] |ESS - ess_min K| */
static void stage_neuron(double* st, const Smc* m, int i, int n_steps, double rho, double ess_min, double delta_min,
                         unsigned long long seed, double* margins)
{
    const int K = m->K, M = m->M, P = m->P;
    VIEW
    const double* ll0 = sc + 10L * R;
    double* logw = sc + 13L * R;
    PglSmc s;
    smc_load(m, i, &s);
    if (margins) { margins[i] = (double)INFINITY; margins[M + i] = (double)INFINITY; }
    if (s.done != 0.0) {
        s.live = 0.0; s.rs = 0.0;
        smc_store(m, i, &s);
        return;
    }
    const int stg = (int)s.stage;
    double a = 0.0;
    for (int k = 0; k < K; ++k) { a += m->acc[(long)k * M + i]; m->acc[(long)k * M + i] = 0.0; }
    s.acc = a;
    if (stg > 0) {
        const double rate = a / ((double)K * (double)n_steps);
        s.step = pgl_smc_step_rule(s.step, rate);
        if (stg - 1 < m->S) m->rec[((long)PGL_SMC_R_ACC * m->S + (stg - 1)) * M + i] = rate;
    }
    double mlw = -(double)INFINITY, mll = -(double)INFINITY;
    for (int k = 0; k < K; ++k) {
        const long r = (long)k * M + i;
        if (pgl_smc_alive(ll0[r], logw[r])) {
            if (logw[r] > mlw) mlw = logw[r];
            if (ll0[r] > mll) mll = ll0[r];
        }
    }
    double es = 0.0;
    for (int k = 0; k < K; ++k) {
        const long r = (long)k * M + i;
        m->w[r] = pgl_smc_alive(ll0[r], logw[r]) ? exp(logw[r] - mlw) : 0.0;
        es += m->w[r];
    }
    for (int k = 0; k < K; ++k) m->w[(long)k * M + i] = es > 0.0 ? m->w[(long)k * M + i] / es : 0.0;
    const double rem = 1.0 - s.beta, target = rho * (double)K;
    double s1 = 0.0, s2 = 0.0, d = rem, beta_new = 1.0;
    if (es > 0.0) {
        cess_sums(m, ll0, i, rem, mll, &s1, &s2);
        double lo = rem;
        if (!(pgl_smc_cess(K, s1, s2) >= target)) {
            double hi = rem;
            lo = 0.0;
            for (int it = 0; it < PGL_SMC_BISECT; ++it) {
                const double mid = 0.5 * (lo + hi);
                cess_sums(m, ll0, i, mid, mll, &s1, &s2);
                if (pgl_smc_cess(K, s1, s2) >= target) lo = mid;
                else hi = mid;
            }
        }
        d = pgl_smc_delta(lo, delta_min, s.beta, &beta_new);
        cess_sums(m, ll0, i, d, mll, &s1, &s2);
    }
    if (!(es > 0.0) || !(s1 > 0.0)) {
        for (int k = 0; k < K; ++k) {
            const long r = (long)k * M + i;
            logw[r] = -(double)INFINITY; m->w[r] = 0.0; m->anc[r] = (double)k;
        }
        s.log_Z = -(double)INFINITY;
        s.done = 1.0; s.live = 0.0; s.rs = 0.0; s.ess = 0.0;
        smc_record(m, i, stg, s.beta, 0.0, 0.0, 0.0, s.step);
        s.stage += 1.0;
        smc_store(m, i, &s);
        return;
    }
    const double cess = pgl_smc_cess(K, s1, s2), ls1 = log(s1), les = log(es);
    s.log_Z += d * mll + ls1;
    double q2 = 0.0;
    for (int k = 0; k < K; ++k) {
        const long r = (long)k * M + i;
        const double W = m->w[r];
        double Wn = 0.0, lw = -(double)INFINITY;
        if (W > 0.0) {
            Wn = W * pgl_smc_v(d, ll0[r], mll) / s1;
            lw = ((logw[r] - mlw) - les) + d * (ll0[r] - mll) - ls1;
        }
        m->w[r] = Wn;
        logw[r] = lw;
        q2 += Wn * Wn;
    }
    const double ess = 1.0 / q2;
    const int rs = ess < ess_min * (double)K;
    if (margins) margins[M + i] = pgl_ls_abs(ess - ess_min * (double)K);
    if (rs) {
        double* cum = m->ts + i;
        double c = 0.0;
        int last_live = 0;
        for (int k = 0; k < K; ++k) {
            const double W = m->w[(long)k * M + i];
            c += W;
            cum[(long)k * M] = c;
            if (W > 0.0) last_live = k;
        }
        const double u = pgl_smc_uniform(seed, (pgl_hmc_u64)sc[7L * R + i], (pgl_hmc_u64)stg);
        for (int k = 0; k < K; ++k) {
            const double pos = pgl_smc_position(u, k, K);
            int j = pgl_smc_search(cum, (long)M, K, pos);
            if (!(m->w[(long)j * M + i] > 0.0)) j = last_live;
            m->anc[(long)k * M + i] = (double)j;
            logw[(long)k * M + i] = 0.0;
            if (margins)
                for (int jj = 0; jj < K; ++jj) {
                    const double gap = pgl_ls_abs(cum[(long)jj * M] - pos);
                    if (jj < last_live && gap < margins[i]) margins[i] = gap;
                }
        }
    } else {
        for (int k = 0; k < K; ++k) m->anc[(long)k * M + i] = (double)k;
    }
    smc_record(m, i, stg, beta_new, ess, cess, (double)rs, s.step);
    s.beta = beta_new;
    s.stage += 1.0;
    s.done = beta_new == 1.0 ? 1.0 : 0.0;
    s.n_resampled += (double)rs;
    s.live = 1.0; s.rs = (double)rs; s.ess = ess;
    smc_store(m, i, &s);
}

/* the stage kernel alone */
void smc_stage_only(double* st, double* smc, int K, int M, int P, int S, int n_steps, double rho, double ess_min,
                    double delta_min, unsigned long long seed, double* margins)
{
    const Smc m = smc_view(smc, K, M, P, S);
    for (int i = 0; i < M; ++i) stage_neuron(st, &m, i, n_steps, rho, ess_min, delta_min, seed, margins);
}

/* gather through the scratch, then scatter and retemper; the count of unfinished neurons */
void smc_gather_retemper(double* st, double* smc, int K, int M, int P, int S, int N, int B, int Dstim, const double* prm)
{
    const Prior q = prior(N, B, Dstim, prm);
    const Smc m = smc_view(smc, K, M, P, S);
    VIEW
    for (int r = 0; r < R; ++r) {
        const int i = r % M;
        if (m.sc[(long)7 * M + i] == 0.0 || m.sc[(long)8 * M + i] == 0.0) continue;
        const long src = (long)m.anc[r] * M + i;
        for (int c = 0; c < P; ++c) {
            m.tq[(long)r * P + c] = Q[src * P + c];
            m.tg[(long)r * P + c] = GL[src * P + c];
        }
        m.ts[r] = sc[10L * R + src];
        m.ts[R + r] = sc[11L * R + src];
    }
    double na = 0.0;
    for (int i = 0; i < M; ++i) na += m.sc[(long)4 * M + i] == 0.0 ? 1.0 : 0.0;
    m.nact[0] = na;
    for (int r = 0; r < R; ++r) {
        const int i = r % M;
        const long o = (long)r * P;
        if (m.sc[(long)7 * M + i] == 0.0) continue;
        const int rs = m.sc[(long)8 * M + i] != 0.0;
        if (rs)
            for (int c = 0; c < P; ++c) { Q[o + c] = m.tq[o + c]; GL[o + c] = m.tg[o + c]; }
        const double beta = m.sc[i];
        target(&q, Q + o, GL + o, G + o, beta);
        PglAis s;
        load(sc, R, r, &s);
        if (rs) pgl_ais_keep(&s, m.ts[r], m.ts[R + r]);
        s.beta = beta;
        s.h.U0 = pgl_ais_energy(beta, s.ll0, s.lp0);
        s.h.step = m.sc[(long)2 * M + i];
        store(sc, R, r, &s);
    }
}

void smc_stage(double* st, double* smc, int K, int M, int P, int S, int N, int B, int Dstim, const double* prm, int n_steps,
               double rho, double ess_min, double delta_min, unsigned long long seed, double* margins)
{
    smc_stage_only(st, smc, K, M, P, S, n_steps, rho, ess_min, delta_min, seed, margins);
    smc_gather_retemper(st, smc, K, M, P, S, N, B, Dstim, prm);
}

/* the guarded moves: ais_begin / ais_leap (adapt = 0) for the rows of the neurons that are not done */
void smc_begin(double* st, double* smc, int K, int M, int P, int S, const double* minv, double* Xt)
{
    const Smc m = smc_view(smc, K, M, P, S);
    VIEW
    for (int r = 0; r < R; ++r) {
        const long o = (long)r * P, om = (long)(r % M) * P;
        if (m.sc[(long)4 * M + r % M] != 0.0) {
            for (int c = 0; c < P; ++c) Xt[o + c] = Q[o + c];
            continue;
        }
        PglAis s;
        load(sc, R, r, &s);
        const pgl_hmc_u64 key = pgl_hmc_row_key(&s.h);
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            const double mi = minv ? minv[om + c] : 1.0;
            double p = pgl_hmc_momentum(pgl_hmc_normal(key, (pgl_hmc_u64)c), mi);
            ks += pgl_hmc_kinetic_elem(p, mi);
            p = pgl_hmc_kick(p, 0.5, s.h.step, G[o + c]);
            Q0[o + c] = Q[o + c];
            Pm[o + c] = p;
            Q[o + c] = pgl_hmc_drift(Q[o + c], s.h.step, mi, p);
            Xt[o + c] = Q[o + c];
        }
        pgl_hmc_begin(&s.h, ks);
        store(sc, R, r, &s);
    }
}

void smc_leap(double* st, double* smc, int K, int M, int P, int S, const double* minv, const double* ll, const double* grad,
              int N, int B, int Dstim, const double* prm, int last, double* Xt, double* margin_out)
{
    const Prior q = prior(N, B, Dstim, prm);
    const Smc m = smc_view(smc, K, M, P, S);
    VIEW
    for (int r = 0; r < R; ++r) {
        const long o = (long)r * P, om = (long)(r % M) * P;
        if (m.sc[(long)4 * M + r % M] != 0.0) {
            if (!last)
                for (int c = 0; c < P; ++c) Xt[o + c] = Q[o + c];
            if (margin_out && last) margin_out[r] = (double)INFINITY;
            continue;
        }
        PglAis s;
        load(sc, R, r, &s);
        const double lp1 = target(&q, Q + o, grad + o, GU + o, s.beta);
        if (!last) {
            for (int c = 0; c < P; ++c) {
                const double mi = minv ? minv[om + c] : 1.0;
                Pm[o + c] = pgl_hmc_kick(Pm[o + c], 1.0, s.h.step, GU[o + c]);
                Q[o + c] = pgl_hmc_drift(Q[o + c], s.h.step, mi, Pm[o + c]);
                Xt[o + c] = Q[o + c];
            }
            continue;
        }
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            const double mi = minv ? minv[om + c] : 1.0;
            Pm[o + c] = pgl_hmc_kick(Pm[o + c], 0.5, s.h.step, GU[o + c]);
            ks += pgl_hmc_kinetic_elem(Pm[o + c], mi);
        }
        const double u = pgl_hmc_accept_uniform(pgl_hmc_row_key(&s.h));
        if (margin_out) margin_out[r] = pgl_ls_abs(log(u) - (s.h.H0 - (pgl_ais_energy(s.beta, ll[r], lp1) + 0.5 * ks)));
        const int acc = pgl_ais_decide(&s, ll[r], lp1, ks, u, 0);
        for (int c = 0; c < P; ++c) {
            if (acc) { G[o + c] = GU[o + c]; GL[o + c] = grad[o + c]; }
            else Q[o + c] = Q0[o + c];
        }
        m.acc[r] += (double)acc;
        store(sc, R, r, &s);
    }
}
