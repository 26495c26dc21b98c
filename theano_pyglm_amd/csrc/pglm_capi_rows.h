// ---- lock-step BFGS bookkeeping kernels (inference/batched_bfgs.py) ----------------------------------------------
long long pgl_bfgs_state_doubles(int M, int P) { return (long long)pgl_bfgs_doubles(M, P); }

// The one place where a pgl_prior is checked and becomes the kernels' BfgsPrior (N, B, Dstim from the handle).  The BFGS
// kernels take any basis width (any_B); pgl_bfgs_step_dev alone takes kind < 0 (final_ok): f and g arrive final, the prior
// is not read and the rows may be in any packing.
// (separable stimulus: the stimulus block of a row is [w_t, w_x], both under N(0, stim_sigma) -- bkgd.py:223-224 with mu = 0)
static_assert(sizeof(pgl_prior) == 56, "pgl_prior: an int and six doubles, as theano_pyglm_amd/_lib.py: Prior lays them out");
static int fill_prior(pgl_handle h, int P, const pgl_prior* prior, BfgsPrior& q, bool any_B = false, bool final_ok = false)
{
    if (!prior) return fail(PGL_ERR_ARG, "bad argument");
    if (final_ok && prior->kind > 1) return fail(PGL_ERR_ARG, "prior kind: 0 Gaussian, 1 group lasso, < 0: f and g arrive final");
    if (!(final_ok && prior->kind < 0)) {
        if (P != 1 + h->Dstim + h->Kimp) return fail(PGL_ERR_ARG, "rows must be theta rows [bias, w_stim, w_ir]");
        if (prior->kind != 0 && prior->kind != 1) return fail(PGL_ERR_ARG, "prior kind: 0 Gaussian, 1 group lasso");
    }
    if (!any_B && h->B > PGL_MAXB) return fail(PGL_ERR_UNSUPPORTED, "impulse basis too wide for the row kernels");
    q.N = h->N; q.B = h->B; q.Dstim = h->Dstim; q.kind = prior->kind;
    q.mu_b = prior->mu_b; q.sg_b = prior->sg_b; q.stim_sigma = prior->stim_sigma;
    q.mu = prior->mu; q.sigma = prior->sigma; q.lam = prior->lam;
    return PGL_OK;
}

int pgl_bfgs_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt)
{
    if (!h || !d_state || !d_Xt || M <= 0 || P <= 0 || L <= 0 || L > M) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_bfgs_trial, L, pgl_bfgs_view(d_state, M, P), d_rows, d_Xt);
}

int pgl_bfgs_objective_dev(pgl_handle h, int L, int P, const double* d_Xt, double* d_ll_f, double* d_grad_g,
                           const pgl_prior* prior)
{
    if (!h || !d_Xt || !d_ll_f || !d_grad_g || L <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_bfgs_objective, L, P, d_Xt, d_ll_f, d_grad_g, q);
}

int pgl_bfgs_init_dev(pgl_handle h, double* d_state, int M, int P, double gtol)
{
    if (!h || !d_state || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_bfgs_init, M, pgl_bfgs_view(d_state, M, P), gtol);
}

static BfgsStepArgs bfgs_step_args(int phases)
{
    BfgsStepArgs a;
    memset(&a, 0, sizeof(a));
    a.phases = phases;
    a.max_trials = 100;
    return a;
}

int pgl_bfgs_linesearch_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                            const double* d_f, const double* d_g, int max_trials)
{
    if (!h || !d_state || !d_Xt || !d_f || !d_g || M <= 0 || P <= 0 || L <= 0 || L > M || max_trials <= 0)
        return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    BfgsStepArgs a = bfgs_step_args(PGL_STEP_LS);            // f, g arrive final: no prior phase
    a.rows = d_rows; a.Xt = d_Xt; a.ft = const_cast<double*>(d_f); a.gt = const_cast<double*>(d_g);
    a.max_trials = max_trials;
    return launch_rows(h, k_bfgs_step<256>, L, pgl_bfgs_view(d_state, M, P), a);
}

int pgl_bfgs_hmul_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_H, int ld)
{
    if (!h || !d_state || !d_H || M <= 0 || P <= 0 || L <= 0 || L > M) return fail(PGL_ERR_ARG, "bad argument");
    if (ld < P || (ld & 1) || (reinterpret_cast<uintptr_t>(d_H) & 15))
        return fail(PGL_ERR_ARG, "H: leading dimension even and >= P, base 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    const unsigned bx = (unsigned)((P + 4 * PGL_HM_ROWS - 1) / (4 * PGL_HM_ROWS));
    hipLaunchKernelGGL(k_bfgs_hmul, dim3(bx, (unsigned)L), dim3(256), 0, h->stream, pgl_bfgs_view(d_state, M, P), d_rows,
                       d_H, ld);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_bfgs_hmul_hist_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_hist,
                           const double* d_coef, int Kmax, double* d_ab)
{
    if (!h || !d_state || !d_hist || !d_coef || !d_ab || M <= 0 || P <= 0 || L <= 0 || L > M || Kmax <= 0)
        return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const BfgsView v = pgl_bfgs_view(d_state, M, P);
    hipLaunchKernelGGL(k_bfgs_hdots, dim3((unsigned)((Kmax + 3) / 4), (unsigned)L), dim3(256), 0, h->stream, v, d_rows, d_hist,
                       d_coef, Kmax, d_ab);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bfgs_hcomb, dim3((unsigned)((P + 63) / 64), (unsigned)L), dim3(512), 0, h->stream, v, d_rows, d_hist, Kmax,
                       (const double*)d_ab);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_bfgs_update_dev(pgl_handle h, double* d_state, int M, int P, double gtol, int maxiter, int init_scaling, double* d_hist,
                        double* d_coef, int Kmax)
{
    if (!h || !d_state || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    if ((d_hist != nullptr) != (d_coef != nullptr) || (d_hist && Kmax < maxiter))
        return fail(PGL_ERR_ARG, "history buffers: both or none, room for maxiter updates");
    HIPCHK(hipSetDevice(h->device));
    BfgsStepArgs a = bfgs_step_args(PGL_STEP_UPDATE);        // every row of the shard, no trial points
    a.gtol = gtol; a.maxiter = maxiter; a.init_scaling = init_scaling; a.Wh = d_hist; a.cs = d_coef; a.Kmax = Kmax;
    return launch_rows(h, k_bfgs_step<256>, M, pgl_bfgs_view(d_state, M, P), a);
}

// the address the device uses for a buffer of pinned host memory that a row kernel writes its flags into (looked up once)
static int flags_device_pointer(pgl_handle h, double* flags_out, double** flags_dev)
{
    *flags_dev = nullptr;
    if (!flags_out) return PGL_OK;                             // (optional everywhere: no flags wanted)
    for (int i = 0; i < 4; ++i)
        if (h->flags_host[i] == flags_out) {
            *flags_dev = h->flags_dev[i];
            return PGL_OK;
        }
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, flags_out, 0) != hipSuccess || !dp) {
        (void)hipGetLastError();
        return fail(PGL_ERR_ARG, "flags_out must be pinned (page-locked, device-mapped) host memory");
    }
    *flags_dev = (double*)dp;
    h->flags_host[h->flags_next] = flags_out;
    h->flags_dev[h->flags_next] = *flags_dev;
    h->flags_next = (h->flags_next + 1) & 3;
    return PGL_OK;
}

// One whole iteration behind an evaluation (see k_bfgs_step): in ONE launch while the update history of a row is short
// (hk_bound * P numbers, PGL_OPT_BFGS_MERGE), else as line search | k_bfgs_hdots | k_bfgs_hcomb | update (dense inverse
// Hessians: line search | k_bfgs_hmul | update).
int pgl_bfgs_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt, double* d_ll_f,
                      double* d_grad_g, const pgl_prior* prior, int max_trials, double gtol, int maxiter, int init_scaling,
                      double* d_hist, double* d_coef, int Kmax, double* d_ab, int hk_bound, double* d_H, int ld,
                      const int* d_pos_next, double* d_Xt_next, double* flags_out)
{
    if (!h || !d_state || !d_Xt || !d_ll_f || !d_grad_g || M <= 0 || P <= 0 || L <= 0 || L > M || max_trials <= 0)
        return fail(PGL_ERR_ARG, "bad argument");
    BfgsStepArgs a = bfgs_step_args(0);
    int rc = fill_prior(h, P, prior, a.q, true, true);
    if (rc) return rc;
    if ((d_hist != nullptr) != (d_coef != nullptr) || (d_hist && (Kmax < maxiter || !d_ab)))
        return fail(PGL_ERR_ARG, "history buffers: all or none, room for maxiter updates");
    if ((d_hist != nullptr) == (d_H != nullptr)) return fail(PGL_ERR_ARG, "either the update history or dense inverse Hessians");
    if (d_H && (ld < P || (ld & 1) || (reinterpret_cast<uintptr_t>(d_H) & 15)))
        return fail(PGL_ERR_ARG, "H: leading dimension even and >= P, base 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    const BfgsView v = pgl_bfgs_view(d_state, M, P);
    a.rows = d_rows; a.Xt = d_Xt; a.ft = d_ll_f; a.gt = d_grad_g;
    a.have_prior = prior->kind >= 0 ? 1 : 0;
    a.max_trials = max_trials; a.gtol = gtol; a.maxiter = maxiter; a.init_scaling = init_scaling;
    a.Wh = d_hist; a.cs = d_coef; a.Kmax = Kmax; a.ab = d_ab;
    a.pos_next = d_pos_next; a.Xt_next = d_Xt_next; a.flags_out = flags_dev;
    const bool merged = d_hist && (long long)std::max(hk_bound, 0) * P <= (long long)h->opt_bfgs_merge;
    if (merged) {
        a.phases = PGL_STEP_LS | PGL_STEP_HIST | PGL_STEP_UPDATE;
        hipLaunchKernelGGL(k_bfgs_step<1024>, dim3(L), dim3(1024), 0, h->stream, v, a);
        HIPCHK(hipGetLastError());
        return PGL_OK;
    }
    a.phases = PGL_STEP_LS;
    rc = launch_rows(h, k_bfgs_step<256>, L, v, a);
    if (rc) return rc;
    if (d_hist) {
        const int Kb = std::min(Kmax, std::max(hk_bound, 1));       // no row holds more than hk_bound updates
        hipLaunchKernelGGL(k_bfgs_hdots, dim3((unsigned)((Kb + 3) / 4), (unsigned)L), dim3(256), 0, h->stream, v, d_rows,
                           (const double*)d_hist, (const double*)d_coef, Kmax, d_ab);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_bfgs_hcomb, dim3((unsigned)((P + 63) / 64), (unsigned)L), dim3(512), 0, h->stream, v, d_rows,
                           (const double*)d_hist, Kmax, (const double*)d_ab);
        HIPCHK(hipGetLastError());
    } else {
        const unsigned bx = (unsigned)((P + 4 * PGL_HM_ROWS - 1) / (4 * PGL_HM_ROWS));
        hipLaunchKernelGGL(k_bfgs_hmul, dim3(bx, (unsigned)L), dim3(256), 0, h->stream, v, d_rows, d_H, ld);
        HIPCHK(hipGetLastError());
    }
    a.phases = PGL_STEP_UPDATE;
    return launch_rows(h, k_bfgs_step<256>, L, v, a);
}

// ---- lock-step Newton-CG row kernels (inference/batched_newton_cg.py) --------------------------------------------------
long long pgl_ncg_state_doubles(int M, int P) { return (long long)pgl_ncg_doubles(M, P); }

int pgl_ncg_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                     int maxiter, double* d_V, double* flags_out)
{
    if (!h || !d_state || !d_ll || !d_grad || !d_V || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    return launch_rows(h, k_ncg_init, M, pgl_ncg_view(d_state, M, P), d_ll, d_grad, q, maxiter, d_V, flags_dev);
}

int pgl_ncg_cg_step_dev(pgl_handle h, double* d_state, int M, int P, double* d_hv, const pgl_prior* prior, double* d_V,
                        double* flags_out)
{
    if (!h || !d_state || !d_hv || !d_V || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    return launch_rows(h, k_ncg_cg_step, M, pgl_ncg_view(d_state, M, P), d_hv, q, d_V, flags_dev);
}

// what both optimisers' trial and search-step launches check and fill (pglm_rowsearch.hip.h)
static int row_trial(pgl_handle h, const double* X, const double* d, const double* sc, int f_alpha, int f_phase, int M, int P,
                     const int* d_rows, int L, double* d_Xt)
{
    if (!h || !X || !d_Xt || M <= 0 || P <= 0 || L <= 0 || L > M) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_row_trial, L, X, d, sc + (size_t)f_alpha * M, sc + (size_t)f_phase * M, P, d_rows, d_Xt);
}

static int row_search_args(pgl_handle h, const double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                           double* d_ll_f, double* d_grad_g, const pgl_prior* prior, int maxiter, const int* d_pos_next,
                           double* d_Xt_next, double* flags_out, RowSearchArgs& a)
{
    if (!h || !d_state || !d_Xt || !d_ll_f || !d_grad_g || M <= 0 || P <= 0 || L <= 0 || L > M)
        return fail(PGL_ERR_ARG, "bad argument");
    if (d_Xt_next == d_Xt) return fail(PGL_ERR_ARG, "the next trial points need a buffer of their own");
    memset(&a, 0, sizeof(a));
    int rc = fill_prior(h, P, prior, a.q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (flags_device_pointer(h, flags_out, &a.flags)) return PGL_ERR_ARG;
    a.rows = d_rows; a.Xt = d_Xt; a.ft = d_ll_f; a.gt = d_grad_g; a.maxiter = maxiter;
    a.pos_next = d_pos_next; a.Xt_next = d_Xt_next;
    return PGL_OK;
}

int pgl_ncg_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt)
{
    const NcgView v = pgl_ncg_view(d_state, M, P);
    return row_trial(h, d_state, v.xs, v.sc, PGL_NCG_F_ALPHA, PGL_NCG_F_PHASE, M, P, d_rows, L, d_Xt);
}

int pgl_ncg_search_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                            double* d_ll_f, double* d_grad_g, const pgl_prior* prior, int maxiter, const int* d_pos_next,
                            double* d_Xt_next, double* d_V, double* flags_out)
{
    if (!d_V) return fail(PGL_ERR_ARG, "bad argument");
    RowSearchArgs a;
    int rc = row_search_args(h, d_state, M, P, d_rows, L, d_Xt, d_ll_f, d_grad_g, prior, maxiter, d_pos_next, d_Xt_next,
                             flags_out, a);
    if (rc) return rc;
    a.V = d_V;
    return launch_rows(h, k_ncg_search_step, L, pgl_ncg_view(d_state, M, P), a);
}

// ---- lock-step HMC row kernels (inference/batched_hmc.py) --------------------------------------------------------------
long long pgl_hmc_state_doubles(int M, int P) { return (long long)pgl_hmc_doubles(M, P); }

// R = C M rows: chain c of neuron n_lo + m is row c M + m and runs on pgl_chain_seed(seed, c)
int pgl_hmc_init_dev(pgl_handle h, double* d_state, int M, int C, int P, int n_lo, double* d_ll, double* d_grad,
                     const pgl_prior* prior, double step0, uint64_t seed)
{
    if (!h || !d_state || !d_ll || !d_grad || M <= 0 || C <= 0 || P <= 0 || n_lo < 0 || n_lo + M > h->N || !(step0 > 0.0) ||
        (long long)M * C > 0x7fffffffLL)
        return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_hmc_init, M * C, pgl_hmc_view(d_state, M * C, P), d_ll, d_grad, q, n_lo, step0, seed, M);
}

// ---- windowed diagonal mass adaptation (mass='adapt'; pglm_adapt.h) ---------------------------------------------------
long long pgl_adapt_state_doubles(int R, int P)
{
    if (R <= 0 || P <= 0) return 0;
    return (long long)pgl_adapt_doubles(R, P);
}

int pgl_mass_adapt_dev(pgl_handle h, double* d_state, int R, int P, double* d_adapt, const int* d_sched, double* d_minv)
{
    if (!h || !d_state || !d_adapt || !d_sched || !d_minv || R <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_hmc_mass_adapt, R, pgl_hmc_view(d_state, R, P), pgl_adapt_view(d_adapt, R, P), d_sched, d_minv);
}

int pgl_hmc_begin_dev(pgl_handle h, double* d_state, int M, int P, const double* d_minv, double* d_Xt)
{
    if (!h || !d_state || !d_Xt || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_hmc_begin, M, pgl_hmc_view(d_state, M, P), d_minv, M, d_Xt);
}

int pgl_hmc_leap_dev(pgl_handle h, double* d_state, int M, int P, const double* d_minv, double* d_ll, double* d_grad,
                     const pgl_prior* prior, int last, int n_warmup, double* d_Xt, double* d_sample_out)
{
    if (!h || !d_state || !d_ll || !d_grad || !d_Xt || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_hmc_leap, M, pgl_hmc_view(d_state, M, P), d_minv, d_ll, d_grad, q, last ? 1 : 0, n_warmup, d_Xt,
                       d_sample_out);
}

// ---- lock-step HMC with a dense mass matrix (inference/batched_hmc.py: mass = (M, P, P) or 'laplace_dense') -------------
// The kick and the drift are epilogues of the products (pglm_hmc_dense.hip.h): no product is ever stored, no workspace.

// The four (TRANS, EPI) instantiations of a product kernel that the chains and pgl_tri_matvec*_dev use: LAUNCH(TRANS, EPI, KC)
// for the one that (trans, epi) names.
#define PGL_TRI_DISPATCH(LAUNCH, KC)                                           \
    do {                                                                       \
        if (epi == PGL_TRI_KICK) LAUNCH(1, PGL_TRI_KICK, KC);                  \
        else if (epi == PGL_TRI_DRIFT) LAUNCH(0, PGL_TRI_DRIFT, KC);           \
        else if (trans) LAUNCH(1, PGL_TRI_STORE, KC);                          \
        else LAUNCH(0, PGL_TRI_STORE, KC);                                     \
    } while (0)

// one product launch, one vector per matrix (the chain, NUTS, pgl_tri_matvec_dev)
static int tri_launch(pgl_handle h, int trans, int epi, const double* d_W, int M, int P, const double* d_x, double* d_y,
                      double* d_Xt, const double* d_step, double scale)
{
    if (M > 65535) return fail(PGL_ERR_ARG, "at most 65535 rows per call");
    const dim3 grid(h->opt_tri_rows ? 1 : (P + PGL_TRI_TILE - 1) / PGL_TRI_TILE, M);
#define PGL_TRI_LAUNCH(T, E, KC) hipLaunchKernelGGL((k_tri_matvec<T, E>), grid, dim3(256), 0, h->stream, d_W, d_x, P, d_y, d_Xt, d_step, scale)
    PGL_TRI_DISPATCH(PGL_TRI_LAUNCH, 1);
#undef PGL_TRI_LAUNCH
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_tri_matvec_dev(pgl_handle h, const double* d_W, int M, int P, int trans, const double* d_x, double* d_y)
{
    if (!h || !d_W || !d_x || !d_y || d_x == d_y || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return tri_launch(h, trans, PGL_TRI_STORE, d_W, M, P, d_x, d_y, nullptr, nullptr, 0.0);
}

// ---- batched dense factorisation for the Laplace posterior (pglm_chol.hip.h) ------------------------------------------
int pgl_chol_factor_dev(pgl_handle h, double* d_A, int M, int P, int ld, double* d_scale, double* d_logdet, int* d_info)
{
    if (!h || !d_A || !d_scale || !d_logdet || !d_info || M <= 0 || P <= 0 || ld < P) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_chol_factor, M, d_A, P, ld, d_scale, d_logdet, d_info);
}

int pgl_tri_inverse_dev(pgl_handle h, double* d_L, int M, int P, int ld, const int* d_info)
{
    if (!h || !d_L || !d_info || M <= 0 || P <= 0 || ld < P) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_tri_inverse, M, d_L, P, ld, d_info);
}

int pgl_chol_solve_dev(pgl_handle h, const double* d_Ls, int M, int P, int ld, const double* d_scale, const int* d_info,
                       const double* d_b, double* d_x)
{
    if (!h || !d_Ls || !d_scale || !d_info || !d_b || !d_x || M <= 0 || P <= 0 || ld < P) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_chol_solve, M, d_Ls, P, ld, d_scale, d_info, d_b, d_x);
}

// ---- lock-step dense Newton row kernels (inference/batched_newton.py) --------------------------------------------------
long long pgl_newton_state_doubles(int M, int P) { return (long long)pgl_newton_doubles(M, P); }

int pgl_newton_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                        double gtol, int maxiter, double* flags_out)
{
    if (!h || !d_state || !d_ll || !d_grad || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    return launch_rows(h, k_newton_init, M, pgl_newton_view(d_state, M, P), d_ll, d_grad, q, gtol, maxiter, flags_dev);
}

int pgl_newton_assemble_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_H, int ld,
                            const pgl_prior* prior, double* d_rhs)
{
    if (!h || !d_state || !d_H || M <= 0 || P <= 0 || L <= 0 || L > M || ld < P) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_newton_assemble, L, pgl_newton_view(d_state, M, P), d_rows, d_H, ld, q, d_rhs);
}

int pgl_newton_direction_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const int* d_info,
                             const double* d_p, double* flags_out)
{
    if (!h || !d_state || !d_info || !d_p || M <= 0 || P <= 0 || L <= 0 || L > M) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    return launch_rows(h, k_newton_direction, L, pgl_newton_view(d_state, M, P), d_rows, d_info, d_p, flags_dev);
}

int pgl_newton_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt)
{
    const NewtonView v = pgl_newton_view(d_state, M, P);
    return row_trial(h, d_state, v.p, v.sc, PGL_NEWTON_F_ALPHA, PGL_NEWTON_F_PHASE, M, P, d_rows, L, d_Xt);
}

int pgl_newton_search_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                               double* d_ll_f, double* d_grad_g, const pgl_prior* prior, double gtol, int maxiter,
                               const int* d_pos_next, double* d_Xt_next, double* flags_out)
{
    RowSearchArgs a;
    int rc = row_search_args(h, d_state, M, P, d_rows, L, d_Xt, d_ll_f, d_grad_g, prior, maxiter, d_pos_next, d_Xt_next,
                             flags_out, a);
    if (rc) return rc;
    a.gtol = gtol;
    return launch_rows(h, k_newton_search_step, L, pgl_newton_view(d_state, M, P), a);
}

int pgl_hmc_dense_begin_dev(pgl_handle h, double* d_state, int M, int P, const double* d_W, double* d_Xt)
{
    if (!h || !d_state || !d_W || !d_Xt || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const HmcView v = pgl_hmc_view(d_state, M, P);
    int rc = launch_rows(h, k_hmc_dense_draw, M, v);
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * M;
    rc = tri_launch(h, 1, PGL_TRI_KICK, d_W, M, P, v.g, v.p, nullptr, step, 0.5);
    if (rc) return rc;
    return tri_launch(h, 0, PGL_TRI_DRIFT, d_W, M, P, v.p, v.q, d_Xt, step, 1.0);
}

int pgl_hmc_dense_leap_dev(pgl_handle h, double* d_state, int M, int P, const double* d_W, double* d_ll, double* d_grad,
                           const pgl_prior* prior, int last, int n_warmup, double* d_Xt, double* d_sample_out)
{
    if (!h || !d_state || !d_W || !d_ll || !d_grad || !d_Xt || M <= 0 || P <= 0) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const HmcView v = pgl_hmc_view(d_state, M, P);
    rc = launch_rows(h, k_hmc_dense_target, M, v, d_ll, d_grad, q);
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * M;
    rc = tri_launch(h, 1, PGL_TRI_KICK, d_W, M, P, d_grad, v.p, nullptr, step, last ? 0.5 : 1.0);
    if (rc) return rc;
    if (!last) return tri_launch(h, 0, PGL_TRI_DRIFT, d_W, M, P, v.p, v.q, d_Xt, step, 1.0);
    return launch_rows(h, k_hmc_dense_end, M, v, d_ll, d_grad, n_warmup, d_sample_out);
}

// ---- NUTS row kernels (inference/batched_nuts.py) ------------------------------------------------------------------------
long long pgl_nuts_state_doubles(int M, int P, int max_depth)
{
    if (M <= 0 || P <= 0 || max_depth < 1 || max_depth > PGL_NUTS_MAX_DEPTH) return 0;
    return (long long)pgl_nuts_doubles(M, P, max_depth);
}

static int nuts_args(pgl_handle h, const double* d_state, int M, int P, int max_depth, const double* d_ll, const double* d_grad,
                     int n_warmup, int thin, int n_keep, const double* d_Xt)
{
    if (!h || !d_state || !d_ll || !d_grad || !d_Xt || M <= 0 || P <= 0 || n_warmup < 0 || thin <= 0 || n_keep < 0 ||
        (long long)n_warmup + (long long)n_keep * thin > 0x7fffffffLL)
        return fail(PGL_ERR_ARG, "bad argument");
    if (max_depth < 1 || max_depth > PGL_NUTS_MAX_DEPTH) return fail(PGL_ERR_ARG, "max_depth: 1 .. 10");
    return PGL_OK;
}

// d_minv, d_W: (C M0, P) / (C M0, P, P), one per row
int pgl_nuts_init_dev(pgl_handle h, double* d_state, int M0, int C, int P, int max_depth, int n_lo, double* d_ll,
                      double* d_grad, const pgl_prior* prior, const double* d_minv, const double* d_W, const double* d_step0,
                      uint64_t seed, int n_warmup, int thin, int n_keep, double* d_Xt)
{
    if (M0 <= 0 || C <= 0 || (long long)M0 * C > 0x7fffffffLL) return fail(PGL_ERR_ARG, "bad argument");
    const int M = M0 * C;                                                      // rows: chain c of neuron n_lo + m is row c M0 + m
    int rc = nuts_args(h, d_state, M, P, max_depth, d_ll, d_grad, n_warmup, thin, n_keep, d_Xt);
    if (rc) return rc;
    if (!d_step0 || n_lo < 0 || n_lo + M0 > h->N) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const NutsView v = pgl_nuts_view(d_state, M, P, max_depth);
    const size_t MP = (size_t)M * P;
    if (d_W) {
        rc = launch_rows(h, k_nuts_target, M, v, (int)PGL_NUTS_QC, d_ll, d_grad, q);
        if (rc) return rc;
        rc = tri_launch(h, 1, PGL_TRI_STORE, d_W, M, P, d_grad, v.vec + PGL_NUTS_HB * MP, nullptr, nullptr, 0.0);
        if (rc) return rc;
    }
    rc = launch_rows(h, k_nuts_init, M, v, d_ll, d_grad, q, d_W ? 1 : 0, d_minv, n_lo, d_step0, seed,
                     n_warmup + n_keep * thin, d_Xt, M0);
    if (rc || !d_W) return rc;
    return tri_launch(h, 0, PGL_TRI_DRIFT, d_W, M, P, v.vec + PGL_NUTS_RW * MP, v.vec + PGL_NUTS_QW * MP, d_Xt,
                      v.sc + (size_t)PGL_NUTS_F_VE * M, 1.0);
}

int pgl_nuts_step_dev(pgl_handle h, double* d_state, int M, int P, int max_depth, double* d_ll, double* d_grad,
                      const pgl_prior* prior, const double* d_minv, const double* d_W, double target_accept, int n_warmup,
                      int thin, int n_keep, double* d_Xt, double* d_samples, double* d_stats)
{
    int rc = nuts_args(h, d_state, M, P, max_depth, d_ll, d_grad, n_warmup, thin, n_keep, d_Xt);
    if (rc) return rc;
    if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(PGL_ERR_ARG, "target_accept: in (0, 1)");
    BfgsPrior q;
    rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const NutsView v = pgl_nuts_view(d_state, M, P, max_depth);
    const size_t MP = (size_t)M * P;
    if (d_W) {
        rc = launch_rows(h, k_nuts_target, M, v, (int)PGL_NUTS_QW, d_ll, d_grad, q);
        if (rc) return rc;
        rc = tri_launch(h, 1, PGL_TRI_STORE, d_W, M, P, d_grad, v.vec + PGL_NUTS_HB * MP, nullptr, nullptr, 0.0);
        if (rc) return rc;
    }
    rc = launch_rows(h, k_nuts_step, M, v, d_ll, d_grad, q, d_W ? 1 : 0, d_minv, target_accept, n_warmup, thin, n_keep, d_Xt,
                     d_samples, d_stats);
    if (rc || !d_W) return rc;
    return tri_launch(h, 0, PGL_TRI_DRIFT, d_W, M, P, v.vec + PGL_NUTS_RW * MP, v.vec + PGL_NUTS_QW * MP, d_Xt,
                      v.sc + (size_t)PGL_NUTS_F_VE * M, 1.0);
}

// pgl_nuts_step_dev for the diagonal chain under mass='adapt': d_minv (M, P) is read and, at a row's window ends, rewritten
int pgl_nuts_adapt_step_dev(pgl_handle h, double* d_state, int M, int P, int max_depth, double* d_ll, double* d_grad,
                            const pgl_prior* prior, double* d_minv, double* d_adapt, const int* d_sched, double target_accept,
                            int n_warmup, int thin, int n_keep, double* d_Xt, double* d_samples, double* d_stats)
{
    int rc = nuts_args(h, d_state, M, P, max_depth, d_ll, d_grad, n_warmup, thin, n_keep, d_Xt);
    if (rc) return rc;
    if (!d_minv || !d_adapt || !d_sched) return fail(PGL_ERR_ARG, "bad argument");
    if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(PGL_ERR_ARG, "target_accept: in (0, 1)");
    BfgsPrior q;
    rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_nuts_adapt_step, M, pgl_nuts_view(d_state, M, P, max_depth), d_ll, d_grad, q, d_minv,
                       target_accept, n_warmup, thin, n_keep, d_Xt, d_samples, d_stats, pgl_adapt_view(d_adapt, M, P), d_sched);
}

// ---- annealed importance sampling row kernels (inference/batched_ais.py) -----------------------------------------------
long long pgl_ais_state_doubles(int R, int P) { return (long long)pgl_ais_doubles((size_t)(R > 0 ? R : 0), (size_t)(P > 0 ? P : 0)); }

static int ais_prior(pgl_handle h, int K, int M, int P, const pgl_prior* prior, BfgsPrior& q)
{
    if (!prior || K <= 0 || M <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL) return fail(PGL_ERR_ARG, "bad argument");
    if (prior->kind == 1)
        return fail(PGL_ERR_UNSUPPORTED, "annealed importance sampling starts from an exact prior draw: Gaussian priors only");
    int rc = fill_prior(h, P, prior, q);
    if (rc) return rc;
    if (!(q.sg_b > 0.0) || !(q.sigma > 0.0) || (h->Dstim > 0 && !(q.stim_sigma > 0.0)))
        return fail(PGL_ERR_ARG, "the prior standard deviations must be positive");
    return PGL_OK;
}

int pgl_ais_init_dev(pgl_handle h, double* d_state, int K, int M, int P, int n_lo, int particle0, const pgl_prior* prior,
                     double step0, uint64_t seed, double* d_Xt)
{
    if (!h || !d_state || !d_Xt || n_lo < 0 || M <= 0 || n_lo + M > h->N || particle0 < -1 || !(step0 > 0.0))
        return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_ais_init, K * M, pgl_ais_view(d_state, K, M, P), d_Xt, q, n_lo, particle0, step0, seed);
}

int pgl_ais_start_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_ll, const double* d_grad,
                      const pgl_prior* prior)
{
    if (!h || !d_state || !d_ll || !d_grad) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_ais_start, K * M, pgl_ais_view(d_state, K, M, P), d_ll, d_grad, q);
}

int pgl_ais_temper_dev(pgl_handle h, double* d_state, int K, int M, int P, const pgl_prior* prior, double beta,
                       const double* d_step_row)
{
    if (!h || !d_state || !(beta >= 0.0 && beta <= 1.0)) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_ais_temper, K * M, pgl_ais_view(d_state, K, M, P), q, beta, d_step_row);
}

int pgl_ais_begin_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_minv, double* d_Xt)
{
    if (!h || !d_state || !d_Xt || K <= 0 || M <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL)
        return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_hmc_begin, K * M, pgl_ais_hmc_view(pgl_ais_view(d_state, K, M, P)), d_minv, M, d_Xt);
}

int pgl_ais_leap_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_minv, const double* d_ll,
                     const double* d_grad, const pgl_prior* prior, int last, int adapt, double* d_Xt, double* d_acc_out,
                     double* d_step_out)
{
    if (!h || !d_state || !d_ll || !d_grad || !d_Xt) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return launch_rows(h, k_ais_leap, K * M, pgl_ais_view(d_state, K, M, P), d_minv, d_ll, d_grad, q, last ? 1 : 0,
                       adapt ? 1 : 0, d_Xt, d_acc_out, d_step_out);
}

// ---- annealed importance sampling with a dense mass matrix (inference/batched_ais.py: mass = (M, P, P) or 'laplace_dense') ---
// one shared product launch: the particles of a neuron meet the neuron's W in one workgroup, KC at a time
// (d_done: the guarded form of the sequential Monte Carlo moves, one flag per neuron; null: the plain kernel.  Two
// instantiations per (TRANS, EPI, KC), chosen here, rather than one kernel with a nullable flag pointer: the plain kernel keeps
// the registers and the bits it had before the guard existed, at the price of a second copy in the code object.)
static int tri_shared_launch(pgl_handle h, int trans, int epi, const double* d_W, int K, int M, int P, const double* d_x,
                             double* d_y, double* d_Xt, const double* d_step, double scale, const double* d_done = nullptr)
{
    if (M > 65535) return fail(PGL_ERR_ARG, "at most 65535 neurons per call");
    const dim3 grid((P + PGL_TRI_TILE - 1) / PGL_TRI_TILE, M);
#define PGL_TRI_LAUNCH(T, E, KC)                                                                                               \
    do {                                                                                                                       \
        if (d_done) hipLaunchKernelGGL((k_smc_tri_matvec_shared<T, E, KC>), grid, dim3(256), 0, h->stream, d_W, d_x, K, M, P, d_y, d_Xt, d_step, scale, d_done); \
        else hipLaunchKernelGGL((k_tri_matvec_shared<T, E, KC>), grid, dim3(256), 0, h->stream, d_W, d_x, K, M, P, d_y, d_Xt, d_step, scale); \
    } while (0)
    if (K == 1) PGL_TRI_DISPATCH(PGL_TRI_LAUNCH, 1);
    else if (K == 2) PGL_TRI_DISPATCH(PGL_TRI_LAUNCH, 2);
    else if (K <= 4) PGL_TRI_DISPATCH(PGL_TRI_LAUNCH, 4);
    else PGL_TRI_DISPATCH(PGL_TRI_LAUNCH, PGL_TRI_SHARED_KC);
#undef PGL_TRI_LAUNCH
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_tri_matvec_shared_dev(pgl_handle h, const double* d_W, int M, int K, int P, int trans, const double* d_x, double* d_y)
{
    if (!h || !d_W || !d_x || !d_y || d_x == d_y || M <= 0 || K <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL)
        return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return tri_shared_launch(h, trans, PGL_TRI_STORE, d_W, K, M, P, d_x, d_y, nullptr, nullptr, 0.0);
}

int pgl_ais_dense_begin_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_W, double* d_Xt)
{
    if (!h || !d_state || !d_W || !d_Xt || K <= 0 || M <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL)
        return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    int rc = launch_rows(h, k_hmc_dense_draw, K * M, pgl_ais_hmc_view(v));
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * v.R;
    rc = tri_shared_launch(h, 1, PGL_TRI_KICK, d_W, K, M, P, v.g, v.p, nullptr, step, 0.5);
    if (rc) return rc;
    return tri_shared_launch(h, 0, PGL_TRI_DRIFT, d_W, K, M, P, v.p, v.q, d_Xt, step, 1.0);
}

int pgl_ais_dense_leap_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_W, const double* d_ll,
                           const double* d_grad, const pgl_prior* prior, int last, int adapt, double* d_Xt, double* d_acc_out,
                           double* d_step_out)
{
    if (!h || !d_state || !d_W || !d_ll || !d_grad || !d_Xt) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    int rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    rc = launch_rows(h, k_ais_dense_target, K * M, v, d_grad, q);
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * v.R;
    rc = tri_shared_launch(h, 1, PGL_TRI_KICK, d_W, K, M, P, v.gu, v.p, nullptr, step, last ? 0.5 : 1.0);
    if (rc) return rc;
    if (!last) return tri_shared_launch(h, 0, PGL_TRI_DRIFT, d_W, K, M, P, v.p, v.q, d_Xt, step, 1.0);
    return launch_rows(h, k_ais_dense_end, K * M, v, d_ll, d_grad, q, adapt ? 1 : 0, d_acc_out, d_step_out);
}

// ---- adaptive sequential Monte Carlo of the evidence (inference/batched_smc.py) ----------------------------------------
long long pgl_smc_state_doubles(int K, int M, int P, int S)
{
    if (K <= 0 || M <= 0 || P <= 0 || S <= 0) return 0;
    return (long long)pgl_smc_doubles((size_t)K, (size_t)M, (size_t)P, (size_t)S);
}

static int smc_args(pgl_handle h, const double* d_state, const double* d_smc, int S)
{
    if (!h || !d_state || !d_smc || S <= 0) return fail(PGL_ERR_ARG, "bad argument");
    return PGL_OK;
}

int pgl_smc_init_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, int n_lo, const pgl_prior* prior,
                     double step0, uint64_t seed, double* d_Xt)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    rc = pgl_ais_init_dev(h, d_state, K, M, P, n_lo, 0, prior, step0, seed, d_Xt);
    if (rc) return rc;
    return launch_rows(h, k_smc_init, M, pgl_smc_view(d_smc, K, M, P, S), step0);
}

// the second half of a stage on its own: gather and retemper by the block's anc, live, rs, beta and step as they stand
int pgl_smc_gather_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const pgl_prior* prior)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    BfgsPrior q;
    rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    const SmcView m = pgl_smc_view(d_smc, K, M, P, S);
    rc = launch_rows(h, k_smc_gather, K * M, v, m);
    if (rc) return rc;
    return launch_rows(h, k_smc_retemper, K * M, v, m, q);
}

int pgl_smc_stage_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const pgl_prior* prior,
                      int n_steps, double cess, double ess_min, double delta_min, uint64_t seed)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    if (n_steps <= 0 || !(cess > 0.0 && cess < 1.0) || !(ess_min >= 0.0 && ess_min <= 1.0) || !(delta_min > 0.0 && delta_min <= 1.0))
        return fail(PGL_ERR_ARG, "n_steps positive, cess in (0, 1), ess_min in [0, 1], delta_min in (0, 1]");
    BfgsPrior q;
    rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    const SmcView m = pgl_smc_view(d_smc, K, M, P, S);
    rc = launch_rows(h, k_smc_stage, M, v, m, n_steps, cess, ess_min, delta_min, (unsigned long long)seed);
    if (rc) return rc;
    return pgl_smc_gather_dev(h, d_state, d_smc, K, M, P, S, prior);
}

int pgl_smc_begin_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_minv,
                      double* d_Xt)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    if (!d_Xt || K <= 0 || M <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const SmcView m = pgl_smc_view(d_smc, K, M, P, S);
    return launch_rows(h, k_smc_begin, K * M, pgl_ais_hmc_view(pgl_ais_view(d_state, K, M, P)), d_minv, M, d_Xt,
                       m.sc + (size_t)PGL_SMC_F_DONE * M);
}

int pgl_smc_leap_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_minv,
                     const double* d_ll, const double* d_grad, const pgl_prior* prior, int last, double* d_Xt)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    if (!d_ll || !d_grad || !d_Xt) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const SmcView m = pgl_smc_view(d_smc, K, M, P, S);
    return launch_rows(h, k_smc_leap, K * M, pgl_ais_view(d_state, K, M, P), d_minv, d_ll, d_grad, q, last ? 1 : 0, d_Xt, m.acc,
                       m.sc + (size_t)PGL_SMC_F_DONE * M);
}

int pgl_smc_dense_begin_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_W,
                            double* d_Xt)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    if (!d_W || !d_Xt || K <= 0 || M <= 0 || P <= 0 || (long long)K * M > 0x7fffffffLL) return fail(PGL_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    const double* done = pgl_smc_view(d_smc, K, M, P, S).sc + (size_t)PGL_SMC_F_DONE * M;
    rc = launch_rows(h, k_smc_dense_draw, K * M, pgl_ais_hmc_view(v), done, M);
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * v.R;
    rc = tri_shared_launch(h, 1, PGL_TRI_KICK, d_W, K, M, P, v.g, v.p, nullptr, step, 0.5, done);
    if (rc) return rc;
    return tri_shared_launch(h, 0, PGL_TRI_DRIFT, d_W, K, M, P, v.p, v.q, d_Xt, step, 1.0, done);
}

int pgl_smc_dense_leap_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_W,
                           const double* d_ll, const double* d_grad, const pgl_prior* prior, int last, double* d_Xt)
{
    int rc = smc_args(h, d_state, d_smc, S);
    if (rc) return rc;
    if (!d_W || !d_ll || !d_grad || !d_Xt) return fail(PGL_ERR_ARG, "bad argument");
    BfgsPrior q;
    rc = ais_prior(h, K, M, P, prior, q);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const AisView v = pgl_ais_view(d_state, K, M, P);
    const SmcView m = pgl_smc_view(d_smc, K, M, P, S);
    const double* done = m.sc + (size_t)PGL_SMC_F_DONE * M;
    rc = launch_rows(h, k_smc_dense_target, K * M, v, d_grad, q, done);
    if (rc) return rc;
    const double* step = v.sc + (size_t)2 * v.R;
    rc = tri_shared_launch(h, 1, PGL_TRI_KICK, d_W, K, M, P, v.gu, v.p, nullptr, step, last ? 0.5 : 1.0, done);
    if (rc) return rc;
    if (!last) return tri_shared_launch(h, 0, PGL_TRI_DRIFT, d_W, K, M, P, v.p, v.q, d_Xt, step, 1.0, done);
    return launch_rows(h, k_smc_dense_end, K * M, v, d_ll, d_grad, q, m.acc, done);
}

// ---- lock-step proximal gradient row kernels for the group-lasso MAP (inference/batched_prox.py) -------------------------
long long pgl_prox_state_doubles(int M, int P) { return (long long)pgl_prox_doubles(M, P); }

static int prox_args(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                     const double* d_lam, double gtol, int maxiter, int max_backtrack, double* d_Xt, double* flags_out,
                     ProxArgs& a)
{
    if (!h || !d_state || !d_ll || !d_grad || !prior || !d_lam || !d_Xt || M <= 0 || P <= 0)
        return fail(PGL_ERR_ARG, "bad argument");
    if (prior->kind != 1) return fail(PGL_ERR_ARG, "proximal gradient serves the group-lasso prior (kind 1) only");
    if (!(gtol > 0.0) || !(prior->sigma > 0.0)) return fail(PGL_ERR_ARG, "gtol and sigma must be positive");
    memset(&a, 0, sizeof(a));
    int rc = fill_prior(h, P, prior, a.q);
    if (rc) return rc;
    a.q.lam = 0.0;                                             // the per-row d_lam rules
    HIPCHK(hipSetDevice(h->device));
    double* flags_dev;
    if (flags_device_pointer(h, flags_out, &flags_dev)) return PGL_ERR_ARG;
    a.ll = d_ll; a.grad = d_grad; a.lam = d_lam; a.gtol = gtol; a.maxiter = maxiter; a.max_backtrack = max_backtrack;
    a.Xt = d_Xt; a.flags = flags_dev;
    return PGL_OK;
}

int pgl_prox_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                      const double* d_lam, double gtol, int maxiter, double* d_Xt, double* flags_out)
{
    ProxArgs a;
    int rc = prox_args(h, d_state, M, P, d_ll, d_grad, prior, d_lam, gtol, maxiter, 1, d_Xt, flags_out, a);
    if (rc) return rc;
    return launch_rows(h, k_prox_init, M, pgl_prox_view(d_state, M, P), a);
}

int pgl_prox_step_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                      const double* d_lam, double gtol, int maxiter, int max_backtrack, double* d_Xt, double* flags_out)
{
    if (max_backtrack <= 0) return fail(PGL_ERR_ARG, "max_backtrack must be positive");
    ProxArgs a;
    int rc = prox_args(h, d_state, M, P, d_ll, d_grad, prior, d_lam, gtol, maxiter, max_backtrack, d_Xt, flags_out, a);
    if (rc) return rc;
    return launch_rows(h, k_prox_step, M, pgl_prox_view(d_state, M, P), a);
}
