/*
 * pyglm_hip.h -- C ABI of the MI355X (gfx950) population-GLM likelihood library.
 *
 * The reference (slinderman/theano_pyglm) has no FFI: its operator boundary is
 *   seval(expr, syms, vals)            pyglm/utils/theano_func_wrapper.py:12-51
 * evaluated on Theano shared variables filled by
 *   Glm.set_data / Population.set_data pyglm/glm.py:99-110, pyglm/population.py:223-231
 * Each entry point below names the reference expression(s) it replaces.  All
 * pointers are plain host pointers unless the name ends in `_dev`; the caller
 * owns host buffers, the library owns device buffers.  Every function returns
 * 0 on success and a negative code on failure; pgl_last_error() gives the text.
 * A handle is bound to one GPU; calls on one handle must be serialised by the
 * caller (like the reference's module-global _func_cache / shared variables).
 *
 * Flat feature-weight layout ("theta", one row per post-synaptic neuron):
 *     theta[0]                      bias                     (bias.py:32)
 *     theta[1 .. 1+Dstim)           stimulus feature weights (bkgd.py:81 / 227: w_stim,
 *                                   for SpatiotemporalStimulus vec(w_t (x) w_x), bkgd.py:214-220)
 *     theta[1+Dstim .. 1+Dstim+N*B) impulse weights w[n_pre*B + b]
 *                                   (impulse.py:58 w_ir; for DirichletImpulses beta, impulse.py:286-308)
 *   P = 1 + Dstim + N*B.  Gradients come back in the same layout (chain rules
 *   through w_t (x) w_x or |g|/sum|g| are applied by the host mirror).
 * Weff is the (N x N) row-major matrix A[n_pre,n_post]*W[n_pre,n_post] (glm.py:31-37).
 */
#ifndef PYGLM_HIP_H
#define PYGLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgl_context* pgl_handle;

#define PGL_OK 0
#define PGL_ERR_ARG (-1)       /* bad argument */
#define PGL_ERR_HIP (-2)       /* HIP runtime error (no device, OOM, launch failure) */
#define PGL_ERR_STATE (-3)     /* call order (e.g. ll before set_spikes) */
#define PGL_ERR_UNSUPPORTED (-4) /* shape outside what the kernels were built for */

#define PGL_NLIN_EXP 0         /* nlin.py:25 */
#define PGL_NLIN_EXPLINEAR 1   /* nlin.py:43 */

/* flags for pgl_set_option */
#define PGL_OPT_FEATURE_F32 1  /* 0 (default): f64 features.  1: the in-kernel-feature kernels stage the feature tile in LDS as f32.
                                * 2: reduced-traffic mode for narrow shards -- the RESIDENT feature blocks of the one-post-tile
                                * kernel (a shard of <= 16 neurons against a 400..640-column row: north star's neuron split at
                                * 8 GPUs) are STORED as f32 and widened to f64 on their way into LDS; every arithmetic operation
                                * stays f64, only the stored feature is rounded (2^-24 relative).  Other shapes ignore it. */
#define PGL_OPT_NCHUNKS 2      /* override the number of time chunks (0 = auto) */
#define PGL_OPT_KERNEL 3       /* 0 = auto: two-pass kernel on resident tiles for >= 65 post-synaptic neurons per call;
                                * below that the K-split kernel, on resident feature tiles (6) when the
                                * feature row is short enough for two LDS step buffers (N*B + Dstim up to
                                * ~320-450 columns depending on the post block), else with in-kernel
                                * feature generation (2); rows of <= 320 columns and <= 64 post neurons: one wave per
                                * post tile without any K split (7);  6 / 7 = force those kernels when they fit;
                                * 2 = force the K-split kernel; 3 = force the two-pass kernel with
                                * on-the-fly features; 4 = force the two-pass kernel on resident feature
                                * tiles.  Auto uses 4's kernel (k_fused5) when the call covers >= 65
                                * post-synaptic neurons and the device can hold the tiles
                                * (nT/16 * 2 * ~41 KB at K = 640: 3.1 GB for nT = 600 000) */

#define PGL_OPT_GIBBS_KERNEL 4 /* pgl_gibbs_ll_cols with the explinear nonlinearity: 0 = auto (regime-split kernels: single
                                * precision for the log1p(exp(-|x|)) term where |x| >= 12, compacted f64 elsewhere (log1p
                                * through a 32-interval table: < 2e-16 absolute),
                                * spike terms from the event lists); 1 = the all-f64 one-thread-per-(column, weight)
                                * kernel (always used for the exp nonlinearity) */
#define PGL_OPT_EPI_F64 5      /* 1 = all-f64 rate epilogue of the fused ll+grad kernels.  Default 0: in waves whose currents
                                * are all > 12 the exp(-x) < 6.2e-6 inside softplus / sigmoid comes from the single-precision
                                * hardware exp (rate and residual within 5e-13 relative of the all-f64 form) */

#define PGL_OPT_TIMING 6       /* HIP events around every n-th evaluation (pgl_last_timing / pgl_timing_summary): 1 = every call
                                * (default), n > 1 = a sample, 0 = none.  An event between two kernels of a stream costs ~6 us of
                                * GPU idle time; loops that queue evaluations back to back (optimisers, bench.py) sample or
                                * switch the events off */
#define PGL_OPT_BFGS_MERGE 7   /* pgl_bfgs_step_dev: a whole optimiser iteration is ONE row kernel while hk_bound * P <= value
                                * (doubles of update history per row that one workgroup walks; default 65536), else the split
                                * form with the multi-workgroup history kernels; 0 = always split */

#define PGL_OPT_RECORD_KERNELS 96 /* dev / test: 1 = every ll(+grad) evaluation and pgl_gibbs_prepare_all records the fused kernel
                                   * instantiations it launches, in launch order (pgl_last_kernels), and so do pgl_hvp_prepare_* /
                                   * pgl_hvp_apply_dev (k_hvp5 and the k_fused* launches around it), pgl_hess_dev (k_hess) and
                                   * pgl_rescale_dev (the forward launches, then k_rescale_*) and pgl_pointwise_dev (the forward launches,
                                   * then k_pw_chunk and k_pw_block); pgl_gibbs_ll_cols and pgl_gibbs_update_cols APPEND the names of
                                   * their launches (k_gibbs_cols_setup, k_gibbs_pre_features, k_gibbs_rate_cols, k_gibbs_reduce_cols2 /
                                   * k_gibbs_ll_cols, k_gibbs_reduce_cols / k_gibbs_update_cols) to the record, which setting the option
                                   * clears; 0 (default) = off */

#define PGL_OPT_DECODE_CUT 89  /* dev / test: the 256-bin chunks a workgroup of k_dec_forward and the 64-bin tiles a workgroup of
                                * k_dec_backward take (0 or 1 = one, the default; at most 64).  The results are the same bits at
                                * every value: each element has one thread and a fixed order of additions. */

/* Development switches (not part of the drop-in surface; results stay valid unless stated): 99 = debug word: bits 16..20 force
 * the sub-block loop of k_gibbs_rate_cols (1 .. 16; bits 8..11 are the older 4-bit field of the same, bit 12 switches the
 * shared-presynaptic path off), the low bits are timing ablations with invalid results; 95 = 2 keeps the narrow post
 * blocks of a wide population off the one-image-buffer form of k_fused6 and the block-ring kernel k_fused8 (they run on
 * k_fused2); 97 = waves per block of
 * the partial reduction; 98 = post tiles per workgroup of the K-split kernels; 99 = kernel-internal ablation bits of the
 * fused / Gibbs kernels (!= 0 invalidates the results, except bit 0x1000: event-window pair currents although all columns
 * share the presynaptic neuron, and bits 8-11: forced sub-block count of k_gibbs_rate_cols). */

/* What pgl_version() returns: it changes with every change of a signature or a struct below, and a binding refuses a
 * library that reports another number (theano_pyglm_amd/_lib.py: ABI_VERSION). */
#define PGL_ABI_VERSION 119

const char* pgl_last_error(void);
int pgl_version(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int pgl_device_count(void);

/* Context for a population of N neurons observed for nT bins of width dt, with
 * B impulse basis functions of R taps (impulse.py:92-112).  Mirrors
 * Population.__init__/Glm.__init__ (population.py:12-32, glm.py:8-63). */
int pgl_create(int N, int64_t nT, int B, int R, int nlin, double dt, int device,
               pgl_handle* out);
int pgl_destroy(pgl_handle h);
int pgl_set_option(pgl_handle h, int option, int value);

/* Glm.set_data: S.set_value(data["S"]) (glm.py:99-103).  Spike counts (nT,N)
 * row-major.  The f64 form checks that every count is an integer in 0..255
 * (population.py:345-349 caps at 10) and stores uint8. */
int pgl_set_spikes_u8(pgl_handle h, const uint8_t* S);
int pgl_set_spikes_f64(pgl_handle h, const double* S);

/* The interpolated impulse basis `ibasis` (R,B) row-major (impulse.py:92-112, 359-376). */
int pgl_set_basis(pgl_handle h, const double* ibasis);

/* bkgd_model.set_data: stim.set_value(data['fstim']) (bkgd.py:156-157, 342-345).
 * fstim is (nT, Dstim) row-major; Dstim = 0 / NULL = NoStimulus (bkgd.py:29-43). */
int pgl_set_stim_features(pgl_handle h, const double* fstim, int Dstim);

/* BasisStimulus / SpatiotemporalStimulus.preprocess_data on the device (bkgd.py:122-154,
 * 303-340; basis.py:201-273): linear interpolation of the raw stimulus (Tstim, D) from the dt_stim
 * grid to the dt grid (np.interp, clamped at the ends), projection on the spatial basis
 * basis_x (D,Bx) (NULL = identity), strictly causal convolution with every temporal basis
 * basis_t (Rt,Bt).  The features stay on the device as the Dstim = Bx*Bt extra columns of F:
 * layout 0: column bt*Bx+bx (SpatiotemporalStimulus, bkgd.py:337-340), layout 1: column bx*Bt+bt
 * (BasisStimulus d*B+b, bkgd.py:148-152).  pgl_get_stim_features copies them out (nT, Dstim). */
int pgl_set_stimulus(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim,
                     const double* basis_x, int Bx, const double* basis_t, int Rt, int Bt,
                     int layout);
int pgl_get_stim_features(pgl_handle h, double* fstim_out);

/* SpatiotemporalStimulus with a WIDE stimulus (bkgd.py:172-345): the rank-1 structure
 * w_stim = vec(w_t (x) w_x) (bkgd.py:214-220) is kept on the device instead of materialising the
 * (nT, Bt*Bx) feature matrix of pgl_set_stimulus (7.4 GB at D = 1024, T = 300 s):
 *   I_stim[:,n] = causal conv( np.interp( (stim . basis_x) . w_x[n] ), basis_t . w_t[n] )
 * -- one GEMM at the stimulus frame rate plus a 1-D convolution per neuron; gradients by the transposed
 * operations.  After this call a theta row is [bias, w_t(Bt), w_x(Bx), w_imp(N*B)] (the reference's own
 * packing order of 'bkgd': 'w_t' < 'w_x', packvec.py:22) with P = 1 + Bt + Bx + N*B, and gradients come
 * back in that layout (no host chain rule).  basis_x (D,Bx) row-major or NULL = identity.
 * When dt_stim is an integer multiple q of dt, ceil(Rt / q) + 2 <= 8 and Bt <= 4 (the reference's frames of 100
 * bins with Rt = 300 qualify) the evaluation runs at the FRAME rate: the interpolated projection is piecewise
 * linear over q-bin frames, so the Rt taps of a bin collapse to <= 8 frame values through a coefficient table
 * built here (k_sepf_fwd / k_sepf_bwd), and the impulse columns run on resident feature tiles -- for neuron ranges
 * and neuron lists of up to 128 neurons (up to 64 neurons, <= 3 temporal bases, <= 5 frame values and q >= 16 the
 * stimulus current is five more k-steps of the fused kernel's forward contraction instead of a kernel of its own);
 * other ratios and populations of more than 128 neurons keep the tap-rate kernels (same results to 1e-12;
 * pgl_info[12] tells which). */
int pgl_set_stimulus_separable(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim,
                               const double* basis_x, int Bx, const double* basis_t, int Rt, int Bt);

/* Restrict pgl_ll_grad to the bins [t_lo, t_hi) (t_lo a multiple of 16): ll and gradient
 * become the partial sums over that range, while features still see the spikes before t_lo.
 * The likelihood is a sum over data segments (population.py:41-43), so a time range per GPU
 * plus an all-reduce of (ll, grad) shards one evaluation over GPUs.  Default: [0, nT). */
int pgl_set_time_range(pgl_handle h, int64_t t_lo, int64_t t_hi);

/* seval(glm.ll) and seval(g_glm_ll) for every post-synaptic neuron n in
 * [n_lo, n_hi) in one fused pass (glm.py:39-52; coord_descent.py:27-30, 52-57, 73-78;
 * population.py:71-86).  theta is ((n_hi-n_lo), P), Weff is (N,N).
 * ll_out[(n_hi-n_lo)], grad_out[(n_hi-n_lo)*P] (grad_out may be NULL: ll only). */
int pgl_ll_grad(pgl_handle h, int n_lo, int n_hi, const double* theta,
                const double* Weff, double* ll_out, double* grad_out);

/* Same with device pointers, asynchronous on the handle's stream; pair with pgl_sync. */
int pgl_ll_grad_dev(pgl_handle h, int n_lo, int n_hi, const double* d_theta,
                    const double* d_Weff, double* d_ll, double* d_grad);
/* The same for an arbitrary list of post-synaptic neurons: d_idx[j] (device, int32, distinct) is the
 * neuron of row j of d_theta / d_ll / d_grad.  Lets a lock-step optimiser evaluate only the neurons
 * whose line search is still running (the reference fits one neuron per call, coord_descent.py:161-204). */
int pgl_ll_grad_list_dev(pgl_handle h, const int* d_idx, int count, const double* d_theta,
                         const double* d_Weff, double* d_ll, double* d_grad);
int pgl_sync(pgl_handle h);

/* Hessian-vector products of ll: hessian_rop_wrt_list (pyglm/utils/grads.py:68-95, T.Rop of the gradient) and the
 * hessp that fmin_ncg takes in map.py:38-45.  With the feature row f_t = [1, fstim[t,:], Weff[n',n] fS[t,n',b]] and
 * x_t = f_t . theta_n:
 *     H_n . v = sum_t c_t f_t (f_t . v),    c_t = -dt lam''(x_t) + S[t,n] (log lam)''(x_t)
 *     exp:        lam'' = e^x, (log lam)'' = 0
 *     explinear:  lam'' = sig (1 - sig), (log lam)'' = sig (1 - sig) / lam - sig^2 / lam^2,  sig = 1 / (1 + e^-x)
 * c depends on theta only, so the interface has two steps:
 *   prepare: forward contraction with theta, c[t,n] of the listed rows over the handle's time range stays on the device
 *            (all f64; nT * 16 ceil(rows / 16) doubles, the footprint of the residual slab).  Limits: exp -- x is
 *            clamped at 709, c stays finite; explinear -- c -> 0 for x -> +inf and for x -> -inf (the limit of
 *            (log lam)'' there, not the reference's 0/0 at lam == 0); a NaN current gives a NaN c.
 *   apply:   hv = F^T . (c o (F . v)): rows as prepared, d_v (count, P) in, d_hv (count, P) out, both in the theta layout.
 *            One forward contraction, one multiply per element, one backward contraction: 4 nT N^2 B flops and no
 *            transcendental.  Calls of >= 65 neurons against one column slice run the fused kernel on resident feature
 *            tiles (k_hvp5, then pass 2 of k_fused5; visible through pgl_last_kernels); every other population, range
 *            or list runs the forward-only / backward-only launches of the 3-phase path around a row kernel.
 * hv is H . v of ll itself: not negated, no prior.  The _dev forms are asynchronous on the handle's stream.
 * pgl_set_time_range is honoured: the product is the partial sum over the range (all-reduce it like (ll, grad)).
 * apply before prepare, after a changed time range or after new spikes / basis / stimulus: PGL_ERR_STATE.  A separable
 * stimulus (pgl_set_stimulus_separable: the current is not linear in w_t, w_x) gives PGL_ERR_UNSUPPORTED.
 * The handle keeps its own copy of Weff and of the neuron list between prepare and apply. */
int pgl_hvp_prepare_dev(pgl_handle h, int n_lo, int n_hi, const double* d_theta, const double* d_Weff);
int pgl_hvp_prepare_list_dev(pgl_handle h, const int* d_idx, int count, const double* d_theta, const double* d_Weff);
int pgl_hvp_apply_dev(pgl_handle h, const double* d_v, double* d_hv);
/* prepare + one apply with host pointers: theta, v, hv_out ((n_hi-n_lo), P), Weff (N,N).  A call that repeats the range,
 * time range, theta and Weff of the previous pgl_hvp call (the products of one CG solve) skips the prepare. */
int pgl_hvp(pgl_handle h, int n_lo, int n_hi, const double* theta, const double* v, const double* Weff, double* hv_out);

/* Dense Hessians of ll: hessian_wrt_list (pyglm/utils/grads.py:30-66), the default of the reference's parallel driver
 * (parallel_coord_descent.py:62 use_hessian=True).  With f_t and c_t as above:
 *     H_n = sum_t c_t f_t f_t^T
 * for every row of the last pgl_hvp_prepare_dev / pgl_hvp_prepare_list_dev, from the curvature that prepare left on the
 * device: one weighted Gram contraction over time on the f64 matrix cores (k_hess: nT P^2 flops per row over one triangle,
 * against P applies of 4 nT N^2 B flops each for the same matrix from products), features built in LDS from the event
 * lists, per-chunk partials reduced in a fixed order (deterministic).
 *   d_H (count, P, ld), ld >= P, is the caller's (uninitialised is fine; columns P .. ld-1 are not written); rows and
 *   columns in the theta layout.  Both triangles are stored, from the same registers: H[i][j] and H[j][i] hold the same bits.
 * The result is the Hessian of ll itself: not negated, no prior.  Asynchronous on the handle's stream.  pgl_set_time_range
 * is honoured: the result is the partial sum over the range.  Without a valid prepare (none yet, a changed time range, new
 * spikes / basis / stimulus): PGL_ERR_STATE, as pgl_hvp_apply_dev; a separable stimulus: PGL_ERR_UNSUPPORTED; ld < P:
 * PGL_ERR_ARG.  Needs count * (P / 64)^2 / 2 * 32 KB of scratch memory for the partials, at most 512 MB (more rows than fit
 * run as several launches). */
int pgl_hess_dev(pgl_handle h, double* d_H, int ld);
/* prepare + pgl_hess_dev with host pointers: theta ((n_hi-n_lo), P), Weff (N,N), H_out ((n_hi-n_lo), P, P). */
int pgl_hess(pgl_handle h, int n_lo, int n_hi, const double* theta, const double* Weff, double* H_out);

/* Batched dense factorisation for the Laplace posterior (inference/laplace.py; the reference builds the Hessian for its
 * Newton fit and has no Laplace step).  With A_m = minus the Hessian of the log posterior of row m, symmetric, in the
 * theta layout as pgl_hess_dev leaves it:
 *     D = diag A,  C = D^-1/2 A D^-1/2 = Ls Ls^T                    (the equilibrated factorisation of laplace_from_hessian)
 *     log det A = 2 sum_i log Ls_ii + sum_i log A_ii
 * factor: in place on d_A (M, P, ld), ld >= P.  Only the lower triangle is read; it becomes Ls.  The strict upper triangle
 *   and the columns P .. ld-1 are neither read nor written.  d_scale (M, P) = sqrt(A_ii), d_logdet (M), d_info (M) int32:
 *   0, or k + 1 for the first column k whose diagonal entry or pivot is non-finite or <= 0 -- then the lower triangle, the
 *   scales and the log det of that row are NaN (the other rows are not affected).  One workgroup per matrix, blocked
 *   right-looking in blocks of 32 columns (k_chol_factor: diagonal block in LDS, panel rows solved against it 128 at a
 *   time, trailing 64 x 64 tiles updated); LDS holds the 32 x 32 diagonal block and 128 rows of the panel (42 KB) whatever
 *   P is, so any P runs.  P^3 / 3 flops per matrix; the length of the recording does not enter.
 * inverse: the lower triangle of every d_L (M, P, ld) becomes its inverse, in place, by blocked forward substitution
 *   (k_tri_inverse; |L X - I| <= c P u |L| |X| componentwise, as a column-by-column substitution gives).  Rows with
 *   d_info[m] != 0 are skipped (they stay NaN after a failed factor); the same parts stay untouched.  Meant for the
 *   well-scaled Ls: the caller puts the scales back, (D^1/2 Ls)^-1 = Ls^-1 D^-1/2.
 * Both are f64 throughout, sum in an order that depends on P alone (a row's bits do not depend on the batch it is in, two
 * runs give the same bits), use no atomics and are asynchronous on the handle's stream.  M <= 0, P <= 0, ld < P or a null
 * pointer: PGL_ERR_ARG.  The handle supplies device and stream only: no data set is needed. */
int pgl_chol_factor_dev(pgl_handle h, double* d_A, int M, int P, int ld, double* d_scale, double* d_logdet, int* d_info);
int pgl_tri_inverse_dev(pgl_handle h, double* d_L, int M, int P, int ld, const int* d_info);
/* solve against the factor: for every row m with d_info[m] == 0
 *     x = D^-1/2 Ls^-T Ls^-1 D^-1/2 b = A^-1 b
 *   with d_Ls (M, P, ld) and d_scale (M, P) exactly as pgl_chol_factor_dev left them (only the lower triangle is read);
 *   d_b and d_x are (M, P) and may be the same memory.  A row with d_info[m] != 0 gets NaN in x, and nothing else of it is
 *   read or written.  One workgroup per matrix (k_chol_solve): blocked forward then backward substitution in blocks of 32,
 *   the diagonal block in LDS and solved in the registers of one wave, the off-diagonal part as a blocked matrix-vector
 *   product along the rows of Ls; 2 P^2 flops per matrix, where the inverse costs P^3 / 3 and two products.  The result
 *   satisfies the componentwise bound of a substitution, |Ls y - D^-1/2 b| <= c P u |Ls| |y| and its transpose.
 *   f64 throughout, no atomics, sums in an order that depends on P alone, asynchronous on the handle's stream; argument
 *   errors as for the factor. */
int pgl_chol_solve_dev(pgl_handle h, const double* d_Ls, int M, int P, int ld, const double* d_scale, const int* d_info,
                       const double* d_b, double* d_x);

/* The lock-step optimiser (inference/batched_bfgs.py) as row kernels on the handle's stream.  The reference calls
 * scipy.optimize.minimize(method="bfgs") neuron by neuron (coord_descent.py:161-204); these run the same algorithm --
 * BFGS from H = I, More'-Thuente strong-Wolfe line search with scipy's constants and first trial step
 * (csrc/pglm_linesearch.h), stop on max|g| <= gtol or maxiter iterations -- for all M neurons of a shard at once, one
 * fused ll+grad launch per trial step.  All optimiser state of a shard of M neurons with P parameters lives in ONE
 * device block of pgl_bfgs_state_doubles(M, P) doubles (flags and counters stored as doubles), in this order:
 *   (M,P) each: X, g, p, H g, s, y, t = H g_new, Xb, gb (best trial of the running search);
 *   (M,P,3) each: U, V (pending H += U V^T);
 *   (M) each: f, fprev, alpha, slope, rho, hscale, iters, restarts, active, frozen, acc, upd, stall, ident, pend, fb,
 *             nfev, hk (updates in the history);  then the line-search state, (18, M).
 * The dense inverse Hessians d_H (M, P, ld), ld even and >= P, are the caller's buffer (uninitialised is fine).
 *   init:       X, f, g of every row in place -> steepest-descent start, first trial step min(1, 1.01/|g|)
 *   trial:      Xt[j] = X[r] + alpha[r] p[r], r = d_rows[j] (NULL: j), j < L
 *   objective:  rows of d_Xt are theta rows [bias, w_stim, w_ir]; in place ll -> f = -(ll + log prior),
 *               grad -> g = -(grad + prior gradient) with fit_glm's NaN rules (coord_descent.py:170-182);
 *               the prior is a pgl_prior (rows in another packing: the caller supplies f and g itself)
 *   linesearch: one step of every listed row's search: next trial step, or the row takes the step (acc = 1), or the
 *               search is stuck: best sufficient-decrease point if any, else stall = 1 (scipy stops with
 *               "precision loss" there); at most max_trials steps per search (scipy: 100)
 *   hmul:       rows with acc = 1: H += U V^T (pending update) and t = H g in one pass over H
 *   update:     U, V, H_new g, next direction and first step, restart (once) / freeze of stalled rows, convergence;
 *               init_scaling != 0: H <- (s.y / y.y) I before the first update after a (re)start (not scipy's). */

/* The prior of a theta row [bias, w_stim, w_ir], for every lock-step call below that takes one (read during the call, not
 * kept):  bias ~ N(mu_b, sg_b) (bias.py:33), stimulus weights ~ N(0, stim_sigma) (bkgd.py:76), and the impulse weights
 * kind 0: N(mu, sigma) (priors.py:139), kind 1: group lasso, -(lam / sigma) sum_g |w_g - mu|_2 over the N groups of B
 * (priors.py:202).  Any other kind is PGL_ERR_ARG, except that pgl_bfgs_step_dev takes kind < 0 as "f and g arrive final".
 * A NULL prior is PGL_ERR_ARG. */
typedef struct pgl_prior { int kind; double mu_b, sg_b, stim_sigma, mu, sigma, lam; } pgl_prior;

long long pgl_bfgs_state_doubles(int M, int P);
int pgl_bfgs_init_dev(pgl_handle h, double* d_state, int M, int P, double gtol);
int pgl_bfgs_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt);
int pgl_bfgs_objective_dev(pgl_handle h, int L, int P, const double* d_Xt, double* d_ll_f, double* d_grad_g,
                           const pgl_prior* prior);
int pgl_bfgs_linesearch_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                            const double* d_f, const double* d_g, int max_trials);
int pgl_bfgs_hmul_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_H, int ld);
/* hmul with the inverse Hessians kept implicit: H = hscale I + sum_j U_j V_j^T over the update history that
 * pgl_bfgs_update_dev appends to -- d_hist [M][Kmax][2][P] (s_j, H y_j), d_coef [M][Kmax][2] -- Kmax >= maxiter;
 * d_ab: scratch [M][Kmax][2].  Reads 4 hk P numbers per row instead of 2 P^2: the cheaper form while hk <= P / 2,
 * and no P^2 memory. */
int pgl_bfgs_hmul_hist_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_hist,
                           const double* d_coef, int Kmax, double* d_ab);
/* d_hist / d_coef NULL: dense form (pgl_bfgs_hmul_dev) */
int pgl_bfgs_update_dev(pgl_handle h, double* d_state, int M, int P, double gtol, int maxiter, int init_scaling, double* d_hist,
                        double* d_coef, int Kmax);
/* Everything an evaluation of the L listed rows is followed by, as ONE call (and, while the update history is short, ONE
 * row kernel -- one workgroup per row -- instead of objective | linesearch | hmul | update | trial): priors and NaN rules on
 * (d_ll_f, d_grad_g) in place (prior->kind >= 0; < 0: they already hold f and g), the line-search step, t = H g for the rows
 * that took a step (update history d_hist / d_coef / d_ab as for pgl_bfgs_hmul_hist_dev, or dense d_H / ld as for
 * pgl_bfgs_hmul_dev -- exactly one of the two), the update, and the NEXT trial point of every listed row:
 *   d_Xt_next[d_pos_next[r]] = X[r] + alpha[r] p[r]   (d_pos_next (M) int32: position of row r in the next launch's list, < 0
 *   = not listed any more; NULL = same positions as this launch; d_Xt_next NULL = no trial points).
 * flags_out (NULL or M doubles of PINNED host memory): active flag of every listed row, written by the kernel itself -- the
 * driver polls it behind an event, no copy kernel.  hk_bound: upper bound on the updates in any row's history (launches so
 * far), selects the one-kernel or the split form (PGL_OPT_BFGS_MERGE).  coord_descent.py:161-204 is the unit replaced. */
int pgl_bfgs_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt, double* d_ll_f,
                      double* d_grad_g, const pgl_prior* prior, int max_trials, double gtol, int maxiter, int init_scaling,
                      double* d_hist, double* d_coef, int Kmax, double* d_ab, int hk_bound, double* d_H, int ld,
                      const int* d_pos_next, double* d_Xt_next, double* flags_out);

/* Lock-step Newton-CG (inference/batched_newton_cg.py) as row kernels on the handle's stream: the algorithm of
 * scipy.optimize.minimize(method='Newton-CG', jac=, hessp=) as fit_glm(use_rop=True) calls it per neuron
 * (parallel_coord_descent.py:119-121 / map.py:38-45; restated in csrc/pglm_ncg.h with the places where it differs), for all
 * M neurons of a range at once: every CG iteration is ONE pgl_hvp_apply_dev over all M rows, every line-search trial one
 * pgl_ll_grad_list_dev of the rows still searching.  All optimiser state of M rows of P parameters lives in ONE device block
 * of pgl_ncg_state_doubles(M, P) doubles (flags and counters stored as doubles), in this order:
 *   (M,P) each: X, g, xsupi (the direction pk), ri, psupi, Xb, gb (best trial of the running search);
 *   (M) each:   f, fprev, dri0, termcond, cgit, alphai, nit, nhev, nfev, status (-1 running, else scipy's 0 success,
 *               1 maxiter, 2 precision loss, 3 CG failure), phase (0 CG, 1 line search, 2 finished), slope, alpha, fb,
 *               alpha_acc, moved;  then the line-search state, (18, M).
 * Rows are theta rows [bias, w_stim, w_ir]; the objective is f = -(ll + log prior), H v = -(H_ll v + H_prior v) with the
 * pgl_prior and fit_glm's NaN rules (objective NaN -> 1e16, a gradient or a
 * product holding a NaN -> 0).  d_V (M, P) is the input of the next product, row by row (zero for every row whose CG does
 * not run, so that its product is harmless); flags_out (NULL or M doubles of PINNED host memory) receives the phase of
 * every row a kernel has advanced, written by the kernel itself.  A finished row is never written again.
 *   init:        X in the state, (d_ll, d_grad) = ll and gradient at X by row (overwritten with f, g): start of the first
 *                outer iteration (b, termcond, CG start, d_V); maxiter <= 0 ends every row with status 1.
 *   cg_step:     d_hv (M, P) = the product of d_V just made (overwritten): prior term, sign, NaN rule, curvature and the
 *                stop tests, CG update, next d_V; a row whose CG ends starts its line search (phase 1) or finishes.
 *   trial:       Xt[j] = X[r] + alpha[r] pk[r], r = d_rows[j] (NULL: j), j < L.
 *   search_step: (d_ll_f, d_grad_g) = evaluation of the trial points d_Xt of the L listed rows by list position
 *                (overwritten): one More'-Thuente step per row; another trial -> d_Xt_next[d_pos_next[r]] (NULL: same
 *                position; < 0: not listed; d_Xt_next NULL: none, use trial); accepted -> convergence test
 *                (|alpha pk|_1 <= P * 1e-5: status 0) or the start of the next outer iteration as in init. */
long long pgl_ncg_state_doubles(int M, int P);
int pgl_ncg_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                     int maxiter, double* d_V, double* flags_out);
int pgl_ncg_cg_step_dev(pgl_handle h, double* d_state, int M, int P, double* d_hv, const pgl_prior* prior, double* d_V,
                        double* flags_out);
int pgl_ncg_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt);
int pgl_ncg_search_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                            double* d_ll_f, double* d_grad_g, const pgl_prior* prior, int maxiter, const int* d_pos_next,
                            double* d_Xt_next, double* d_V, double* flags_out);

/* Lock-step dense Newton (inference/batched_newton.py) as row kernels on the handle's stream: the reference's default
 * second-order route (parallel_coord_descent.py:62 use_hessian=True; map.py:38-45) as a line-search Newton method with
 * Hessian modification (restated in csrc/pglm_newton.h), for all M neurons of a range at once.  Per outer iteration, for
 * the rows still running: pgl_hvp_prepare_list_dev + pgl_hess_dev (summed over the data sequences), assemble,
 * pgl_chol_factor_dev, pgl_chol_solve_dev, direction; then one pgl_ll_grad_list_dev of the rows still searching per
 * line-search trial.  All optimiser state of M rows of P parameters lives in ONE device block of
 * pgl_newton_state_doubles(M, P) doubles (flags and counters stored as doubles), in this order:
 *   (M,P) each: X, g, p (the direction), Xb, gb (best trial of the running search);
 *   (M) each:   f, fprev, slope, alpha, shift, nit, nfev, nhess, nfact, status (-1 running, 0 converged, 1 maxiter, 2 the
 *               search found no acceptable point, 3 no descent direction), phase (0 needs a Hessian, 1 line search,
 *               2 finished, 3 refactor: its shift was raised);  then the line-search state, (18, M).
 * Rows are theta rows [bias, w_stim, w_ir]; the objective is f = -(ll + log prior) with the pgl_prior and fit_glm's NaN
 * rules (objective NaN -> 1e16, a gradient holding a NaN -> 0), as pgl_ncg_* applies them.  d_rows (L) int32 lists rows of
 * the state (NULL: row j at position j); everything "by list position" is (L, ..).  flags_out (NULL or M doubles of PINNED
 * host memory) receives the phase of every row a kernel has advanced.  A finished row is never written again.
 *   init:        X in the state, (d_ll, d_grad) = ll and gradient at X by row (overwritten with f, g); maxiter <= 0 ends
 *                every row with status 1, else a row with max|g| <= gtol ends with status 0, else phase 0.
 *   assemble:    d_H (L, P, ld) holds the sum over the data sequences of the Hessians of ll of the listed rows
 *                (pgl_hess_dev); its lower triangle becomes A = -H - H_prior(X) + shift diag(-H - H_prior) in place (the
 *                strict upper triangle is neither read nor written).  H_prior: kind 0 a constant diagonal; kind 1 the
 *                B x B block of every group, -(lam / sigma) (I / |d| - d d^T / |d|^3), d = w_g - mu: non-finite at a zero
 *                group, which then fails the factor.  d_rhs (L, P) or NULL: -g of the listed rows, the solve's input.
 *                The state is read only (X, g, shift).
 *   direction:   d_info (L) and d_p (L, P) = -(A + shift diag A)^-1 g from factor and solve.  A row whose factor failed or
 *                whose slope g.p is not negative (or not finite) raises its shift, 0 -> 1e-6 -> x 100 -> .. -> 1e2, and
 *                goes to phase 3: assemble from the SAME Hessian, factor, solve, direction again -- the Hessian is not
 *                recomputed, the caller keeps an unshifted copy.  After the last shift the row takes p = -g.  Otherwise
 *                p = d_p, and the row's More'-Thuente search starts with first step 1 (phase 1).
 *   trial:       Xt[j] = X[r] + alpha[r] p[r] for a row in phase 1, X[r] for any other (the points of a Hessian list).
 *   search_step: as pgl_ncg_search_step_dev; a row that takes a point converges when max|g| <= gtol (status 0), stops
 *                with status 1 when nit == maxiter, else goes back to phase 0 with shift 0; a stuck search: status 2. */
long long pgl_newton_state_doubles(int M, int P);
int pgl_newton_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                        double gtol, int maxiter, double* flags_out);
int pgl_newton_assemble_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_H, int ld,
                            const pgl_prior* prior, double* d_rhs);
int pgl_newton_direction_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const int* d_info,
                             const double* d_p, double* flags_out);
int pgl_newton_trial_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, double* d_Xt);
int pgl_newton_search_step_dev(pgl_handle h, double* d_state, int M, int P, const int* d_rows, int L, const double* d_Xt,
                               double* d_ll_f, double* d_grad_g, const pgl_prior* prior, double gtol, int maxiter,
                               const int* d_pos_next, double* d_Xt_next, double* flags_out);

/* Lock-step Hamiltonian Monte Carlo (inference/batched_hmc.py) as row kernels on the handle's stream: posterior samples of
 * the theta rows [bias, w_stim, w_ir] of M neurons n_lo .. n_lo + M - 1 at once (C chains each: see "chains" below; every
 * call but init takes the C M rows as its M), one workgroup per row around ONE
 * pgl_ll_grad_dev over all rows per leapfrog step.  The algorithm is Neal (2011) fig. 2 as inference/hmc.py: hmc_lockstep
 * states it (restated in csrc/pglm_hmc.h) with a diagonal mass matrix:
 *     U = -(ll + log prior), the prior a pgl_prior.  A non-finite ll + log prior gives
 *         U = +inf; a NaN or infinite entry of its gradient becomes 0; a transition that ends at a non-finite energy is
 *         rejected (the rules of hmc_lockstep's callers, gibbs.py: _neg_lp_grad).
 *     K = 1/2 sum_j p_j^2 minv_j;  d_minv (M, P) is the diagonal of the inverse mass matrix, NULL = identity.
 *     transition t:  p_j = z_j / sqrt(minv_j);  H0 = U + K;  p -= step/2 grad U;  n_leapfrog times { q += step minv o p;
 *         p -= step grad U(q) (step/2 the last time) };  H1 = U(q) + K(p);  accept iff H1 is finite and log u < H0 - H1.
 * Random numbers are stateless, from the mix of pgl_simulate_batch:
 *     G      = 0x9e3779b97f4a7c15                                   (all arithmetic in uint64, wrapping)
 *     mix(z) : z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
 *     key    = mix(mix(mix(seed + G) + G * (n + 1)) + G * (t + 1))   n: NEURON index (n_lo + row), t: transition, from 0
 *     U(k)   = ((double)(mix(key + G * (k + 1)) >> 11) + 0.5) * 2^-53                       in (0, 1]
 *     u      = U(0)                                                   the accept uniform of (seed, n, t)
 *     z_j    = sqrt(-2 log U(2 j + 1)) * cos(6.283185307179586 * U(2 j + 2))               component j (Box-Muller)
 * The key holds the neuron index, not the row of the call: a chain over [n_lo, n_hi) equals the matching rows of a chain
 * over [0, N).  Every sum over a row has a fixed order: two runs give the same bits.
 * Step size: one per row.  While t < n_warmup, after the decision: factor = 1.02 if avg_accept > 0.9 else 0.98 (avg_accept
 * before the update), avg_accept = 0.95 avg_accept + (1 - 0.95) accepted, step = clip(step * factor, 1e-3, 1)
 * (adapt_step_size of inference/hmc.py); from t = n_warmup on it is frozen.  (The reference, gibbs.py:306-316, shares one
 * step size among all neurons and adapts for ever.)
 * All state of M rows of P parameters lives in ONE device block of pgl_hmc_state_doubles(M, P) doubles, in this order:
 *   (M,P) each: q (the current point), p (momentum), q0 (start of the running transition), g (grad U at the last accepted
 *               point);
 *   (M) each:   U0 (U at the last accepted point), H0, step, avg_accept (starts at 0.9), n_accept (accepted transitions
 *               among those with t >= n_warmup), t (completed transitions), acc (the last decision), neuron, seed_lo,
 *               seed_hi (the 32-bit halves of the seed).
 *   init:   q in the state, (d_ll, d_grad) = ll (C M) and its gradient (C M, P) at q (overwritten with U, grad U); t = 0.
 *   begin:  draws the momentum, H0, the half kick and the first drift; d_Xt (M, P, not part of the state) = the points to
 *           evaluate next.
 *   leap:   (d_ll, d_grad) = the evaluation at d_Xt (overwritten).  last == 0: full kick, next drift into d_Xt.
 *           last != 0: half kick, H1, accept or reject (on accept U and grad U of the new point are kept: the next
 *           transition needs no evaluation), the step-size rule while t < n_warmup, t += 1, and, unless d_sample_out is
 *           NULL, the rows' current points q into d_sample_out (M, P).
 * One transition is n_leapfrog evaluations and n_leapfrog + 1 row launches; nothing has to be read back in between. */
long long pgl_hmc_state_doubles(int M, int P);
int pgl_hmc_init_dev(pgl_handle h, double* d_state, int M, int C, int P, int n_lo, double* d_ll, double* d_grad,
                     const pgl_prior* prior, double step0, uint64_t seed);
int pgl_hmc_begin_dev(pgl_handle h, double* d_state, int M, int P, const double* d_minv, double* d_Xt);
int pgl_hmc_leap_dev(pgl_handle h, double* d_state, int M, int P, const double* d_minv, double* d_ll, double* d_grad,
                     const pgl_prior* prior, int last, int n_warmup, double* d_Xt, double* d_sample_out);

/* Lock-step HMC with a DENSE mass matrix (inference/batched_hmc.py: mass = (M, P, P) or 'laplace_dense'; restated in
 * csrc/pglm_hmc_dense.h).  The inverse mass matrix of row m is Sigma_m = W_m W_m^T, d_W (M, P, P) row-major with W_m lower
 * triangular; only the entries j <= i are ever read (the strict upper triangle may hold anything).  The chain above runs
 * in the whitened momentum r = W^T p, which is standard normal: the state block is pgl_hmc_state_doubles(M, P) with r in
 * the place of p, pgl_hmc_init_dev starts it, and the random numbers, the target, the decision and the step-size rule are
 * those above:
 *     transition t:  r_j = z_j (the SAME draws as the diagonal chain);  H0 = U + 1/2 sum_j r_j^2;  r -= step/2 W^T grad U;
 *         n_leapfrog times { q += step W r;  r -= step W^T grad U(q) (step/2 the last time) };  H1 = U(q) + 1/2 sum_j r_j^2.
 * That is the algorithm above with M^-1 = Sigma; with W = diag(sqrt(minv)) it is the diagonal chain in exact arithmetic.
 *   pgl_tri_matvec_dev:  d_y (M, P) = W_m d_x[m] (trans == 0) or W_m^T d_x[m] (trans != 0), every row m; d_y != d_x.  All
 *           arithmetic in f64, no atomics; every output is summed in an order that depends on P alone, so a row of an
 *           M-row call equals the one-row call bit for bit and two calls give the same bits.  One launch on a grid of
 *           (tiles of 64 outputs, rows).
 *   begin:  the momentum draw and H0, then the half kick and the first drift as epilogues of the two products: three
 *           launches.  d_Xt (M, P) = the points to evaluate next.
 *   leap:   (d_ll, d_grad) = the evaluation at d_Xt (overwritten with U, grad U).  last == 0: the kick and the next drift,
 *           again inside the products: three launches.  last != 0: the half kick, then H1, accept or reject, the step-size
 *           rule while t < n_warmup, t += 1 and d_sample_out as pgl_hmc_leap_dev: three launches.
 * No product is ever stored, so the calls need no workspace.
 * One transition is n_leapfrog evaluations and 3 (n_leapfrog + 1) small launches; nothing has to be read back in between. */
int pgl_tri_matvec_dev(pgl_handle h, const double* d_W, int M, int P, int trans, const double* d_x, double* d_y);
int pgl_hmc_dense_begin_dev(pgl_handle h, double* d_state, int M, int P, const double* d_W, double* d_Xt);
int pgl_hmc_dense_leap_dev(pgl_handle h, double* d_state, int M, int P, const double* d_W, double* d_ll, double* d_grad,
                           const pgl_prior* prior, int last, int n_warmup, double* d_Xt, double* d_sample_out);

/* The No-U-Turn sampler for the same posteriors (inference/batched_nuts.py; the transition is restated in
 * csrc/pglm_nuts.h and, with its leaves in a list, in inference/nuts.py), as row kernels on the handle's stream: one
 * workgroup per neuron row, ONE pgl_ll_grad_dev of all rows per leapfrog step, and rows that do not wait for each other.
 * Multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017) in the whitened momentum r = W^T p, K = 1/2 sum r_j^2, the
 * inverse mass matrix of row m being W_m W_m^T:  d_W (M, P, P) lower triangular (only j <= i is read), or d_W NULL and
 * d_minv (M, P) (W = diag(sqrt(minv)), applied inside the row kernel), or both NULL (identity).
 *   target      U, its gradient, the priors and the non-finite rules of pgl_hmc_leap_dev.
 *   leapfrog    from an edge (q, r, h = W^T grad U(q)) in direction v:  r' = r - v eps/2 h;  q' = q + v eps W r';  one
 *               evaluation;  h' = W^T grad U(q');  r'' = r' - v eps/2 h'.  Every edge keeps (q, r, h): no second product.
 *   tree        doubling d = 0, 1, ... < max_depth (at most 10) draws a direction and builds 2^d leaves from that edge.
 *               The U-turn test  rho . r_first > 0 and rho . r_last > 0  (rho: the sum of r over the block; Euclidean in
 *               these coordinates) is applied to every aligned block of 2^k leaves of the new subtree, k >= 1, as soon as
 *               its last leaf exists, and to the whole tree after a merge; nothing else is cross-checked.  A U-turn or a
 *               divergence inside the new subtree discards the subtree and ends the transition; a U-turn of the merged
 *               tree or d + 1 = max_depth ends it after the merge.  'depth' counts the doublings begun.
 *   divergence  a leaf with non-finite H, or H - H0 > 1000: weight 0, and the transition is counted (t >= n_warmup).
 *   proposal    log weights H0 - H.  Leaf i of a subtree replaces the subtree's candidate iff i = 0 or
 *               log u < log w_i - log sum_{k<=i} w_k;  at a merge the subtree's candidate replaces the tree's iff
 *               log u < log w_subtree - log w_tree.
 *   storage     O(max_depth) vectors per row: an even leaf i checkpoints (r_i, the subtree's running rho before it) in
 *               slot popcount(i); the odd leaf i reads slot popcount(i) - k for each of its k = 1 .. trailing one bits.
 *               The candidate keeps (q, U, grad U, h): a new transition needs no evaluation.
 *   statistic   the mean over all leaves built in the transition of min(1, exp(H0 - H)), 0 for a divergent leaf.
 *   step size   per row, dual averaging (Hoffman & Gelman 2014, alg. 5) with delta = target_accept, gamma = 0.05, t0 = 10,
 *               kappa = 0.75, mu = log(10 step0), clipped to [1e-4, 10]; at t = n_warmup frozen at exp(log eps bar).
 *   random numbers  stateless: pgl_hmc's key (seed, neuron index, transition) and uniforms.  z_j: counters 2 j + 1,
 *               2 j + 2 (the momentum of the HMC chain);  direction of doubling d: 2 P + 1 + d (forward iff u < 1/2);
 *               merge uniform of doubling d: 2 P + 17 + d;  selection uniform of leaf i of doubling d:
 *               2 P + 33 + (2^d - 1 + i).  A chain over [n_lo, n_hi) equals the matching rows of a chain over all neurons.
 * d_state: pgl_nuts_state_doubles(M, P, max_depth) doubles = 17 + 2 max_depth (M, P) arrays -- the first is the rows'
 * current point -- then 30 (M) arrays of scalars, field-major (PglNuts of csrc/pglm_nuts.h: 2 step, 3 t, 7 done,
 * 21 leapfrog steps so far, 22 divergent transitions and 23 the sum of the statistic with t >= n_warmup, 24 - 28 depth,
 * leaves, stop reason (1 block U-turn, 2 tree U-turn, 3 max_depth, 4 divergence), selected leaf and statistic of the last
 * transition).  Every row runs n_warmup + n_keep thin transitions, counts its own t, writes its kept points into
 * d_samples (n_keep, M, P) and (depth, leapfrog steps) of the kept transitions into d_stats (n_keep, 2, M) (either may
 * be NULL), then sets done and idles with its d_Xt row left at its current point.
 *   pgl_nuts_init_dev:  C chains of M neurons ("chains" below; every array here then has C M rows, d_minv and d_W one per
 *           row).  The rows' points are the first array of d_state; d_ll (M), d_grad (M, P) hold ll and its gradient
 *           there (overwritten).  d_step0 (M): the starting steps.  Draws the first momentum; d_Xt = the first points to
 *           evaluate.  1 launch (diagonal), 4 (dense).
 *   pgl_nuts_step_dev:  after one evaluation of all rows at d_Xt: one leapfrog step of every row that is not done and
 *           d_Xt = the next points.  1 launch (diagonal); dense: 2 small launches and 2 products (pgl_tri_matvec_dev's
 *           kernel, the drift its epilogue). */
long long pgl_nuts_state_doubles(int M, int P, int max_depth);
int pgl_nuts_init_dev(pgl_handle h, double* d_state, int M, int C, int P, int max_depth, int n_lo, double* d_ll,
                      double* d_grad, const pgl_prior* prior, const double* d_minv, const double* d_W, const double* d_step0,
                      uint64_t seed, int n_warmup, int thin, int n_keep, double* d_Xt);
int pgl_nuts_step_dev(pgl_handle h, double* d_state, int M, int P, int max_depth, double* d_ll, double* d_grad,
                      const pgl_prior* prior, const double* d_minv, const double* d_W, double target_accept, int n_warmup,
                      int thin, int n_keep, double* d_Xt, double* d_samples, double* d_stats);

/* Several chains per neuron, and a diagonal mass matrix learned during the warm-up (inference/batched_hmc.py and
 * batched_nuts.py: n_chains, mass='adapt'; the rules are csrc/pglm_adapt.h, the host side inference/mass_adapt.py).
 *   chains      a run of C chains of the M neurons n_lo .. n_lo + M - 1 has R = C M rows, chain-major: row c M + m is chain
 *               c of neuron n_lo + m, so block c of any (R, P) array is the (M, P) theta block one pgl_ll_grad_dev(n_lo,
 *               n_lo + M) takes and returns.  Chain c runs on the seed  chain_seed(seed, c) = seed for c = 0, else
 *               mix(mix(seed + G) ^ (G c))  (64-bit; mix = pgl_hmc's finaliser, G = 0x9e3779b97f4a7c15), with the key
 *               (that seed, neuron index, transition): chain c equals the single-chain run with that seed, bit for bit.
 *               pgl_hmc_init_dev and pgl_nuts_init_dev set this up from (M, C); every other call of the chain takes M = R
 *               rows (d_minv (R, P), d_W (R, P, P): one per row).
 *   schedule    host side, from n = n_warmup (Stan's windowed adaptation):  n < 20: no window.  n >= 150: init = 75, term
 *               = 50, base = 25;  else init = floor(0.15 n), term = floor(0.10 n), base = n - init - term.  Windows start
 *               at init, have sizes base, 2 base, 4 base, ... and tile [init, n - term): a window is stretched to n - term
 *               unless its doubled successor would end before n - term.  d_sched (ints, on the device, uploaded once):
 *               [n_win, start of window 0, end of window 0, end of window 1, ...].
 *   estimate    per row and parameter a Welford count n, mean, M2 over the row's point q after every transition t of the
 *               running window (a rejected transition contributes the repeated point):  d = q - mean;  mean += d / n;
 *               M2 += d (q - mean).  After the transition with t + 1 = the window's end:  var = M2 / (n - 1);
 *               minv = n / (n + 5) var + 1e-3 * 5 / (n + 5)  (non-finite: 1);  the row of d_minv is rewritten, the
 *               accumulators are zeroed, and the row's step-size adaptation restarts -- HMC: avg_accept = 0.9, step kept;
 *               NUTS: mu = log(10 step), Hbar = 0, log eps bar = 0, and the iterate m of the dual averaging counts from the
 *               window's end (the averaged step is still taken at t = n_warmup).  After the last window d_minv is never
 *               written again.  A transition runs wholly under one minv: the switch falls between the end of transition
 *               t and the momentum draw of t + 1.
 * d_adapt: pgl_adapt_state_doubles(R, P) doubles, zeroed by the caller = mean (R, P), M2 (R, P), count (R), window index (R).
 * d_minv (R, P): ones at the start (the chain before the first window's end is the identity-mass chain, bit for bit).
 *   pgl_mass_adapt_dev:  HMC, one small launch after the last pgl_hmc_leap_dev of a transition and before the next
 *           pgl_hmc_begin_dev (which reads d_minv); needed only for transitions init <= t < the last window's end.
 *   pgl_nuts_adapt_step_dev:  pgl_nuts_step_dev for the diagonal chain, with the rules above applied inside the row kernel
 *           at the row's own transition boundary (rows are asynchronous), before the next momentum and edge are formed;
 *           h = sqrt(minv) o grad U of the current point is recomputed at a switch.  1 launch. */
long long pgl_adapt_state_doubles(int R, int P);
int pgl_mass_adapt_dev(pgl_handle h, double* d_state, int R, int P, double* d_adapt, const int* d_sched, double* d_minv);
int pgl_nuts_adapt_step_dev(pgl_handle h, double* d_state, int M, int P, int max_depth, double* d_ll, double* d_grad,
                            const pgl_prior* prior, double* d_minv, double* d_adapt, const int* d_sched, double target_accept,
                            int n_warmup, int thin, int n_keep, double* d_Xt, double* d_samples, double* d_stats);

/* Annealed importance sampling (Neal 2001; inference/batched_ais.py) of the evidence log Z_n of every neuron given the
 * network, as row kernels on the handle's stream, on top of the HMC moves above (restated nowhere: csrc/pglm_ais.h uses
 * csrc/pglm_hmc.h).  The run covers R = K M rows: K particles of the M neurons n_lo .. n_lo + M - 1, particle-major -- row
 * r = k M + i is particle particle0 + k of neuron n_lo + i -- so block k of any (R, P) array is the (M, P) theta block one
 * pgl_ll_grad_dev(n_lo, n_lo + M) takes and returns.  Over a ladder 0 = beta_0 < ... < beta_J = 1 the target is
 *     U_beta = -(beta ll + log prior),  grad U_beta = -(beta grad ll + grad log prior),  with the NaN rules above.
 * Only the Gaussian priors are served (pgl_prior kind 0, all standard deviations positive): the start is an exact draw
 * from the normalised prior.  kind 1 returns PGL_ERR_UNSUPPORTED.  Per row:
 *     1. q_j = m_j + s_j z_j;  evaluate;  log w = 0.
 *     2. for j = 1 .. J:  log w += (beta_j - beta_{j-1}) ll0, ll0 = ll at the current point -- the point that was sampled
 *        under beta_{j-1} (a non-finite ll0 makes log w = -inf for good);  then the target becomes U_{beta_j}.
 *     3. for j < J: transitions as above (n_leapfrog steps each) that leave prior x L^beta_j invariant.
 * Random numbers: the formulas above with a seed per particle,
 *     s_k  = mix(seed + G * (particle + 1))                            particle = particle0 + k;  -1 is allowed (a pilot)
 *     key  = mix(mix(mix(s_k + G) + G * (n + 1)) + G * (t + 1))          n: NEURON index, t: transition number
 *     t = 0: the prior draw, z_j of that key;  the moves are numbered t = 1, 2, ... across the whole ladder.
 * So a run over neurons [a, b) equals the matching rows of a run over [0, N), particles [k0, k0 + K) equal the matching
 * particles of a larger run, and two runs give the same bits.
 * Step sizes: one per row.  adapt != 0: the rule above after EVERY transition (weights of such a run are not valid; it is
 * how a pilot finds steps).  adapt == 0: a decision never changes the step; temper sets it from d_step_row.
 * d_minv (M, P), NULL = identity: the diagonal inverse mass, shared by the particles of a neuron.
 * All state of R rows lives in ONE device block of pgl_ais_state_doubles(R, P) doubles, in this order:
 *   (R,P) each: q (the current point), p, q0 (start of the running transition), g (grad U_beta at the current point), gll
 *               (grad ll at the current point), gu (grad U_beta along the running trajectory);
 *   (R) each:   U0 (U_beta at the current point), H0, step, avg_accept, n_accept (accepted transitions with adapt == 0), t
 *               (the next transition's number, from 1), acc (the last decision), neuron, seed_lo, seed_hi (halves of s_k),
 *               ll0, lp0 (log likelihood and log prior -- constants dropped -- at the current point), beta, logw, particle.
 *   init:   the prior draws into q and into d_Xt (R, P), the points to evaluate; log w = 0, beta = 0, every step = step0.
 *   start:  (d_ll (R), d_grad (R, P)) = the evaluation at the draws (left as they are): ll0, lp0, gll.
 *   temper: the weight increment for the change to beta, U0 and g of the new target from ll0, lp0, gll (no evaluation),
 *           and, unless d_step_row is NULL, step of row r = d_step_row[r mod M] (M entries, one per neuron).
 *   begin:  as pgl_hmc_begin_dev.
 *   leap:   (d_ll, d_grad) = the evaluation at d_Xt (left as they are).  last == 0: full kick, next drift into d_Xt.
 *           last != 0: half kick, H1, accept (ll, log prior, grad ll and grad U of the new point are kept) or reject,
 *           t += 1; d_acc_out[r] += the decision and d_step_out[r] = the row's step after it (R entries each; NULL: none).
 * One leapfrog step is K pgl_ll_grad_dev calls (one per particle block) and one row launch; nothing is read back. */
long long pgl_ais_state_doubles(int R, int P);
int pgl_ais_init_dev(pgl_handle h, double* d_state, int K, int M, int P, int n_lo, int particle0, const pgl_prior* prior,
                     double step0, uint64_t seed, double* d_Xt);
int pgl_ais_start_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_ll, const double* d_grad,
                      const pgl_prior* prior);
int pgl_ais_temper_dev(pgl_handle h, double* d_state, int K, int M, int P, const pgl_prior* prior, double beta,
                       const double* d_step_row);
int pgl_ais_begin_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_minv, double* d_Xt);
int pgl_ais_leap_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_minv, const double* d_ll,
                     const double* d_grad, const pgl_prior* prior, int last, int adapt, double* d_Xt, double* d_acc_out,
                     double* d_step_out);

/* Annealed importance sampling with a DENSE mass matrix (inference/batched_ais.py: mass = (M, P, P) or 'laplace_dense';
 * restated in csrc/pglm_ais_dense.h over csrc/pglm_ais.h and csrc/pglm_hmc_dense.h).  The inverse mass matrix of NEURON i is
 * Sigma_i = W_i W_i^T, d_W (M, P, P) row-major with W_i lower triangular, shared by the K particles of the neuron; only the
 * entries j <= i are ever read (the strict upper triangle may hold anything).  The run above goes on in the whitened
 * momentum r = W^T p: the state block is pgl_ais_state_doubles(R, P) with r in the place of p; pgl_ais_init_dev, _start_dev
 * and _temper_dev are used unchanged, and the random numbers, the target, the weights, the decision and the step-size rule
 * are those above:
 *     transition t:  r_j = z_j (the SAME draws as the diagonal run);  H0 = U_beta + 1/2 sum_j r_j^2;  r -= step/2 W^T grad U_beta;
 *         n_leapfrog times { q += step W r;  r -= step W^T grad U_beta(q) (step/2 the last time) };  H1, the decision.
 * With W = diag(sqrt(minv)) it is the diagonal run in exact arithmetic.  d_W may change between two transitions (a mass
 * per temperature): a mass that does not depend on the particle's state keeps every transition valid for its target.
 *   pgl_tri_matvec_shared_dev:  d_x, d_y (K M, P), particle-major; row r: d_y[r] = W_{r mod M} d_x[r] (trans == 0) or
 *           W_{r mod M}^T d_x[r] (trans != 0); d_y != d_x.  One launch on a grid of (tiles of 64 outputs, neurons): a
 *           workgroup produces its tile for all K particles from one read of its part of W (8 particles per pass; more are
 *           further passes inside the workgroup, any K).  f64, no atomics; every output is summed in the order of
 *           pgl_tri_matvec_dev, which depends on P alone: row (k, i) equals the one-row pgl_tri_matvec_dev call with W_i bit
 *           for bit, for any K and M, and two calls give the same bits.
 *   begin:  the momentum draw and H0, then the half kick and the first drift as epilogues of the two products: three
 *           launches.  d_Xt (R, P) = the points to evaluate next.
 *   leap:   (d_ll, d_grad) = the evaluation at d_Xt (left as they are).  last == 0: grad U_beta, then the kick and the next
 *           drift inside the products: three launches.  last != 0: grad U_beta, the half kick, then H1, accept or reject, the
 *           step-size rule if adapt, t += 1, d_acc_out and d_step_out as pgl_ais_leap_dev: three launches.
 * One leapfrog step is K pgl_ll_grad_dev calls and 3 small launches, whatever K is; nothing is read back.  A prior of
 * kind 1 returns PGL_ERR_UNSUPPORTED. */
int pgl_tri_matvec_shared_dev(pgl_handle h, const double* d_W, int M, int K, int P, int trans, const double* d_x, double* d_y);
int pgl_ais_dense_begin_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_W, double* d_Xt);
int pgl_ais_dense_leap_dev(pgl_handle h, double* d_state, int K, int M, int P, const double* d_W, const double* d_ll,
                           const double* d_grad, const pgl_prior* prior, int last, int adapt, double* d_Xt, double* d_acc_out,
                           double* d_step_out);

/* Adaptive sequential Monte Carlo (Del Moral, Doucet & Jasra 2006; ladder rule of Jasra et al. 2011 / Zhou, Johansen &
 * Aston 2016; inference/batched_smc.py) of the evidence log Z_n on the tempered path above, restated in csrc/pglm_smc.h over
 * csrc/pglm_ais.h.  The rows are the AIS rows (d_state: the pgl_ais_state_doubles(K M, P) block, r = k M + i, particles
 * 0 .. K - 1); every NEURON owns its temperature, its evidence, ONE step size shared by its K particles, and a done flag.
 * The estimate of Z is consistent, not unbiased as Neal's AIS is.  A stage of a neuron that is not done, with W_k the
 * normalised weights exp(logw_k) / sum (a particle with a non-finite ll0 or logw = -inf is dead: W_k = 0 for good):
 *   0. step rule (stages after the first): a = acceptances of the moves since the last stage / (K n_steps),
 *      step = clip(step exp(a - 0.9), 1e-3, 1).
 *   1. next temperature: CESS(d) = K (sum W_k v_k)^2 / sum W_k v_k^2, v_k = exp(d (ll0_k - max ll0)).  CESS(1 - beta) >=
 *      cess K: d = 1 - beta.  Else 60 halvings of [0, 1 - beta] towards CESS = cess K, d = the lower end.  d = max(d,
 *      delta_min); d >= 1 - beta: d = 1 - beta and beta = 1 exactly.
 *   2. log_Z += d max ll0 + log sum W_k v_k;  W_k = W_k v_k / sum W v, logw_k = log W_k.  No live particle: log_Z = -inf,
 *      the neuron is done and its rows stay as they are.
 *   3. resampling when ESS = 1 / sum W_k^2 < ess_min K: systematic with ONE uniform
 *          u = U_0 of key(mix(seed ^ 0x5eed5eed5eed5eed), n, stage)      n: NEURON index, stage: the stage's number from 0,
 *      key, mix and U_0 as above, u in (0, 1); with c_j = W_0 + ... + W_j summed in index order, anc[k] = the first j with
 *      c_j >= (u + k) / K (past the end by rounding: the last live particle); then logw = 0 for every slot.  Slot k takes q,
 *      gll, ll0, lp0 of slot anc[k], out of place through scratch; its seed, particle index, t and step stay with the
 *      slot, so copies of one particle diverge at their next momentum draw.
 *   4. beta, U0 and g of every row of the neuron from the kept parts at the new beta (no evaluation), step of the row =
 *      the neuron's.  beta = 1: done, no move follows.  Else n_steps transitions under the new target.
 * A done neuron never changes again: stage returns at once for it, and in the moves a row of a done neuron draws nothing,
 * moves nothing, advances no t, adds no acceptance and writes its current q to d_Xt.  Active rows have the bits of the
 * pgl_ais_* kernels on the same state.
 * d_smc: ONE device block of pgl_smc_state_doubles(K, M, P, S) doubles, S = the stage records kept per neuron, in this order:
 *   (M) each:      beta, log_Z, step, stage (completed stages), done, n_resampled, acc (acceptances the last stage summed),
 *                  live (the last stage call changed the neuron's rows), rs (it resampled), ess (before that resampling);
 *   (S, M) each:   records of stage s: beta after it, ESS before resampling, CESS, resampled (0 / 1), accept rate of the moves
 *                  that followed (NaN where none did), the step they ran on; NaN beyond a neuron's last stage;
 *   (R) each:      anc (ancestor particle of every row in the last stage), w (normalised weights after the last stage's update,
 *                  before its resampling), acc (acceptances of every row since the last stage);
 *   (1):           n_active, the neurons not done after the last stage call -- the one number a driver reads per stage;
 *   scratch:       (R, P), (R, P), (2, R): q, gll and ll0, lp0 on their way between slots.
 *   init:   pgl_ais_init_dev with particle0 = 0, and the start of d_smc (every step = step0).  Then pgl_ais_start_dev.
 *   stage:  steps 0 to 4 for every neuron, three launches: one workgroup per neuron (any K >= 1), then two of one workgroup
 *           per row (gather into scratch, scatter and retemper).  f64, no atomics, fixed summation order.
 *   gather: the last two launches of stage on their own, by what d_smc holds: a neuron with live != 0 is retempered to its
 *           beta and step, and where rs != 0 slot k first takes the kept parts of slot anc[k]; n_active is counted.
 *   begin / leap, dense_begin / dense_leap: pgl_ais_begin_dev / _leap_dev / pgl_ais_dense_begin_dev / _dense_leap_dev with
 *           adapt = 0, the guard above, and the decisions added into d_smc's acc. */
long long pgl_smc_state_doubles(int K, int M, int P, int S);
int pgl_smc_init_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, int n_lo, const pgl_prior* prior,
                     double step0, uint64_t seed, double* d_Xt);
int pgl_smc_stage_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const pgl_prior* prior,
                      int n_steps, double cess, double ess_min, double delta_min, uint64_t seed);
int pgl_smc_gather_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const pgl_prior* prior);
int pgl_smc_begin_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_minv,
                      double* d_Xt);
int pgl_smc_leap_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_minv,
                     const double* d_ll, const double* d_grad, const pgl_prior* prior, int last, double* d_Xt);
int pgl_smc_dense_begin_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_W,
                            double* d_Xt);
int pgl_smc_dense_leap_dev(pgl_handle h, double* d_state, double* d_smc, int K, int M, int P, int S, const double* d_W,
                           const double* d_ll, const double* d_grad, const pgl_prior* prior, int last, double* d_Xt);

/* Lock-step accelerated proximal gradient for the group-lasso MAP (inference/batched_prox.py) as row kernels on the
 * handle's stream: the theta rows [bias, w_stim (Ds), w_ir (N groups of B)] of M neurons n_lo .. n_lo + M - 1 at once, one
 * workgroup per row around ONE pgl_ll_grad_dev over all rows per call.  The objective of a row is F = f + h,
 *     f = -ll - log N(bias; mu_b, sg_b) - log N(w_stim; 0, stim_sigma), the bias and stimulus terms of pgl_bfgs_objective_dev.
 *         A non-finite f is +inf (a trial there fails); a NaN or infinite entry of its gradient becomes 0;
 *     h = (lam_r / sigma) sum_g |w_g - mu|_2, minus the group-lasso log prior of pgl_bfgs_objective_dev kind 1, with lam_r
 *         one number per row: d_lam (M), device.  lam_r = 0 and lam_r = +inf are served (+inf: every group ends at mu);
 *     prox_{t h}: w_g <- mu + (v_g - mu) max(0, 1 - t lam_r / (sigma |v_g - mu|)) group by group (0 when the norm is 0),
 *         bias and stimulus entries unchanged.  A shrunk group equals mu EXACTLY.
 * The algorithm is FISTA with backtracking (Beck & Teboulle 2009), restated in csrc/pglm_prox.h, which is compiled for the
 * host too.  From the extrapolated point y with (f_y, g_y) known, the trial z = prox_{t h}(y - t g_y) is evaluated; then
 *     1. sufficient decrease: f_z finite and f_z <= f_y + <g_y, z - y> + |z - y|^2 / (2 t) + 1e-12 max(1, |f_y|);
 *     2. failure: t <- t / 2, new trial; max_backtrack failures in one iteration end the row, status 2;
 *     3. pass, F_z > F_x and y != x: restart -- z is dropped, y = x, tk = 1, t <- 2 t, new trial from x at once;
 *     4. otherwise accept: xprev = x, x = z, g_x = g_z, iters += 1;
 *     5. KKT residual r at x: the largest of |g| over bias and stimulus entries, |g_g + (lam_r / sigma) (w_g - mu) /
 *        |w_g - mu||_inf over the non-zero groups, max(0, |g_g|_2 - lam_r / sigma) over the zero groups (w_g == mu);
 *     6. r <= gtol ends the row with status 0, iters == maxiter with status 1;
 *     7. tk' = (1 + sqrt(1 + 4 tk^2)) / 2, beta = (tk - 1) / tk'; beta = 0: y = x and the next trial goes out at once, else
 *        y = x + beta (x - xprev) is evaluated first (a non-finite f_y restarts from x, t kept).
 * What differs from the textbook: the function restart of step 3 (O'Donoghue & Candes 2015); the step doubles on a restart
 * and never grows otherwise; the first step is BFGS's, t = min(1, 1.01 / |g|_2); and the rounding allowance of test 1,
 * ten times the spread of ll between summation orders, without which the test fails on noise once |z - y|^2 / (2 t) is
 * below the rounding of f.  An iteration is two evaluations, one after a start or a restart.
 * Every sum over a row (<g_y, z - y>, |z - y|^2, the group norms, h, r) has a fixed order and uses no atomics: two runs give
 * the same bits, and a group norm is summed by one thread, so B need not divide the wave size.
 * All state of M rows of P parameters lives in ONE device block of pgl_prox_state_doubles(M, P) doubles, in this order:
 *   (M,P) each: x, xprev, y, g_x (grad f at x), g_y (grad f at y);
 *   (M) each:   f_x, F_x, f_y, t (the step), tk (the momentum parameter), iters (accepted steps), nfev (evaluations, the one
 *               before init included), nbt (failed trials of the running iteration), restarts, phase (0: d_Xt holds y,
 *               1: d_Xt holds the trial z, 2: ended), status, kkt (r at x), y_is_x, and the smallest margin of each kind of
 *               decision taken so far, relative to the compared quantities: m_sd (test 1, over max(1, |f_y|)), m_restart
 *               (test 3, over max(1, |F_x|)), m_zero (|1 - t lam_r / (sigma |v_g - mu|)| of a group), m_kkt (|r - gtol| / gtol).
 *   init:  x in the state, (d_ll, d_grad) = ll (M) and its gradient (M, P) at x (overwritten with f, grad f): y = x, tk = 1,
 *          the KKT test at x (maxiter <= 0 ends every row that fails it with status 1) and the first trial into d_Xt (M, P,
 *          not part of the state), phase 1.
 *   step:  (d_ll, d_grad) = the evaluation at d_Xt (overwritten with f, grad f): one call of the machine for every row
 *          that has not ended; d_Xt = the points to evaluate next.  An ended row keeps x in its row of d_Xt -- it is
 *          evaluated again, harmlessly -- and is never written again.
 * flags_out: NULL, or M doubles of pinned host memory into which every row a kernel has advanced writes its phase: the
 * driver reads it behind an event every few calls and never waits per iteration.
 * prior: kind must be 1 (else PGL_ERR_ARG); its lam is ignored, d_lam rules. */
long long pgl_prox_state_doubles(int M, int P);
int pgl_prox_init_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                      const double* d_lam, double gtol, int maxiter, double* d_Xt, double* flags_out);
int pgl_prox_step_dev(pgl_handle h, double* d_state, int M, int P, double* d_ll, double* d_grad, const pgl_prior* prior,
                      const double* d_lam, double gtol, int maxiter, int max_backtrack, double* d_Xt, double* flags_out);

/* convolve_with_basis(S, ibasis) (basis.py:201-236 via impulse.py:114-130):
 * fS_out (nT,N,B) row-major, float64. */
int pgl_features(pgl_handle h, double* fS_out);

/* seval(imp_model.I_imp) (impulse.py:58 / 308; gibbs.py:812-833):
 * I_imp_out (nT,N) row-major for impulse weights w (N,B). */
int pgl_impulse_currents(pgl_handle h, const double* w, double* I_imp_out);

/* Glm.get_state lam / I_net / I_bkgd for neuron n (glm.py:75-91, population.py:88-120).
 * theta_n is one row (P); Weff_col is column n of Weff (N).  Outputs (nT) or NULL. */
int pgl_state(pgl_handle h, int n, const double* theta_n, const double* Weff_col,
              double* lam_out, double* I_net_out, double* I_stim_out);

/* CollapsedGibbsNetworkColumnUpdate._glm_ll (gibbs.py:910-937): for each w[k],
 * ll_k = sum_t(-dt*lam + log(lam)*S[t,n_post]), lam = nlin(I_bias + I_stim[t] +
 * I_other[t] + w[k]*I_col[t]).  I_stim may be NULL.  Host arrays of nT. */
int pgl_ll_from_current(pgl_handle h, int n_post, double I_bias, const double* I_stim,
                        const double* I_other, const double* I_col, const double* w,
                        int K, double* ll_out);

/* Device-resident form of _precompute_vars + _precompute_other_current + _glm_ll
 * (gibbs.py:812-864, 910-937).  prepare: computes I_imp (all presynaptic columns)
 * and the total I_net for neuron n_post once.  ll: for presynaptic n_pre, removes
 * the current contribution aw_cur*I_imp[:,n_pre] (rank-1 downdate instead of the
 * reference's full gemv per pair) and evaluates ll at the K candidate weights. */
int pgl_gibbs_prepare(pgl_handle h, int n_post, const double* theta_n,
                      const double* Weff_col);
int pgl_gibbs_ll(pgl_handle h, int n_pre, double aw_cur, const double* w, int K,
                 double* ll_out);
/* After A[n_pre,n_post]*W[n_pre,n_post] changed by `delta` (gibbs.py:1044-1066 writes the
 * new sample into the state dict): I_net += delta * I_imp[:,n_pre] on the device. */
int pgl_gibbs_update(pgl_handle h, int n_pre, double delta);

/* The same collapsed-Gibbs inner loop for MANY columns per launch.  Given the rest of the state the
 * columns (A[:,n], W[:,n]) are conditionally independent -- the reference maps them over its engines
 * (parallel_gibbs.py:162-165, concatenate_parallel_updates 24-37) -- so one call serves one
 * (n_pre, n_post) pair of every listed column.
 *   prepare_all: theta (N,P) flat feature weights of all neurons, Weff (N,N); computes the total
 *     current I_stim + I_net of every post-synaptic neuron once (forward-only MFMA pass,
 *     gibbs.py:812-833 for all n_post) and keeps it, with theta, on the device.  Honours
 *     pgl_set_time_range (ll sums then run over [t_lo, t_hi)).
 *   ll_cols: for column c: n_post[c], n_pre[c], aw_cur[c] = current A*W of the pair, w[c*K .. c*K+K)
 *     candidate weights (K <= 16, e.g. the 10 Gauss-Hermite nodes + w = 0, gibbs.py:1002-1032);
 *     ll_out[c*K + k] as pgl_gibbs_ll.  The impulse weights of the pair are theta[n_post][1+Dstim+n_pre*B ..].
 *     explinear: f64 sums; the log1p(exp(-|x|)) term of bins with 12 <= |x| < 700 comes from the single-precision
 *     hardware exp (absolute error <= 6e-12 per bin; see PGL_OPT_GIBBS_KERNEL for the all-f64 kernel).
 *   update_cols: after A*W of pair c changed by delta[c]: I_net[:, n_post[c]] += delta[c]*I_imp (n_post distinct).
 *   currents: copy out bias-free total current I_stim + I_net of one neuron over the prepared range. */
int pgl_gibbs_prepare_all(pgl_handle h, const double* theta, const double* Weff);
int pgl_gibbs_ll_cols(pgl_handle h, int ncols, const int* n_post, const int* n_pre,
                      const double* aw_cur, const double* w, int K, double* ll_out);
int pgl_gibbs_update_cols(pgl_handle h, int ncols, const int* n_post, const int* n_pre,
                          const double* delta);
int pgl_gibbs_currents(pgl_handle h, int n_post, double* x_out);

/* Time-rescaling goodness of fit (Brown, Barbieri, Ventura, Kass & Frank 2002): under the true model the integrated
 * intensity between consecutive spikes is Exp(1).  The reference has no counterpart; its result plots start from the
 * rates of eval_state (population.py:88-120), one neuron and three (nT) host arrays per pgl_state call.  For neuron n over
 * the handle's time range [t_lo, t_hi) (pgl_set_time_range is honoured):
 *     lam_t = nlin(theta_n[0] + x[t,n]), x the bias-free total current of pgl_gibbs_prepare_all, all f64 (no
 *             single-precision shortcut: the rate functions of the PGL_OPT_EPI_F64 = 1 epilogue);
 *     event bins t_1 < ... < t_K: the bins of the range with S[t,n] >= 1 -- a bin with several spikes is ONE event
 *             (pgl_rescale applies no discrete-time correction; pgl_rescale_corr below does);
 *     tau_k = dt * sum_{s = t_{k-1}+1 .. t_k} lam_s, k = 2 .. K: the interval before the first event of the range is
 *             left-censored and dropped, so a neuron with K events gives max(K - 1, 0) intervals;
 *     Lambda_n = dt * sum_{t in range} lam_t, the expected count.
 * rescale_count: off_out (N + 1), host: off_out[n] = position of neuron n's first interval in the concatenated output,
 *     off_out[N] = their number, for the current time range (from the host copy of the event lists; needs spikes only).
 * rescale_dev:   device pointers, asynchronous on the handle's stream.  d_theta (N, P), d_Weff (N, N): the forward pass of
 *     pgl_gibbs_prepare_all runs on them (and leaves its state, as that call does); d_off (N + 1) int64: the offsets of
 *     rescale_count; d_tau (d_off[N], at least one double): tau of neuron n at d_off[n] ..; d_stats (N, 4): Lambda_n, K_n,
 *     the number of event bins holding more than one spike, 0 (reserved).  A segmented sum over time behind the forward
 *     launches (k_rescale_chunk / _scan / _finish: one read of the currents, no (nT, N) rate array), every sum in a fixed
 *     order: two calls give the same bits.
 * rescale:       the same with host pointers; tau_out holds off[N] doubles, stats_out (N, 4).
 * Before pgl_set_spikes_* / pgl_set_basis: PGL_ERR_STATE; a NULL argument: PGL_ERR_ARG. */
int pgl_rescale_count(pgl_handle h, int64_t* off_out);
int pgl_rescale_dev(pgl_handle h, const double* d_theta, const double* d_Weff, double* d_tau, const int64_t* d_off,
                    double* d_stats);
int pgl_rescale(pgl_handle h, const double* theta, const double* Weff, double* tau_out, double* stats_out);

/* The same intervals with the discrete-time correction of Haslinger, Pipa & Brown (2010).  The model is Poisson per bin,
 * P(event in bin s) = 1 - exp(-q_s) with q_s = dt lam_s, so Haslinger's q = -log(1 - p) is the term the sum above holds
 * already, and only the event bin's own term changes -- the event lies somewhere inside its bin, not at its end:
 *     open_k = dt * sum_{s = t_{k-1}+1 .. t_k - 1} lam_s      the bins strictly between the two events (none: 0)
 *     q_k    = dt * lam_{t_k}
 *     e_k    = -log1p(u_k * expm1(-q_k))                       in (0, q_k]
 *     tau'_k = open_k + e_k
 * with the stateless uniform (G and mix as in pgl_simulate_streams below, the draw where that has the replicate)
 *     z = mix(mix(mix(mix(seed + G) + G * (draw + 1)) + G * (n + 1)) + G * (j + 1))
 *     u = ((double)(z >> 11) + 0.5) * 2^-53                                                  in (0, 1]
 * n: NEURON index, j: the index of the event t_k in the neuron's whole event list of the data sequence -- not in the time
 * range, so the interval between two given events has the same u whatever pgl_set_time_range says.  The corrected
 * intervals, and every statistic of them, are therefore a RANDOM function of seed (and draw): average over seeds, or
 * report the seed.  At lam dt << 1, e_k -> u q_k and the correction vanishes with the bias it removes; at lam dt = 0.2 ..
 * 0.5 the uncorrected KS distance of a true model is about 0.2 and fails every test (README.md, "Goodness of fit").
 * open_k is summed in the pieces tau_k is made of, on chunks of 256 bins that lie on the ABSOLUTE bin grid (multiples of
 * 256 from bin 0 of the data sequence; the first and last chunk of a range may be partial): the sum behind the earlier
 * event to the end of its chunk, the chunks strictly between the two events total by total in chunk order, the sum from
 * the start of the later event's chunk up to its bin (one sum between the two events where they share a chunk).  Every
 * in-chunk sum starts anew behind an event, so open_k is never a difference -- not tau_k - q_k, not two running sums --
 * and consecutive event bins give open_k = 0 exactly.  The rate of these pieces and of q_k is pgl_rescale's arithmetic with
 * the log1p series of the explinear rate chosen from the element's own current: pgl_rescale chooses it by a vote of the 64
 * lanes of a wavefront (other neurons, other chunks -- and which chunks share a wavefront changes with t_lo), which can move
 * the last bit of a rate.  Two calls give the same bits, and ANY sub-range gives, bit for bit, the intervals of the whole
 * range that lie wholly inside it, for both nonlinearities.  d_stats equals pgl_rescale_dev's bit for bit (column 3
 * stays 0): a range whose t_lo is a multiple of 256 shares that call's chunks (one read of the currents: k_rcorr_chunk,
 * k_rescale_scan, k_rcorr_finish); a range that starts inside a chunk takes the expected count from that call's own
 * chunk and scan launches first (k_rescale_chunk, k_rescale_scan, k_rcorr_chunk, k_rcorr_finish: a second read, for such
 * ranges only).
 * Arguments and errors as pgl_rescale_dev / pgl_rescale; draw < 0: PGL_ERR_ARG.  (Rule and host mirror: csrc/pglm_gof.h.) */
int pgl_rescale_corr_dev(pgl_handle h, const double* d_theta, const double* d_Weff, uint64_t seed, int64_t draw, double* d_tau,
                         const int64_t* d_off, double* d_stats);
int pgl_rescale_corr(pgl_handle h, const double* theta, const double* Weff, uint64_t seed, int64_t draw, double* tau_out,
                     double* stats_out);

/* Kolmogorov-Smirnov distance of segmented samples of rescaled intervals from Exp(1).  Segment m is
 * tau[off[m] .. off[m+1]) (off: M + 1 non-decreasing int64 from 0; lengths from 0 up), n its length:
 *     z_i = -expm1(-tau_i);  with z sorted ascending  D+ = max_p ((double)(p + 1) / (double)n - z_(p)),
 *     D- = max_p (z_(p) - (double)p / (double)n), p from 0;  D = max(D+, D-);
 *     n < 2: the three distances are NaN;  any tau_i that is NaN or negative: NaN as well (n is still reported, the
 *     segment's part of zsorted is then unspecified);  tau = +inf is legal (z = 1).  Offsets that decrease give a segment
 *     of negative length: NaN distances and that length in n, nothing read or written for it (the device entry does not
 *     read the offsets; pgl_ks_uniform checks them on the host).
 * ks (M, 4) = D, D+, D-, n per segment.  zsorted (the length of tau; may be NULL): every segment's z, sorted.  The sort is a
 * fixed compare-exchange network (one workgroup per segment, k_ks_segment): its running time does not depend on the
 * values (recorded as k_ks_segment under PGL_OPT_RECORD_KERNELS, appended to the record), the maxima and the sorted values do not depend on how ties fall, a segment gives the same bits alone or among
 * others, and given the same z the result equals numpy's max((arange(1, n + 1) / n - z).max(), (z - arange(0, n) / n).max())
 * bit for bit.
 * ks_uniform_dev: device pointers, asynchronous on the handle's stream when d_zsorted is given; with d_zsorted = NULL the
 *     call waits once for the stream to read off[M] and sorts in a buffer of the handle.  The handle supplies device and
 *     stream only: no data set is needed.
 * ks_uniform:     the same with host pointers.
 * M < 1 or a NULL tau / off / ks: PGL_ERR_ARG. */
#define PGL_KS_NOUT 4
int pgl_ks_uniform_dev(pgl_handle h, const double* d_tau, const int64_t* d_off, int64_t M, double* d_ks, double* d_zsorted);
int pgl_ks_uniform(pgl_handle h, const double* tau, const int64_t* off, int64_t M, double* ks_out, double* zsorted_out);

/* Independence of the rescaled intervals: the serial correlation of their normal scores at the lags 1 .. max_lag and a
 * portmanteau statistic over the lags (the second half of the time-rescaling check; the KS distance above tests the marginal
 * law only).  A SEGMENT is one neuron and is made of RUNS, one per data sequence: intervals of one run are consecutive in
 * time, intervals of different runs are not neighbours.
 *     run_off (R + 1 int64, non-decreasing from 0): run r is tau[run_off[r] .. run_off[r+1]);
 *     seg_run (M + 1 int64, non-decreasing from 0): segment m holds the runs seg_run[m] .. seg_run[m+1];
 *     n = the segment's number of intervals.  Empty runs and empty segments are legal.
 * Score:  z = -expm1(-tau), q = z - 1/2.  |q| <= 0.425: Wichura's AS 241 (PPND16), central branch, on q -- evaluated as
 *     -expm1((LN2_HI - tau) + LN2_LO) / 2 (the two halves of log 2 as doubles), the same number without the cancellation at
 *     the median; the branch is chosen on the plain z - 0.5.  Otherwise the tail branch on r = z (q < 0) or r = exp(-tau)
 *     (q > 0: the upper tail directly, not 1 - z), r clamped below at DBL_MIN: tau = 0, a subnormal tau and tau = +inf give
 *     finite scores of magnitude about 37.5.  The coefficients are those of pgl_chain_diag's scores.
 * Statistics:  m = (sum g_i) / n, d_i = g_i - m, c_0 = sum d_i^2; c_k = sum d_i d_{i+k} over the pairs whose two members lie
 *     in the same run, n_k their number; r_k = c_k / c_0; v_k = n_k / (n (n + 2));  Q = sum over the lags with n_k >= 1 of
 *     r_k^2 / v_k in ascending k (one run: Ljung-Box), dof = the number of those lags.  n_k = 0: r_k = NaN, left out of Q.
 *     Under independence Q is approximately chi-square with dof degrees of freedom and r_k lies within z_{1-a/2} sqrt(v_k).
 * Order of the sums (part of the rule): every sum runs over the segment's index i, cut into pieces of 256 consecutive i
 *     counted from the segment's FIRST element; inside a piece the terms are added in ascending i, invalid pairs skipped;
 *     the piece totals are added in ascending piece order; every product and every sum is rounded on its own (no fused
 *     multiply-add).  The bits depend neither on the launch, nor on M, the other segments or max_lag: r_k is the same
 *     number whatever max_lag >= k is, and a segment gives the same bits alone or among others.
 * Voids:  any tau of the segment NaN or negative: every output but n is NaN.  n < 3 or c_0 == 0: r and Q are NaN, dof = 0.
 * out (M, PGL_ACF_NHEAD + max_lag) = n, mean, c_0, Q, dof, 0 (reserved), r_1 .. r_max_lag per segment.
 * scores (the length of tau): every g_i, the kernel's working array (required by the device entry; NULL allowed on the host).
 * One workgroup per segment (k_acf_segment, recorded under PGL_OPT_RECORD_KERNELS like k_ks_segment); its running time does
 * not depend on the values.  The device entry is asynchronous on the handle's stream and does not read the offsets; the host
 * entry checks them (a decreasing one: PGL_ERR_ARG).  The handle supplies device and stream only.
 * max_lag outside 1 .. PGL_ACF_MAX_LAG, M < 1, a NULL tau / run_off / seg_run / out (/ d_scores): PGL_ERR_ARG.
 * (Rule and host mirror: csrc/pglm_acf.h.) */
#define PGL_ACF_MAX_LAG 64
#define PGL_ACF_NHEAD 6
int pgl_rescale_acf_dev(pgl_handle h, const double* d_tau, const int64_t* d_run_off, const int64_t* d_seg_run, int64_t M,
                        int max_lag, double* d_out, double* d_scores);
int pgl_rescale_acf(pgl_handle h, const double* tau, const int64_t* run_off, const int64_t* seg_run, int64_t M, int max_lag,
                    double* out, double* scores_out);

/* Pointwise log-likelihood of a parameter draw, resolved in time, and its accumulation over posterior draws for WAIC
 * (Watanabe 2010; Vehtari, Gelman & Gabry 2017) and held-out predictive densities.  The reference computes the held-out
 * density with a callback per Gibbs sample (test/parallel_mcmc.py:59-90) and has no pointwise criterion.  For neuron n over
 * the handle's time range [t_lo, t_hi) (pgl_set_time_range is honoured):
 *     term_t = -dt * lam_t + S[t,n] * log lam_t,  lam_t = nlin(theta_n[0] + x[t,n]), x the bias-free total current of
 *             pgl_gibbs_prepare_all; all f64 (the rate function of pgl_rescale); log lam = the current itself for the exp
 *             nonlinearity; a bin with S = 0 contributes -dt * lam only (never 0 * log 0).  Spike counts come from the
 *             event lists.
 *     chunk   256 consecutive bins, counted from t_lo; the last one may be short;
 *     block   block_chunks >= 1 consecutive chunks, counted from the first; the last one may be short:
 *             n_blocks = ceil(nchunks / block_chunks); a block_chunks >= nchunks gives one block, the ll of the range;
 *     ll_blk[b][n] = sum of term_t over the bins of block b.  Given the spike history the likelihood factorises over bins,
 *             so the block sums are conditionally independent pointwise terms.
 *     accumulator over draws, per (block, neuron) four doubles in planes (4, n_blocks, N) -- m, e, mean, M2 -- by the rule of
 *             theano_pyglm_amd/csrc/pglm_pointwise.h:  draw 0 sets m = l, e = 1, mean = l, M2 = 0 (the caller need not
 *             clear the state); draw s >= 1:  l > m: e = e exp(m - l) + 1, m = l;  else e += exp(l - m);  d = l - mean;
 *             mean += d / (s + 1);  M2 += d (l - mean).  After S draws log mean_s exp(l_s) = log(e / S) + m and the sample
 *             variance is M2 / (S - 1).  A non-finite l makes the four values of that (block, neuron) NaN for good and
 *             touches nothing else.
 * pointwise_count: n_blocks_out (host) for the current time range.
 * pointwise_dev:   device pointers, asynchronous on the handle's stream.  d_theta (N, P), d_Weff (N, N): the forward pass of
 *     pgl_gibbs_prepare_all runs on them (and leaves its state, as that call does); d_ll_blk (n_blocks, N) out, or NULL;
 *     d_acc (4, n_blocks, N) in/out, or NULL; at least one of the two; draw = the index s of this draw for d_acc.  Two
 *     launches behind the forward ones (k_pw_chunk: one read of the currents, no (nT, N) array; k_pw_block), every sum in a
 *     fixed order and no atomics: two calls give the same bits.
 * pointwise:       host pointers, ll_blk_out (n_blocks, N).
 * Stimulus forms and errors as pgl_rescale_dev; block_chunks < 1, draw < 0 or both outputs NULL: PGL_ERR_ARG. */
int pgl_pointwise_count(pgl_handle h, int block_chunks, int64_t* n_blocks_out);
int pgl_pointwise_dev(pgl_handle h, const double* d_theta, const double* d_Weff, int block_chunks, double* d_ll_blk,
                      double* d_acc, int64_t draw);
int pgl_pointwise(pgl_handle h, const double* theta, const double* Weff, int block_chunks, double* ll_blk_out);

/* Expected and observed spike counts over time windows, and their accumulation over posterior draws: the firing rate of every
 * neuron with its posterior band, and windowed predictive residuals.  The reference draws the rate with a +-2 sd band over the
 * samples from the averaged eval_state dicts (pyglm/plotting/plot_results.py: plot_firing_rate(s_glm, s_glm_std);
 * population.py:88-120: one neuron and three (nT) host arrays per call, per draw).  For neuron n over the handle's time range
 * [t_lo, t_hi) (pgl_set_time_range is honoured):
 *     window  win >= 1 consecutive bins, counted from t_lo; the last one may be short: n_win = ceil((t_hi - t_lo) / win).  win
 *             is unrelated to the 256-bin chunk grid of pgl_rescale / pgl_pointwise: 1, 10, 50, 256, 300 and any win >= the
 *             range (one window) are all valid.
 *     Lam[w][n] = dt * sum_{t in window w} lam_t,  lam_t = nlin(theta_n[0] + x[t,n]), x the bias-free total current of
 *             pgl_gibbs_prepare_all; all f64, the rate function of pgl_rescale and pgl_pointwise except that every element
 *             picks the series of its own argument (theirs is picked by a vote of the wavefront, which would let a window's
 *             last bit depend on its neighbours).  The order of the sum is fixed (theano_pyglm_amd/csrc/pglm_ratewin.h) and does
 *             not depend on the launch geometry: the window is cut into pieces of at most 256 bins counted from the window's
 *             own first bin, a piece is summed in ascending time, the pieces are added in ascending order, dt multiplies
 *             last.  No atomics: two calls give the same bits, and a window gives the same bits whatever the other windows
 *             and neurons are.
 *     obs[w][n] = the sum of the spike counts of the event lists over the window's bins (a bin with several spikes counts
 *             them all), as a double.
 *     accumulator over draws, per (window, neuron) five doubles in planes (PGL_RW_NACC = 5, n_win, N) -- mean, M2, min, max,
 *             pit -- by the rule of pglm_ratewin.h:  draw 0 sets mean = min = max = Lam, M2 = 0, pit = u (the caller need not
 *             clear the state); draw s >= 1:  d = Lam - mean;  mean += d / (s + 1);  M2 = fma(d, Lam - mean, M2);  min, max;
 *             pit += (u - pit) / (s + 1), where u = F(y - 1) + 0.5 f(y) is the mid-p value of y = obs under a Poisson law of
 *             mean Lam: term_0 = exp(-Lam), term_k = term_{k-1} * Lam / k, summed ascending.  u is NaN if Lam > 700 or
 *             y > PGL_RW_MAX_COUNT (1024): the pit plane of that entry then stays NaN, the other four planes are not
 *             affected.  A non-finite Lam makes all five planes of that (window, neuron) NaN for good and touches nothing else.
 *     pit is the posterior mean of the one-step-ahead predictive probability of the observed window count GIVEN THE OBSERVED
 *             HISTORY: the currents come from the recorded spikes.  It is exact for win = 1; for longer windows it is an
 *             approximation, because spikes inside the window feed back into the rate of its later bins.
 * rate_windows_count: n_win_out (host) for the current time range.
 * rate_windows_dev:   device pointers, asynchronous on the handle's stream.  d_theta (N, P), d_Weff (N, N): the forward pass of
 *     pgl_gibbs_prepare_all runs on them (and leaves its state, as that call does); d_lam (n_win, N) out, or NULL; d_obs
 *     (n_win, N) out, or NULL; d_acc (5, n_win, N) in/out, or NULL; at least one of the three; draw = the index s of this
 *     draw for d_acc.  Two launches behind the forward ones (k_rw_piece: one read of the currents, no (nT, N) array;
 *     k_rw_window).
 * rate_windows:       host pointers, lam_out and obs_out (n_win, N).
 * Stimulus forms as pgl_rescale_dev.  win < 1, draw < 0, all three outputs NULL or a NULL d_theta / d_Weff: PGL_ERR_ARG; n_win
 * or the number of pieces times the neurons (padded to 16) beyond 2^31 - 1: PGL_ERR_UNSUPPORTED, nothing launched (a property
 * of the shape: answered before the state of the handle); before pgl_set_spikes_* / pgl_set_basis: PGL_ERR_STATE. */
#define PGL_RW_NACC 5
#define PGL_RW_MAX_COUNT 1024
int pgl_rate_windows_count(pgl_handle h, int64_t win, int64_t* n_win_out);
int pgl_rate_windows_dev(pgl_handle h, const double* d_theta, const double* d_Weff, int64_t win, double* d_lam, double* d_obs,
                         double* d_acc, int64_t draw);
int pgl_rate_windows(pgl_handle h, const double* theta, const double* Weff, int64_t win, double* lam_out, double* obs_out);

/* PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao &
 * Gabry 2024) of the columns of a matrix ll (S, C), element [s, c] at s * ld + c: column c holds the pointwise term of one
 * (block, neuron) under the S posterior draws -- the matrix pgl_pointwise_dev writes draw after draw.  The reference has no
 * pointwise criterion.  The rule of one column l_0 .. l_{S-1} (theano_pyglm_amd/csrc/pglm_psis.h):
 *   ratios    r_s = -l_s, x_s = r_s - max r;
 *   order     on the raw doubles l_s, before any arithmetic: descending l, ties by the draw index (smaller first);
 *   tail      M = ceil(min(S / 5, 3 sqrt(S))); the cutoff element has rank S - M - 1 (0-based), x_cut = max(its x,
 *             log(DBL_MIN)); the tail = the n <= M elements whose raw l is strictly smaller than the cutoff element's;
 *   n < 5     khat = +inf and nothing is smoothed;
 *   fit       generalized Pareto law on the excesses e_i = exp(x_tail,i) - exp(x_cut), ascending, by Zhang & Stephens (2009)
 *             as loo / ArviZ state it: m = 30 + floor(sqrt(n)) candidates b_i = 1 / e_n + (1 - sqrt(m / (i - 0.5))) /
 *             (3 e_q), q = floor(n / 4 + 0.5);  k_i = mean log1p(-b_i e);  L_i = n (log(-b_i / k_i) - k_i - 1);
 *             w_i = 1 / sum_j exp(L_j - L_i), those below 10 DBL_EPSILON dropped, the rest renormalised;  b = sum w_i b_i;
 *             k = mean log1p(-b e);  sigma = -k / b;  khat = (n k + 5) / (n + 10);
 *   smooth    (khat finite) the tail element of rank i of n:  x = log(exp(x_cut) + sigma expm1(-khat log1p(-p_i)) / khat),
 *             p_i = (i - 0.5) / n; the limit -sigma log1p(-p_i) for |khat| < DBL_EPSILON;
 *   weights   every x truncated at 0;  lw_s = x_s - logsumexp(x)  (shifted by max x);
 *   out       planes (PGL_PSIS_NOUT = 4, C):  elpd = log sum_s exp(lw_s + l_s) (shifted by its maximum), khat,
 *             n_eff = 1 / sum_s exp(2 lw_s), the tail length n.
 *   A column that holds a NaN or an infinite l gives four NaNs (and NaN weights) and touches no other column.
 * Every sum has a fixed order (pglm_psis.hip.h) and nothing is atomic: two calls give the same bits, and a column gives the
 * same bits alone and among others.  One workgroup per column, the column in LDS: S <= PGL_PSIS_MAX_DRAWS (4096).
 * psis_loo_dev: device pointers, asynchronous on the handle's stream; needs no data on the handle.  d_out (4, C); d_lw the log
 *     weights (S, C) at the same ld, or NULL.  d_lw must not overlap d_ll.
 * psis_loo:     host pointers, ll (S, C) and lw (S, C) or NULL contiguous, out (4, C).
 * S < 2, C < 1, ld < C or a NULL pointer: PGL_ERR_ARG;  S > PGL_PSIS_MAX_DRAWS: PGL_ERR_UNSUPPORTED. */
#define PGL_PSIS_NOUT 4
#define PGL_PSIS_MAX_DRAWS 4096
int pgl_psis_loo_dev(pgl_handle h, const double* d_ll, int64_t S, int64_t C, int64_t ld, double* d_out, double* d_lw);
int pgl_psis_loo(pgl_handle h, const double* ll, int64_t S, int64_t C, double* out, double* lw);

/* Wald statistics of the coupling groups from the factor of the Laplace covariance: which couplings are there (the per-pair
 * Granger-causality test of Kim, Putrino, Ghosh & Brown 2011 in its Wald form; inference/connectivity.py: coupling_tests).
 * The reference has no such test.  d_W (M, P, ld): row m lower triangular with W_m W_m^T = A_m^-1, as laplace_from_factor
 * leaves it; only the entries j <= i are read (the strict upper triangle and the columns P .. ld-1 may hold anything).
 * d_theta (M, P); group g of a row is the B entries from o = first + g B (theta rows [bias, w_stim (Ds), w_ir (N groups of B)]:
 * first = 1 + Ds, G = N); d_c (B) a contrast.  For every row and group
 *     S = W_g W_g^T  (the group's B x B block of the covariance),  y = S^-1 w_g  by an unpivoted Cholesky factorisation,
 *     T = w_g^T y,  lin = c^T w_g,  var = c^T S c
 * and d_out (M, G, PGL_WALD_NOUT) = T, lin, var, info: info = 0, or a + 1 for the first pivot a of S that is not finite or
 * <= 0 -- then T, lin and var of that group alone are NaN.  Under H0: w_g = 0 and the quadratic approximation T is chi-square
 * with B degrees of freedom.  d_u: NULL, or (G M, P) with row g M + m (the particle-major order of pgl_tri_matvec_shared_dev
 * with K = G) = W_g^T y, zero from column o + B on: theta_m - W_m u is the restricted one-step point with group g at
 * zero.  Whole rows are written; a group with info != 0 has NaN in the columns below o + B.  d_info (M) int32 as
 * pgl_chol_factor_dev leaves it: a row with d_info[m] != 0 gets NaN in d_out (and d_u) and its W and theta are not read.
 * The order of every sum is part of the rule (csrc/pglm_wald.h: columns by lane k mod 64, ascending, a binary tree over the
 * lanes, no fused multiply-add) and depends on (o, B) alone: a group gives the same bits alone or among others, two calls
 * give the same bits, and the gcc build of the rule (tests/csrc/wald_host.c) gives the device's bits.
 * One wave per group, four groups per workgroup, on a grid of (blocks of groups, rows) (k_wald_groups<B>): the group's rows of
 * W are read once along the rows for S; with d_u they are read a second time by the same wave.  f64 throughout, no atomics,
 * no scratch, asynchronous on the handle's stream; the handle supplies device and stream only.
 * M, G, B <= 0, ld < P, first < 0, first + G B > P or a NULL pointer other than d_u: PGL_ERR_ARG;  B > PGL_WALD_MAX_B or
 * M > 65535: PGL_ERR_UNSUPPORTED.
 * wald_groups: the same with host pointers, W (M, P, ld), u (G M, P) or NULL. */
#define PGL_WALD_MAX_B 16
#define PGL_WALD_NOUT 4
int pgl_wald_groups_dev(pgl_handle h, const double* d_W, int M, int P, int ld, const double* d_theta, int first, int G, int B,
                        const double* d_c, const int* d_info, double* d_out, double* d_u);
int pgl_wald_groups(pgl_handle h, const double* W, int M, int P, int ld, const double* theta, int first, int G, int B, const double* c,
                    const int* info, double* out, double* u);

/* Convergence diagnostics of posterior draws (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021): rank-normalised and folded
 * split-R-hat, bulk and tail effective sample size, the Monte-Carlo standard error of the mean, and the pooled moments and
 * quantiles, of every column of the tensor x (n, C, K) the lock-step samplers keep: draw i of chain c of column k (parameter p
 * of neuron m, k = m * P + p) at (i * C + c) * ld + k.  The reference has no convergence diagnostic.  The rule of one column
 * (theano_pyglm_amd/csrc/pglm_diag.h), S = C n pooled draws, every chain split into halves of h = n / 2 draws (the middle draw
 * of an odd n is in no half):
 *   ranks     on the raw doubles, ties averaged; order statistics from the ranks; quantiles by numpy.percentile's linear rule;
 *   scores    z = Phi^-1((rank - 3/8) / (S + 1/4)), Phi^-1 by Wichura's AS 241 (PPND16); folded: the scores of |x - median|;
 *   R-hat     sqrt(var+ / W) over the 2 C split chains (eqs. 1-4);
 *   ESS       biased autocovariances per split chain, rho_t = 1 - (W - mean acov[t]) / var+, Geyer's initial positive and
 *             monotone sequences on pairs, the final odd term, tau >= 1 / log10(N): ESS = N / tau, N = 2 C h.
 * out: PGL_DIAG_NOUT rows of K doubles, in this order:
 *    0 mean   1 sd (n - 1)   2 median   3 q025   4 q975   5 rhat_plain (the split-R-hat of x itself)
 *    6 rhat (the larger of the split-R-hats of z and of the folded scores)   7 ess_bulk (of z)
 *    8 ess_tail (the smaller of the ESS of I(x <= q05) and I(x <= q95))   9 ess_mean (of x)   10 mcse_mean = sd / sqrt(ess_mean)
 *   11 .. 14 the truncation lags of the ESS of z, I(x <= q05), I(x <= q95) and x.
 * A column that holds a NaN or an infinity gives PGL_DIAG_NOUT NaNs; a constant column gives its value as mean, median and
 * quantiles, sd = 0, every ESS and lag 0, and NaN R-hats and mcse_mean.  No column touches another.
 * Every sum has a fixed order (pglm_diag.hip.h) and nothing is atomic: two calls give the same bits, and a column gives the
 * same bits alone and among others.  One workgroup per column, the pooled column in LDS: C n <= PGL_DIAG_MAX_DRAWS (4096).
 * chain_diag_dev: device pointers, asynchronous on the handle's stream; needs no data on the handle.  d_out (PGL_DIAG_NOUT, K).
 * chain_diag:     host pointers, x (n, C, K) and out (PGL_DIAG_NOUT, K) contiguous.
 * n < 8, C < 1, K < 1, ld < K or a NULL pointer: PGL_ERR_ARG;  C n > PGL_DIAG_MAX_DRAWS: PGL_ERR_UNSUPPORTED, nothing launched. */
#define PGL_DIAG_NOUT 15
#define PGL_DIAG_MAX_DRAWS 4096
int pgl_chain_diag_dev(pgl_handle h, const double* d_x, int64_t n, int64_t C, int64_t K, int64_t ld, double* d_out);
int pgl_chain_diag(pgl_handle h, const double* x, int64_t n, int64_t C, int64_t K, double* out);

/* Posterior bands of the filters: the curves h(tau) = sum_b basis[tau, b] w_b of the groups of B weights of the theta rows,
 * summarised over the draws of a samplers' tensor d_samples (n_keep, C M, P) -- draw i of chain c of row m at
 * ((i C + c) M + m) P, pooled s = c n_keep + i as pgl_chain_diag pools them, S = C n_keep -- where it lies: the counterpart of
 * the reference's average_list_of_dicts / std_list_of_dicts over eval_state (utils/avg_dicts.py) for the curves
 * plot_imp_responses draws as mean +- 2 sd, plus quantiles and a simultaneous credible band.  Group g of a row is the B entries
 * from o = first + g B.  Theta rows are [bias, w_stim (D groups of B_stim, dimension-major), w_ir (N groups of B_imp,
 * presynaptic-neuron-major)]: the impulse responses are first = 1 + D B_stim, G = N, B = B_imp with the impulse basis, the
 * stimulus filters first = 1, G = D, B = B_stim with the stimulus basis.  d_basis (R, B) row-major; d_c (B) a contrast (the
 * effective weight: c_b = dt sum_t basis[t, b]); level in (0, 1).  The rule of one (row, group) is csrc/pglm_filters.h's:
 *   per lag   mean, sd (S - 1), and q_lo, median, q_hi at (1 - level) / 2, 1 / 2, (1 + level) / 2 by numpy.percentile's linear
 *             rule on the sorted values; a lag whose curve overflows in some draw is NaN;
 *   band      d_s = max over the lags with sd > 0 of |h_s - mean| / sd; c_sim = the ceil(level S)-th smallest d_s: at least a
 *             share `level` of the draws lies within mean +- c_sim sd at every lag at once;
 *   weight    omega_s = sum_b c[b] w_s[b]: its mean, sd and the three quantiles, and p_pos = #{omega_s > 0} / S.
 * d_out (M, G, R, PGL_FILT_NLAG) = mean, sd, q_lo, median, q_hi;  d_grp (M, G, PGL_FILT_NGRP) = c_sim, the five figures of
 * omega, p_pos, info.  info = 0, or 1 where a weight of the group is not finite in some draw: every other output of that group
 * alone is NaN.  Every sum has a fixed order (pieces of 256 consecutive draws, ascending, the pieces in order; no fused
 * multiply-add) that depends on (S, B, R, o) alone: a group gives the same bits alone or among others, two calls give the same
 * bits, and the gcc build of the rule (tests/csrc/filters_host.c) gives the device's bits.
 * One workgroup per (group, row) (k_filter_bands<B>): the group's weights are read once into LDS where they fit beside the
 * sort buffer (S B + next_pow2(S) <= 18 432 doubles) and re-read per lag through L2 otherwise; the S values of a lag are sorted
 * by a bitonic network in LDS.  f64 throughout, no atomics, no scratch, asynchronous on the handle's stream; the handle supplies
 * device and stream only.
 * n_keep, C, M, G, B, R <= 0, S < 2, first < 0, first + G B > P, level outside (0, 1) or a NULL pointer: PGL_ERR_ARG;
 * S > PGL_FILT_MAX_DRAWS, B > PGL_FILT_MAX_B or M > 65535: PGL_ERR_UNSUPPORTED; nothing is launched.
 * filter_bands: the same with host pointers, all arrays contiguous. */
#define PGL_FILT_MAX_B 16
#define PGL_FILT_MAX_DRAWS 4096
#define PGL_FILT_NLAG 5
#define PGL_FILT_NGRP 8
int pgl_filter_bands_dev(pgl_handle h, const double* d_samples, int64_t n_keep, int64_t C, int M, int P, int first, int G, int B,
                         const double* d_basis, int R, const double* d_c, double level, double* d_out, double* d_grp);
int pgl_filter_bands(pgl_handle h, const double* samples, int64_t n_keep, int64_t C, int M, int P, int first, int G, int B,
                     const double* basis, int R, const double* c, double level, double* out, double* grp);

/* Spike-triggered average, pyglm/utils/sta.py:6-85 (used by smart_init.py:28-98 and 100-158):
 *   A[i,l,d] = sum_t S[t,n_i] * istim[t-l,d] / sum_t S[t,n_i],  l = 0..L-1, terms with t-l < 0 dropped,
 * istim = np.interp of stim (Tstim,D) to the bin grid, divided by dt_stim/dt (sta.py:27-41).
 *   neurons: n_sel indices (NULL = all N);  A_out host (n_sel, L, D).  A silent neuron gives NaN
 *   like the reference's 0/0.  Uses the spike data already resident on the handle. */
int pgl_sta(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim, int L,
            const int* neurons, int n_sel, double* A_out);

/* Leading singular pair (u_0, sigma_0, v_0) of each of n (L x D) row-major matrices -- what initialize_stim_with_sta keeps of
 * np.linalg.svd(STA) (smart_init.py:66-72).  Host arrays: A (n, L, D) in; U (n, L), sigma (n), V (n, D) out; the
 * component of u_0 of largest magnitude is positive.  Device work with the library's own kernels (Gram matrix of the
 * smaller side, repeated squaring, two alternating steps on A).  A == NULL: the averages a preceding pgl_sta call with
 * A_out == NULL has left on the device (same n, L, D; consumed by this call) -- the initialisation of a wide stimulus never
 * moves its 157 MB of averages over PCIe. */
int pgl_leading_singular_pairs(pgl_handle h, const double* A, int n, int L, int D, double* U, double* sigma, double* V);
/* Degenerate matrices of a batch: a matrix of zeros returns sigma = 0 and zeros for both vectors (the start vector e_0 of
 * the zero Gram matrix does not survive the alternating steps: A e_0 = 0 stays unnormalised); a matrix that holds a NaN
 * returns NaN for sigma and in every component of both vectors.  Either touches no other matrix of the batch: every
 * matrix gets the bits it gets alone. */

/* One thin GEMM of the stimulus path on device operands, through the launchers the library itself uses (a test entry: it
 * lets each kernel be observed on its own, at its own tails):
 *   C[b][m scm + n scn] = sum_{k < K} A[b][m sam + k sak] * B[b][n sbn + k sbk],  m < M, n < N, b < batch,
 * strides in doubles, operand b at d_X + b sXb.  Nothing outside those M N batch elements of C is written.  Asynchronous on
 * the handle's stream; needs no data on the handle.  kernel picks the instantiation:
 *   PGL_GEMM_NT         k_gemm_nt: 64 x 64 tiles through LDS.  sak = sbk = scn = 1 (lda = sam, ldb = sbn, ldc = scm), batch = 1.
 *   PGL_GEMM_MFMA_1/_4  k_gemm_mfma<1> / <4>: any strides (0 broadcasts), any batch.
 *   PGL_GEMM_KC_4_1_8   k_gemm_kc<4, 1, 8>: both operands k-contiguous (sak = sbk = 1), d_A and d_B 16-byte aligned, sam and
 *                       sbn even, K even, batch = 1.
 *   PGL_GEMM_KC_1_0_16  k_gemm_kc<1, 0, 16>: A k-contiguous (sak = 1), 16-byte aligned, sam even; B n-contiguous (sbn = 1,
 *                       ldb = sbk); K even, batch = 1.
 * A precondition that does not hold, a NULL pointer, a negative stride, M, N, K or batch < 1: PGL_ERR_ARG, and nothing is
 * launched. */
#define PGL_GEMM_NT 0
#define PGL_GEMM_MFMA_1 1
#define PGL_GEMM_MFMA_4 2
#define PGL_GEMM_KC_4_1_8 3
#define PGL_GEMM_KC_1_0_16 4
int pgl_gemm_dev(pgl_handle h, int kernel, const double* d_A, int64_t sam, int64_t sak, int64_t sAb, const double* d_B,
                 int64_t sbn, int64_t sbk, int64_t sBb, double* d_C, int64_t scm, int64_t scn, int64_t sCb, int M, int N, int K,
                 int batch);

/* Population.simulate (population.py:233-389), native host implementation (no GPU needed):
 * integrate-and-fire thinning of the conditional intensity.  Per bin t: lam = nlin(X[t,:]),
 * acc += lam*dt, a neuron spikes while acc > thr (thr ~ Exp(1), redrawn after each spike,
 * population.py:321-360); every spike of n_pre adds AW[n_pre,:,n_post] to X[t+1 : t+R+1, n_post]
 * (351-353); at most 10 spikes per bin (345-349: the round that would exceed the cap is dropped).
 *   X     (nT,N) in/out: on entry bias + stimulus current (population.py:252-268), on exit the
 *         total current; S (nT,N) out, float64 counts.
 *   AW    (N, R, N) = A[n_pre,n_post]*W[n_pre,n_post]*impulse[n_pre->n_post][tau], layout
 *         [n_pre][tau][n_post].
 *   uniforms: optional stream of U(0,1) numbers consumed in the reference's draw order (N for the
 *         initial thresholds, then one per spiking neuron per round); when exhausted (or NULL) a
 *         splitmix64 generator seeded with `seed` continues.  n_exceptions_out may be NULL. */
int pgl_simulate(int N, int64_t nT, int R, int nlin, double dt, double* X, const double* AW,
                 const double* uniforms, int64_t n_uniforms, uint64_t seed, double* S,
                 int64_t* n_exceptions_out);

/* Batched simulation: many independent spike trains (replicates) of one model, one workgroup per replicate on the device.
 * The algorithm is pgl_simulate's; only the random numbers differ, because the reference's draw order (one draw per spiking
 * neuron per round, in neuron order, from ONE stream) is serial by construction.  Here every neuron of every replicate has a
 * stateless threshold stream of its own:
 *
 *     G      = 0x9e3779b97f4a7c15                                   (all arithmetic in uint64, wrapping)
 *     mix(z) : z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
 *     z      = mix(mix(mix(mix(seed + G) + G * (r + 1)) + G * (n + 1)) + G * (k + 1))
 *     u      = ((double)(z >> 11) + 0.5) * 2^-53                     (IEEE double operations, round to nearest)
 *     thr    = -log(u)
 *
 * is the k-th threshold of neuron n in replicate (stream index) r: k = 0 is the initial one and k increases by one
 * each time that neuron spikes.  u lies in (0, 1]: never 0; 1 (a zero threshold) once in 2^53 draws.  A neuron's
 * thresholds do not depend on what the other neurons do.
 * Per bin t: acc += nlin(X[t,:]) * dt; rounds while any acc > thr: S[t,n] += 1 for those neurons; a round that starts with some
 * S[t,n] >= 10 is dropped and counted as an exception (the check sits after the increment and before the scatter, as in
 * pgl_simulate); otherwise the spiking neurons' AW[n_pre,:,:] are added to X[t+1 : t+1+min(R, nT-t-1), :] in ascending
 * n_pre, acc -= thr (clamped at 0) and a new threshold is drawn.
 *
 * simulate_streams: host reference of one replicate (no GPU needed).  X (nT, N) in/out as in pgl_simulate; S (nT, N) uint8
 *     out; rep = the stream index r; closest_call_out (may be NULL) = the smallest |acc - thr| / thr over every comparison
 *     the run made -- how far the run stayed from a spike decision that a last-place difference could flip.
 * simulate_batch: replicates rep0 .. rep0 + n_rep - 1 on `device`; replicate i of a call uses stream index rep0 + i, so a
 *     batch equals its replicates run one at a time.  Host arrays: X0 (nT, N) bias + stimulus current shared by all
 *     replicates, AW (N, R, N) in the layout of pgl_simulate; S_out (n_rep, nT, N) uint8 and X_out (n_rep, nT, N) total
 *     currents may be NULL; counts_out (n_rep, N) spikes per neuron; exceptions_out (n_rep).  N <= 1024.
 *     The only state across bins is acc, thr and k per neuron and a ring of the next R bins of current (R x N doubles): in
 *     LDS when it fits, else in a per-replicate global workspace.  flags bit 0 forces the global ring.  All arithmetic f64;
 *     the sums have a fixed order: two calls give the same bits.
 * simulate_batch_dev: the same with device pointers, asynchronous on `stream` (hipStream_t as void*, NULL = the null
 *     stream); d_S / d_X may be NULL (counts alone come back); d_workspace holds n_rep * workspace_bytes_per_rep bytes and
 *     may be NULL when the ring is in LDS.
 * simulate_batch_plan: dry run of the ring placement (no GPU needed): ring_in_lds and the workspace bytes per replicate
 *     (R * N * 8 for the global ring, 0 for LDS).
 * Bad arguments: PGL_ERR_ARG; no visible device: PGL_ERR_HIP as pgl_create. */
int pgl_simulate_streams(int N, int64_t nT, int R, int nlin, double dt, double* X, const double* AW, int rep,
                         uint64_t seed, uint8_t* S, int64_t* n_exceptions_out, double* closest_call_out);
int pgl_simulate_batch(int device, int N, int64_t nT, int R, int nlin, double dt, const double* X0, const double* AW,
                       int n_rep, int rep0, uint64_t seed, int flags, uint8_t* S_out, double* X_out,
                       int64_t* counts_out, int64_t* exceptions_out);
int pgl_simulate_batch_dev(int device, int N, int64_t nT, int R, int nlin, double dt, const double* d_X0,
                           const double* d_AW, int n_rep, int rep0, uint64_t seed, int flags, uint8_t* d_S, double* d_X,
                           int64_t* d_counts, int64_t* d_exceptions, double* d_workspace, void* stream);
int pgl_simulate_batch_plan(int N, int R, int flags, int* ring_in_lds, long long* workspace_bytes_per_rep);

/* Clamped simulation: every neuron simulated with only its OWN spikes fed back, the other neurons held at their recorded
 * spikes -- the single-neuron prediction given the population activity (Pillow et al. 2008).  The rules are plain C in
 * csrc/pglm_condsim.h.
 *
 * Clamped currents.  Xc[t, q] = X0[t, q], then the recorded spikes of the other neurons in a fixed order: bins
 * s = max(0, t - R) .. t - 1 ascending, inside a bin the presynaptic neurons p != q ascending, AW[p, t - s - 1, q] added once per
 * spike of the recorded count (repeated addition, no multiply).  X0 (nT, N) and AW (N, R, N) [n_pre][tau][n_post] as for
 * pgl_simulate_batch.  The recorded spikes come as event lists sorted by (bin, pre): ev_pre (E) int32, ev_cnt (E) uint8 >= 1,
 * bin_off (nT + 1) int64 (bin s owns events bin_off[s] .. bin_off[s + 1] - 1; E = bin_off[nT], E = 0 allowed).
 *
 * One chain (replicate r, neuron n): pgl_simulate_streams' loop for a neuron that is alone, on the threshold stream
 * thr(seed, r, n, k) above.  Per bin: x = Xc[t, n] + AW[n, t - s - 1, n] for every own scattered spike at a bin s in
 * t - R .. t - 1, ascending s, once per spike; acc += nlin(x) * dt; rounds while acc > thr: S[t, n] += 1; a round that starts with
 * S[t, n] >= 10 is dropped and counted as an exception OF THAT NEURON (the cap is the neuron's own, as if it were alone: in
 * pgl_simulate_streams any neuron at 10 drops the round of all; the tenth spike is recorded and not scattered, as there);
 * otherwise the spike is scattered, acc -= thr (clamped at 0), a new threshold is drawn.  Whenever pgl_simulate_streams(N,
 * X = Xc, AW with only its [n, :, n] entries kept, rep = r, seed) reports 0 exceptions, its column n is this chain spike for
 * spike.
 *
 * Accumulators.  Windows of win bins from bin 0 (the last may be short), n_win = ceil(nT / win); acc (6, n_win, N) int64 over
 * the replicates: sum c, sum c^2, #(c < obs), #(c = obs), min c, max c, with c the replicate's count of the window and
 * obs (n_win, N) int64 the recorded one.  accumulate = 0 initialises acc, exceptions and fallbacks; accumulate != 0 continues
 * them: a call over rep0 .. rep0 + n_rep - 1 followed by a continuing call over the next range equals one call over both.
 * Integer atomics (the result does not depend on the order); no f64 atomics.
 *
 * cond_currents[_dev]: Xc (nT, N) out.  simulate_cond[_dev]: exceptions (N) int64 summed over the replicates; counts
 *     (n_rep, N) int64, S (n_rep, nT, N) uint8 (tests) and fallbacks (1) int64 may be NULL.  A chain keeps its own spike bins
 *     of the last R bins in a queue of 32 entries; a chain with more moves to a ring of R doubles in the workspace for the
 *     rest of its bins (fallbacks counts those chains) -- the result does not depend on the queue; flags bit 0 starts every
 *     chain on the ring.  d_workspace: pgl_simulate_cond_workspace(N, R, n_rep) = N R n_rep 8 bytes, required.  The _dev forms
 *     take device pointers and are asynchronous on `stream`.  N <= 1024; R <= 4096 (more: PGL_ERR_UNSUPPORTED); bad arguments:
 *     PGL_ERR_ARG.  The host-pointer form of the currents checks the event lists.
 *     N ceil(n_rep / 64) workgroups must not exceed 2^31 - 1 (PGL_ERR_ARG).
 * simulate_cond_streams: host reference of one replicate (no GPU needed), S (nT, N) uint8, exceptions_out (N), closest_call_out
 *     as pgl_simulate_streams (both may be NULL).  It serves the shapes the device entries serve and refuses the same ones
 *     (dt > 0, N <= 1024, R <= 4096). */
int pgl_simulate_cond_streams(int N, int64_t nT, int R, int nlin, double dt, const double* Xc, const double* AW, int rep,
                              uint64_t seed, uint8_t* S, int64_t* exceptions_out, double* closest_call_out);
int pgl_cond_currents_dev(int device, int N, int64_t nT, int R, const double* d_X0, const double* d_AW, const int32_t* d_ev_pre,
                          const uint8_t* d_ev_cnt, const int64_t* d_bin_off, double* d_Xc, void* stream);
int pgl_cond_currents(int device, int N, int64_t nT, int R, const double* X0, const double* AW, const int32_t* ev_pre,
                      const uint8_t* ev_cnt, const int64_t* bin_off, double* Xc_out);
long long pgl_simulate_cond_workspace(int N, int R, int n_rep);
int pgl_simulate_cond_dev(int device, int N, int64_t nT, int R, int nlin, double dt, const double* d_Xc, const double* d_AW,
                          const int64_t* d_obs, int64_t win, int n_rep, int rep0, uint64_t seed, int flags, int accumulate,
                          int64_t* d_acc, int64_t* d_exceptions, int64_t* d_counts, uint8_t* d_S, int64_t* d_fallbacks,
                          double* d_workspace, void* stream);
int pgl_simulate_cond(int device, int N, int64_t nT, int R, int nlin, double dt, const double* Xc, const double* AW,
                      const int64_t* obs, int64_t win, int n_rep, int rep0, uint64_t seed, int flags, int accumulate,
                      int64_t* acc, int64_t* exceptions, int64_t* counts_out, uint8_t* S_out, int64_t* fallbacks);

/* Stimulus decoding: the MAP stimulus given the spikes (the decoding half of Pillow et al., Nature 454 (2008) 995-999; the
 * reference has no counterpart: its graph has no derivative with respect to the stimulus).  The objective, its gradient and
 * its Hessian-vector products with respect to the stimulus, the parameters and the spikes fixed.  Rule and host mirror:
 * csrc/pglm_decode.h, kernels: csrc/pglm_decode.hip.h.
 * Served: a stimulus set by pgl_set_stimulus with the identity spatial basis in layout 1 (BasisStimulus: D dimensions, B
 * temporal basis functions over Rt taps, feature column d B + b), both nonlinearities, the whole recording.  No stimulus,
 * caller-supplied feature columns, layout 0 or a spatial basis ('spatiotemporal' dense), a separable stimulus and a time range
 * (pgl_set_time_range: a time shard) return PGL_ERR_UNSUPPORTED.
 * The unknown u (Tu, D) lives on the stimulus grid, dt_stim = q dt with an integer q >= 1:
 *     s = L u            s[t] = (1 - r / q) u[i] + (r / q) u[i + 1] for t = q i + r, s[t] = u[Tu - 1] for i >= Tu - 1
 *     K[tau, d, n]     = sum_b basis_t[tau, b] w_stim[n, d B + b],   tau = 0 .. Rt - 1
 *     I[t, n]          = sum_d sum_tau K[tau, d, n] s[t - 1 - tau, d]          (strictly causal, s = 0 before bin 0)
 *     x = c + I,  c[t, n] = bias_n + GX0[t, n]: the currents of the recorded spikes at theta with the stimulus weights zero
 *     F(u)             = sum_t sum_n [S log lam(x) - dt lam(x)] + log p(u)     (the all-f64 rate function of pgl_rescale_dev)
 *     r[t, n]          = S (log lam)'(x) - dt lam'(x)       exp: S - dt e^x;  explinear: (S / lam - dt) sig(x)
 *     cc[t, n]         = the c_t of pgl_hvp_* above, with its limits
 *     g_s[t', d]       = sum_n sum_tau K[tau, d, n] r[t' + 1 + tau, n]         (rows past nT are zero)
 *     grad F           = L^T g_s + grad log p(u)
 *     H v              = L^T K^T (cc o (K L v)) + hess log p . v
 * Prior (pgl_decode_prior), per stimulus dimension Gaussian with mean mu and the tridiagonal precision (1 / sigma^2) I +
 * (1 / rho^2) Dt^T Dt, Dt the first differences in time; rho = inf (or <= 0) gives the iid prior; the normalising constant is
 * dropped:   log p(u) = sum_d [ -1/2 sum_i (u_i - mu)^2 / sigma^2 - 1/2 sum_{i < Tu-1} (u_{i+1} - u_i)^2 / rho^2 ].
 *   pgl_decode_prepare_dev   d_theta (N, P), d_Weff (N, N): builds K (Rt D N doubles), runs the forward-only pass at theta with
 *       the stimulus block written as zeros and keeps c in a buffer of its own (nT N doubles; later forward passes overwrite
 *       GX).  New spikes / basis / stimulus invalidate it.  The handle's own copy of theta (its stimulus block now zeros) and
 *       GX (now the currents WITHOUT the stimulus) are overwritten: what pgl_gibbs_prepare_all left there before is gone.
 *   pgl_decode_eval_dev      d_u (Tu, D) -> d_F[3] = {F, log likelihood, log prior} and d_grad_u (Tu, D) or NULL.  r and cc stay
 *       on the device (2 nT N doubles).  Launches: k_dec_interp, k_dec_forward<nlin, 0>, k_dec_sum and, with a gradient,
 *       k_dec_backward, k_dec_interp_t.  The ll terms are added per (256-bin chunk, neuron), then the chunks in order, then the
 *       neurons in order; nothing is atomic: two calls give the same bits.
 *   pgl_decode_hvp_dev       d_v, d_hv (Tu, D): H v at the point, Tu, q and prior of the last eval (none since the last prepare:
 *       PGL_ERR_STATE).  Launches: k_dec_interp, k_dec_forward<nlin, 1>, k_dec_backward, k_dec_interp_t.
 *   pgl_decode_prepare / pgl_decode_eval / pgl_decode_hvp   the same with host arrays.  They move Tu D doubles each way, so
 *       they take the columns D of the caller's arrays (and pgl_decode_hvp the rows Tu): D other than the stimulus dimensions
 *       of the handle, or Tu other than the last evaluation's, is PGL_ERR_ARG and nothing is copied.
 *   pgl_decode_host          the whole rule on the host, no GPU and no handle: c, S (nT, N) (spike counts as doubles),
 *       basis_t (Rt, B), theta (N, P) with P >= 1 + D B, u (Tu, D) -> F[3], grad_u (or NULL) and, where v is given, hv.
 * The _dev forms are asynchronous on the handle's stream.  Tu < 1, q < 1, sigma <= 0 or a NULL pointer: PGL_ERR_ARG; eval before
 * prepare: PGL_ERR_STATE. */
typedef struct {
    double mu, sigma, rho;
} pgl_decode_prior;
int pgl_decode_prepare_dev(pgl_handle h, const double* d_theta, const double* d_Weff);
int pgl_decode_eval_dev(pgl_handle h, const double* d_u, int64_t Tu, int q, const pgl_decode_prior* prior, double* d_F,
                        double* d_grad_u);
int pgl_decode_hvp_dev(pgl_handle h, const double* d_v, double* d_hv);
int pgl_decode_prepare(pgl_handle h, const double* theta, const double* Weff);
int pgl_decode_eval(pgl_handle h, const double* u, int64_t Tu, int D, int q, const pgl_decode_prior* prior, double* F_out,
                    double* grad_u_out);
int pgl_decode_hvp(pgl_handle h, const double* v, int64_t Tu, int D, double* hv_out);
int pgl_decode_host(int N, int64_t nT, int nlin, double dt, const double* c, const double* S, const double* basis_t, int Rt, int B,
                    int D, const double* theta, int P, const double* u, int64_t Tu, int q, const pgl_decode_prior* prior,
                    const double* v, double* F_out, double* grad_u_out, double* hv_out);

/* Timing of the most recent pgl_ll_grad[_dev] call, measured with HIP events on the
 * handle's stream: ms of the fused kernel alone and of the whole call (prep +
 * fused + finalize).  For the _dev form call after pgl_sync. */
int pgl_last_timing(pgl_handle h, double* fused_ms, double* total_ms);

/* Mean of the same two figures over the pgl_ll_grad[_dev] calls since the last reset (at most the
 * 256 most recent ones; each call records its own HIP event set, so a caller can queue many
 * evaluations without a host synchronisation in between).  Synchronises the stream; reset != 0
 * starts a new window. */
int pgl_timing_summary(pgl_handle h, int reset, int* n_launches, double* mean_fused_ms,
                       double* mean_total_ms);

/* Order all subsequent work of the handle on a caller-owned HIP stream (hipStream_t passed as
 * void*; NULL = back to the handle's own stream).  A caller that runs collectives on its own
 * stream (RCCL through torch.distributed) passes that stream here: evaluation and all-reduce are
 * then ordered by the stream, with no host synchronisation between steps.  The reference has no
 * counterpart (Theano's shared variables are synchronous). */
int pgl_set_stream(pgl_handle h, void* stream);

/* Dev / test: dry run of the kernel dispatch, no device needed -- the names (as in the code object) of the fused kernel
 * instantiations an evaluation of `count` neurons from n_lo of a population of this shape would launch, one per line in
 * launch order (the evaluation's own launch sequence, enqueued on a context without a device; a kernel launched in the
 * forward and again in the backward phase of the 3-phase path is listed twice).
 * stim: 0 none / dense stimulus columns, 1 separable by the tap-rate kernels, 2 separable at the frame rate (stimulus
 * current inside the fused forward where that form exists), 3 at the frame rate through the slab.  path: 0 ll+grad,
 * 1 ll only, 2 the forward launches of pgl_gibbs_prepare_all, 3 the launches of pgl_hvp_prepare_dev /
 * pgl_hvp_prepare_list_dev over these neurons (k_hvp5<.., 1> or the forward-only K-split launches), 4 the launches of
 * pgl_hvp_apply_dev after such a prepare (k_hvp5<.., 0> + pass 2 of k_fused5, or the forward-only and backward-only K-split
 * launches of every column slice), 5 the k_hess launches of pgl_hess_dev after such a prepare (one per batch of rows),
 * 6 the launches of pgl_rescale_dev (those of path 2, then k_rescale_chunk<nlin>, k_rescale_scan, k_rescale_finish; the dry
 * run's context has nlin = PGL_NLIN_EXP), 7 the launches of pgl_pointwise_dev (those of path 2, then k_pw_chunk<nlin>,
 * k_pw_block), 8 the launches of pgl_rate_windows_dev at win = 50 (those of path 2, then k_rw_piece<nlin>, k_rw_window),
 * 9 the launches of pgl_rescale_corr_dev (those of path 2, then k_rcorr_chunk<nlin>, k_rescale_scan, k_rcorr_finish),
 * 11 the launches of pgl_decode_prepare_dev and of a pgl_decode_eval_dev with a gradient behind it (k_dec_filters, those of
 * path 2, k_dec_offset; k_dec_interp, k_dec_forward<nlin, 0>, k_dec_sum, k_dec_backward, k_dec_interp_t; the dry run reads
 * Dstim as one stimulus dimension of Dstim basis functions over R taps; Dstim = 0 or stim >= 1: PGL_ERR_UNSUPPORTED, as the
 * call), 12 the launches of pgl_decode_hvp_dev behind such an eval (k_dec_interp, k_dec_forward<nlin, 1>, k_dec_backward,
 * k_dec_interp_t).
 * Paths 3 / 4 / 5 with stim >= 1 return PGL_ERR_UNSUPPORTED, as the calls themselves.
 * The reference has no counterpart (Theano picks its own C implementations); tests hold every reachable instantiation to
 * zero bytes of scratch. */
int pgl_plan_kernels(int N, int B, int R, int Dstim, long long nT, int stim, int n_lo, int count, int path, int opt_kernel,
                     int opt_f32, char* out, int cap);

/* The fused kernel instantiations the handle's last pgl_ll_grad / pgl_ll_grad_dev / pgl_ll_grad_list_dev /
 * pgl_gibbs_prepare_all / pgl_hvp_prepare_* / pgl_hvp_apply_dev / pgl_hess_dev / pgl_rescale_dev / pgl_pointwise_dev call launched, one per line in `out`, in launch order and in the format of pgl_plan_kernels
 * (which enqueues the same launch sequence on a device-less context).  Needs PGL_OPT_RECORD_KERNELS = 1 on the handle
 * (PGL_ERR_STATE otherwise).  Dev / test entry point: tests compare it with the dry run. */
int pgl_last_kernels(pgl_handle h, char* out, int cap);

/* The launch geometry the host chose for the handle's last pgl_gibbs_ll_cols call made with PGL_OPT_RECORD_KERNELS = 1
 * (PGL_ERR_STATE without one): out[0..9] = {path (0 regime-split, 1 all-f64), CP, nsplit, column groups, nloop, time blocks,
 * spike blocks, same_pre, gtb, rows} (the fields a path does not have: nsplit = nloop = 1, the others 0); n >= 10.
 * Dev / test entry point: tests/test_gpu_gibbs_sweep.py holds it to the Python statement of the arithmetic. */
int pgl_gibbs_last_geometry(pgl_handle h, int* out, int n);

/* Launch geometry and algorithmic work of the fused kernel for [n_lo,n_hi):
 * info[0]=blocks, [1]=threads/block, [2]=time chunks, [3]=k-tiles(16 rows),
 * [4]=LDS bytes, [5]=rows per time tile, [6]=algorithmic flops (4*nT*Ktot*npost),
 * [7]=algorithmic bytes, [8]=number of spike events (nonzero bins), [9]=kernel the call would use
 * (1 4-wave, 2 K-split, 3 K-split with f32 features, 4 two-pass, 5 two-pass on resident feature
 * tiles, 6 K-split on resident feature tiles -- incl. the block-ring form k_fused8 for one post tile of a 25..40 k-tile
 * row --, 7 single pass without K split on resident tiles), [10]=bytes of resident feature tiles (0 unless [9] >= 5),
 * [11]=HBM bytes the hot kernels
 * stream per evaluation on top of the algorithmic ones (feature tiles, residual slab), [12]=stimulus path of the
 * call: 0 none / dense feature columns, 1 separable by the tap-rate kernels, 2 separable at the frame rate.
 * (For a separable stimulus [6] counts the impulse contraction only and [7] the projected stimulus at its frame
 * rate.) */
int pgl_info(pgl_handle h, int n_lo, int n_hi, double* info, int n_info);

#ifdef __cplusplus
}
#endif
#endif
