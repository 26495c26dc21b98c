// C ABI (include/pyglm_hip.h) over the gfx950 kernels in pglm_kernels.hip.h.
// Host side: context, device buffers, spike-event (CSR) index, launch plans, timing.
#include "pglm_kernels.hip.h"
#include "../../include/pyglm_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
// Names of the fused kernel instantiations an evaluation launches, as the code object's demangled symbol reads (dry_record,
// pglm_launch.h):
//  g_dry -- dry run of the dispatch (pgl_plan_kernels): the evaluation is enqueued on a context without a device,
//           launch_kernel records what it would launch and launches nothing, every other device operation is skipped;
//  g_rec -- PGL_OPT_RECORD_KERNELS: a real evaluation records what it launches (pgl_last_kernels).
static thread_local std::vector<std::string>* g_dry = nullptr;
static thread_local std::vector<std::string>* g_rec = nullptr;
#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(PGL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct pgl_context {
    int N = 0, B = 0, R = 0, nlin = 0, device = 0;
    int64_t nT = 0;
    double dt = 0;
    int Dstim = 0, Kimp = 0, Ktot = 0, nT16 = 0;
    int numCU = 256;
    hipStream_t stream = nullptr;        // stream every call of this handle is ordered on
    hipStream_t own_stream = nullptr;    // the handle's own stream (stream == own_stream unless pgl_set_stream)
    hipStream_t aux_stream = nullptr;    // side stream: reduction of the first G half beside pass 2
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    static constexpr int NEV = 256;      // ring of per-launch event sets {start, fused begin, fused end, end}
    hipEvent_t evr[NEV][4] = {};
    hipEvent_t* ev = evr[0];             // event set of the most recent pgl_ll_grad call
    long long ev_launches = 0;           // launches recorded since the last timing reset
    bool have_spikes = false, have_basis = false;
    int64_t nnz = 0;
    DevBuf S, ST, spk, wlo, whi, phi, fstim;
    std::vector<int> h_ptr;              // host copy of the event-list row pointers (N+1)
    std::vector<int2> h_ev;              // host copy of the event lists (window tables are rebuilt
                                         // when the basis support changes)
    int Rk = 0;                          // taps the kernels use: R minus trailing all-zero basis rows
    DevBuf theta, Weff, ll, grad, Wfrag, bias, Gpart, llpart, gbpart, Xbuf;
    // resident feature tiles (k_build_fimg): a few image sets side by side -- a masked MAP line search
    // alternates between post-block widths whose kernels want different column paddings (e.g. k_fused6 with
    // 10 or 12 k-tiles at C2), and rebuilding 0.4 GB of images per call would cost more than the call
    struct ImgSlot {
        DevBuf buf;
        int key = 0, tile0 = 0, ntiles = 0;   // key = ktl << 8 | kth (kth = 0: one-part images); 0 = empty / stale
        unsigned long long stamp = 0;
    };
    static constexpr int NIMG = 8;          // (a wide population keeps one image set per column slice)
    ImgSlot imgs[NIMG];
    int img_cur = 0;
    unsigned long long img_clock = 0;
    double* pin_out = nullptr;           // pinned host buffer for small results (PGL_KMAX doubles)
    DevBuf IimpT, Inet, Istim, tmpA, tmpB, tmpC, wsmall, part, outK, lam, wcol, thetan;
    // separable (rank-1) stimulus: theta rows are [bias, w_t(Bt), w_x(Bx), w_imp]; Dstim = Bt + Bx
    bool sep = false;
    int sepBt = 0, sepBx = 0, sepRt = 0;
    int64_t sepT = 0;
    double sep_dt_stim = 0;
    DevBuf zf, zfT, sbt, Yf, Qb, Qf, spart;
    // frame-rate form of the separable stimulus (dt_stim an integer multiple q of dt, J = ceil(Rt / q) + 2 <= 8 frame
    // values per bin): coefficient table C[q (M + 1)][sepJ][sepBTp], see k_sepf_fwd
    bool sepf = false;
    int sepq = 0, sepM = 0, sepJ = 0, sepBTp = 0;
    int sepNH = 0, sepGs = 0;            // A-fragment table of the fused forward (k_fused7<.., 2>): head tiles, log2 gcd(q, 16)
    bool sepA_ok = false;
    DevBuf sepC, sepA, sepAT, sepD, YfT, Hb, wpart, QvT;
    int opt_sepf = 0;                    // dev option 94: 2 = never take the frame-rate path, 3 = stimulus current through the slab (k_sepf_fwd)
    const int* cur_pidx = nullptr;       // post-neuron list of the evaluation being enqueued (device)
    int gibbs_npost = -1;
    double gibbs_bias = 0;
    // batched column Gibbs (pgl_gibbs_prepare_all / _ll_cols / _update_cols)
    DevBuf GX, gtheta, gargs, gpart, gout, ghs, gfs;
    DevBuf staA;                         // pgl_sta with A_out == NULL: the averages (sta_n, sta_L, sta_D) stay here for
    int sta_n = 0, sta_L = 0, sta_D = 0; // pgl_leading_singular_pairs(A == NULL)
    int gx_xs = 0;                       // row stride of GX (16 * post tiles); 0 = not prepared
    int64_t gx_t_lo = 0, gx_t_hi = 0;    // time range GX was prepared for
    unsigned char* pin_args = nullptr;   // pinned staging of the per-call column arguments / results
    size_t pin_args_cap = 0;
    int opt_f32 = 0, opt_nchunks = 0, opt_dbg = 0, opt_kernel = 0, opt_ptw = 0, opt_gibbs = 0, opt_finw = 0, opt_sb6 = 0, opt_epi64 = 0, opt_timing = 1, opt_slice_cols = 0, opt_hlp = 0, opt_pbmajor = 0, opt_tri_rows = 0;
    int opt_img32 = 0;                   // PGL_OPT_FEATURE_F32 = 2: f32 resident blocks for the narrow-shard kernel (k_fused8<.., 1>)
    int gibbs_geo[10] = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // launch geometry of the last recorded pgl_gibbs_ll_cols (pgl_gibbs_last_geometry)
    int opt_record = 0;                  // PGL_OPT_RECORD_KERNELS: last_kernels holds the fused launches of the last evaluation
    std::vector<std::string> last_kernels;
    long long call_no = 0;               // evaluations enqueued since the last pgl_set_option(PGL_OPT_TIMING)
    int64_t t_lo = 0, t_hi = 0;          // evaluated time range [t_lo, t_hi) (pgl_set_time_range)
    bool timing_valid = false;
    // lock-step optimiser: the pinned flag buffer of pgl_bfgs_step_dev and its device address (looked up once);
    // history size (hk_bound * P doubles per row) up to which a whole iteration is ONE row kernel (PGL_OPT_BFGS_MERGE)
    double* flags_host[4] = {nullptr, nullptr, nullptr, nullptr};
    double* flags_dev[4] = {nullptr, nullptr, nullptr, nullptr};
    int flags_next = 0;
    int opt_bfgs_merge = 65536;
    // Hessian-vector products (pgl_hvp_prepare_* / pgl_hvp_apply_dev): the curvature c[t, n] of the prepared rows stays in
    // Cbuf -- in the accumulator layout of the two-pass kernels' slab (hvp_fused) or as rows (nT, 16 * post tiles) -- with
    // the handle's own copies of Weff and of the neuron list; hvp_ok falls with new spikes / basis / stimulus
    bool hvp_ok = false, hvp_fused = false, hvp_list = false;
    int hvp_n_lo = 0, hvp_count = 0;
    int64_t hvp_t_lo = 0, hvp_t_hi = 0;
    DevBuf Cbuf, hvp_idx, hvp_Weff, hvp_ll;
    DevBuf hess_part;                    // pgl_hess_dev: chunk partials of k_hess
    // time rescaling (pgl_rescale_dev): in-chunk sums at the events, chunk totals and their prefix
    DevBuf rs_pre, rs_tot, rs_cum;
    // the corrected intervals (pgl_rescale_corr_dev): the rate of every event's bin; pgl_ks_uniform_dev: the sorted values where
    // the caller wants none (pgl_ks_uniform and pgl_rescale_acf: their sorted values / scores)
    DevBuf rs_qev, rs_tail, ks_work;
    DevBuf pw_part;                      // pointwise ll (pgl_pointwise_dev): chunk sums
    DevBuf rw_part, rw_cnt;              // rate windows (pgl_rate_windows_dev): piece sums of rate and spike counts
    // stimulus decoding (pgl_decode_*): dec_stim -- the stimulus came through pgl_set_stimulus with the identity spatial basis
    // in layout 1, its temporal basis (dec_Rt, dec_B) is kept in dec_basis and D = dec_D; dec_ok -- K and the offset c of the
    // last prepare stand (new spikes / basis / stimulus: they fall); dec_point -- r and cc of an eval since then, with its Tu,
    // q and prior
    bool dec_stim = false, dec_ok = false, dec_point = false;
    int dec_Rt = 0, dec_B = 0, dec_D = 0, dec_q = 0, opt_dec_cut = 0;
    int64_t dec_Tu = 0;
    PglDecPrior dec_prior = {0.0, 1.0, 0.0};
    DevBuf dec_basis, dec_K, dec_c, dec_r, dec_cc, dec_y, dec_s, dec_gs, dec_part, dec_col;
    // the host-array forms (pgl_hvp .. pgl_chain_diag): the device copies of their arrays, taken by index (stage_up).  Every
    // such call ends in stage_end, so a slot holds nothing across calls and the forms share them
    static constexpr int NSTAGE = 6;     // (pgl_wald_groups moves six arrays)
    DevBuf stage[NSTAGE];
    std::vector<double> hvp_host;        // pgl_hvp: theta and Weff of its last prepare (a CG solve repeats them: no new prepare)
};

static int ensure(DevBuf& b, size_t bytes)
{
    if (g_dry) return PGL_OK;
    if (bytes <= b.cap && b.p) return PGL_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    if (bytes == 0) bytes = 16;
    HIPCHK(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return PGL_OK;
}
static void release(DevBuf& b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}
static int find_img(const pgl_context* h, int key, int tile0, int ntiles)
{
    for (int i = 0; i < pgl_context::NIMG; ++i)
        if (h->imgs[i].key == key && h->imgs[i].tile0 == tile0 && h->imgs[i].ntiles == ntiles && h->imgs[i].buf.p)
            return i;
    return -1;
}
static void invalidate_images(pgl_context* h)
{
    h->hvp_ok = false;                            // (new spikes / basis / stimulus: the prepared curvature is stale too)
    h->dec_ok = h->dec_point = false;             // (and the decoder's filters and offset)
    for (int i = 0; i < pgl_context::NIMG; ++i) h->imgs[i].key = 0;
}
// can a new image set of `want` bytes be placed (in a free slot, or over the least recently used one)?
static bool img_room(const pgl_context* h, size_t want)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return true;
    size_t reclaim = 0;
    int lru = 0;
    for (int i = 1; i < pgl_context::NIMG; ++i)
        if (h->imgs[i].stamp < h->imgs[lru].stamp) lru = i;
    for (int i = 0; i < pgl_context::NIMG; ++i)
        if (h->imgs[i].key == 0) reclaim = std::max(reclaim, h->imgs[i].buf.cap);
    reclaim = std::max(reclaim, h->imgs[lru].buf.cap);
    return want <= reclaim || want - reclaim <= free_b / 10 * 9;
}
// an error code of a step is the call's own
#define PASS(call)                               \
    do {                                         \
        int rc_ = (call);                        \
        if (rc_ != PGL_OK) return rc_;           \
    } while (0)
#define ENSURE(buf, bytes) PASS(ensure(buf, bytes))

// ---- what the host-array forms share: each is check, stage_up, its _dev form, stage_down, stage_end ----
// room for `bytes` (one element at the least) in staging slot `slot`, and the host array `src` on its way there; src ==
// nullptr: room alone, for a result.  No synchronise behind the copy: the caller's arrays live until the stage_end of the same
// call.  Like ensure, the three do nothing in a dry run.
static int stage_up(pgl_handle h, int slot, const void* src, size_t bytes)
{
    ENSURE(h->stage[slot], std::max<size_t>(bytes, 8));
    if (src && bytes && !g_dry) HIPCHK(hipMemcpyAsync(h->stage[slot].p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return PGL_OK;
}
// a result on its way back; dst == nullptr: the caller wants none
static int stage_down(pgl_handle h, void* dst, const void* d_src, size_t bytes)
{
    if (dst && bytes && !g_dry) HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    return PGL_OK;
}
static int stage_end(pgl_handle h)
{
    if (!g_dry) HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}
// host theta of the rows [n_lo, n_hi) -> d_theta (h->theta: an evaluation's, h->gtheta: a draw's) and Weff (N, N) -> h->Weff,
// on stage_up's terms
static int upload_rows(pgl_handle h, DevBuf& d_theta, int n_lo, int n_hi, const double* theta, const double* Weff)
{
    const size_t tb = (size_t)(n_hi - n_lo) * (1 + (size_t)h->Dstim + h->Kimp) * 8, wb = (size_t)h->N * h->N * 8;
    ENSURE(d_theta, tb);
    ENSURE(h->Weff, wb);
    HIPCHK(hipMemcpyAsync(d_theta.p, theta, tb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->Weff.p, Weff, wb, hipMemcpyHostToDevice, h->stream));
    return PGL_OK;
}

// the planner (Plan, Slice, the k-tile lists, make_plan, select_plans, hvp_select) and the launch layer (dry_record,
// launch_kernel, dispatch, the launchers of the fused kernels): both need the context above
#include "pglm_plan.h"
#include "pglm_launch.h"

// workgroups of k_gibbs_rate_cols a CU holds at `lds` bytes of dynamic LDS (occupancy query, cached per size)
static int gibbs_rate_wg_per_cu(size_t lds)
{
    static std::map<size_t, int> cache;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    int& c = cache[lds];
    if (c == 0) {
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_gibbs_rate_cols, 256, lds) != hipSuccess || occ < 1)
            occ = 3;
        c = occ;
    }
    return c;
}

// separable stimulus at the frame rate: which = 0 forward, 1 backward, 2 finish
template <int J, int BT>
static void launch_sepf(int which, const SepfParams& sp, hipStream_t s);
// (the thin GEMMs of the separable stimulus: k_gemm_kc when the k-contiguous operands are 16-byte aligned, else k_gemm_mfma)
static inline bool gemm_aligned(const void* p, long long ld) { return ((uintptr_t)p % 16) == 0 && (ld % 2) == 0; }

template <int J, int BT>
static void launch_sepf(int which, const SepfParams& sp, hipStream_t s)
{
    const long long nF = sp.F1 - sp.F0 + 1;
    const int nG = (sp.nPT + 3) / 4;
    dim3 grid((unsigned)((nF + 3) / 4), (unsigned)nG);
    if (which == 0) hipLaunchKernelGGL((k_sepf_fwd<J, BT>), grid, dim3(256), 0, s, sp);
    else if (which == 1) hipLaunchKernelGGL((k_sepf_bwd<J, BT>), grid, dim3(256), 0, s, sp);
    else {
        const int nA = (int)((sp.Tstim + 15) / 16) * nG;
        hipLaunchKernelGGL((k_sepf_finish<J, BT>), dim3(nA + nG * BT), dim3(1024), 0, s, sp, nA, nG);
    }
}

// ---- the thin GEMMs (pglm_stim.hip.h): one launcher per kernel template, the only places that state a grid shape.  The
// callers below and pgl_gemm_dev (the test entry) all launch through them.
static int launch_gemm_nt(pgl_handle h, const double* A, int lda, const double* B, int ldb, double* C, int ldc,
                          int M, int N, int K)
{
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64));
    hipLaunchKernelGGL(k_gemm_nt, grid, dim3(256), 0, h->stream, A, lda, B, ldb, C, ldc, M, N, K);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// k_gemm_mfma<NT>: any strides, a batch along blockIdx.z
template <int NT>
static int launch_gemm_mfma_nt(pgl_handle h, const double* A, long long sam, long long sak, long long sAb, const double* B,
                               long long sbn, long long sbk, long long sBb, double* C, long long scm, long long scn,
                               long long sCb, int M, int N, int K, int batch)
{
    hipLaunchKernelGGL(k_gemm_mfma<NT>, dim3((M + 15) / 16, (N + 16 * NT - 1) / (16 * NT), batch), dim3(512), 0, h->stream, A,
                       sam, sak, B, sbn, sbk, C, scm, scn, M, N, K, sAb, sBb, sCb);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// k_gemm_kc<NT, BK, NB>: A k-contiguous, 16-byte aligned with lda even, K even; B likewise (BK = 1) or n-contiguous (BK = 0)
template <int NT, int BK, int NB>
static int launch_gemm_kc(pgl_handle h, const double* A, long long lda, const double* B, long long ldb, double* C,
                          long long scm, long long scn, int M, int N, int K)
{
    hipLaunchKernelGGL((k_gemm_kc<NT, BK, NB>), dim3((unsigned)((M + 15) / 16), (unsigned)((N + 16 * NT - 1) / (16 * NT))),
                       dim3(512), 0, h->stream, A, lda, B, ldb, C, scm, scn, M, N, K);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// one workgroup per replicate (k_simulate, pglm_simulate.hip.h)
template <int NLIN, bool RING_LDS>
static int sim_launch(const SimParams& sp, int n_rep, int threads, size_t lds, hipStream_t s)
{
    if (lds > 65536)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_simulate<NLIN, RING_LDS>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_simulate<NLIN, RING_LDS>), dim3(n_rep), dim3(threads), lds, s, sp);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// one workgroup per (group, row) (k_filter_bands, pglm_filters.hip.h); above 64 KiB of LDS the instantiation opts in once
template <int B>
static hipError_t filt_launch_b(const FiltParams& p, size_t lds, hipStream_t stream)
{
    if (lds + 512 > 65536) {                                   // (the static LDS of the kernel is 392 bytes)
        const hipError_t e = ensure_dyn_lds(k_filter_bands<B>, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_filter_bands<B>, dim3((unsigned)p.G, (unsigned)p.M), dim3(PGL_FILT_THREADS), lds, stream, p);
    return hipGetLastError();
}

// B in 1 .. PGL_FILT_MAX_B and n C in 2 .. PGL_FILT_MAX_DRAWS (filt_check); fills Spad and resident
static hipError_t filt_launch(int B, FiltParams p, hipStream_t stream)
{
    const long long S = (long long)p.n * p.C;
    p.Spad = filt_pad(S);
    p.resident = filt_resident(S, B);
    const size_t lds = filt_lds_bytes(S, B);
    switch (B) {
#define PGL_FILT_CASE(b) case b: return filt_launch_b<b>(p, lds, stream);
        PGL_FILT_CASE(1) PGL_FILT_CASE(2) PGL_FILT_CASE(3) PGL_FILT_CASE(4) PGL_FILT_CASE(5) PGL_FILT_CASE(6) PGL_FILT_CASE(7)
        PGL_FILT_CASE(8) PGL_FILT_CASE(9) PGL_FILT_CASE(10) PGL_FILT_CASE(11) PGL_FILT_CASE(12) PGL_FILT_CASE(13)
        PGL_FILT_CASE(14) PGL_FILT_CASE(15) PGL_FILT_CASE(16)
#undef PGL_FILT_CASE
    }
    return hipErrorInvalidValue;
}

// one workgroup of 256 threads per row on the handle's stream: the launch shape of every row kernel of the lock-step methods
template <typename... Params, typename... Args>
static int launch_rows(pgl_handle h, void (*kernel)(Params...), int rows, Args&&... args)
{
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(256), 0, h->stream, static_cast<Params>(args)...);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

extern "C" {

const char* pgl_last_error(void) { return g_err.c_str(); }
int pgl_version(void) { return PGL_ABI_VERSION; }

int pgl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pgl_create(int N, int64_t nT, int B, int R, int nlin, double dt, int device, pgl_handle* out)
{
    if (!out) return fail(PGL_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (N <= 0 || nT <= 0 || B <= 0 || R <= 0) return fail(PGL_ERR_ARG, "N, nT, B, R must be positive");
    if (B > PGL_MAXB) return fail(PGL_ERR_UNSUPPORTED, "B > 8 basis functions");
    if (nlin != PGL_NLIN_EXP && nlin != PGL_NLIN_EXPLINEAR) return fail(PGL_ERR_ARG, "unknown nonlinearity");
    if (nT > (int64_t)1 << 30) return fail(PGL_ERR_UNSUPPORTED, "nT > 2^30 bins");
    if (!(dt > 0)) return fail(PGL_ERR_ARG, "dt must be positive");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(PGL_ERR_HIP, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(PGL_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    pgl_context* h = new pgl_context();
    h->N = N; h->nT = nT; h->B = B; h->R = R; h->Rk = R; h->nlin = nlin; h->dt = dt; h->device = device;
    h->Kimp = N * B; h->Ktot = h->Kimp; h->nT16 = (int)((nT + 15) / 16);
    h->t_lo = 0; h->t_hi = nT;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->numCU = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(PGL_ERR_HIP, hipGetErrorString(e)); }
    h->stream = h->own_stream;
    {
        // the side stream reduces the first G half beside pass 2 of the two-pass kernel: highest priority, so that its
        // blocks take every wave slot pass 2 leaves free and the reduction is over before pass 2 is (at default
        // priority it finished ~15 us after a 1/8-recording pass 2 and delayed the second reduction)
        int prio_lo = 0, prio_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_hi = 0;
        e = hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, prio_hi);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) { pgl_destroy(h); return fail(PGL_ERR_HIP, hipGetErrorString(e)); }
    for (int s = 0; s < pgl_context::NEV; ++s)
        for (int i = 0; i < 4; ++i) {
            e = hipEventCreate(&h->evr[s][i]);
            if (e != hipSuccess) { pgl_destroy(h); return fail(PGL_ERR_HIP, hipGetErrorString(e)); }
        }
    *out = h;
    return PGL_OK;
}

int pgl_destroy(pgl_handle h)
{
    if (!h) return PGL_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    DevBuf* bufs[] = {&h->S, &h->ST, &h->spk, &h->wlo, &h->whi, &h->phi, &h->fstim, &h->theta,
                      &h->Weff, &h->ll, &h->grad, &h->Wfrag, &h->bias, &h->Gpart, &h->llpart,
                      &h->gbpart, &h->Xbuf, &h->imgs[0].buf, &h->imgs[1].buf, &h->imgs[2].buf, &h->imgs[3].buf, &h->imgs[4].buf, &h->imgs[5].buf, &h->imgs[6].buf, &h->imgs[7].buf, &h->IimpT, &h->Inet, &h->Istim, &h->tmpA, &h->tmpB, &h->tmpC,
                      &h->wsmall, &h->part, &h->outK, &h->lam, &h->wcol, &h->thetan, &h->GX, &h->gtheta,
                      &h->gargs, &h->gpart, &h->gout, &h->ghs, &h->gfs, &h->zf, &h->zfT, &h->sbt, &h->Yf, &h->Qb, &h->Qf,
                      &h->spart, &h->sepC, &h->sepA, &h->sepAT, &h->sepD, &h->YfT, &h->Hb, &h->wpart, &h->QvT, &h->staA,
                      &h->Cbuf, &h->hvp_idx, &h->hvp_Weff, &h->hvp_ll, &h->hess_part, &h->rs_pre, &h->rs_tot, &h->rs_cum,
                      &h->rs_qev, &h->rs_tail, &h->ks_work, &h->pw_part, &h->rw_part, &h->rw_cnt, &h->dec_basis, &h->dec_K,
                      &h->dec_c, &h->dec_r, &h->dec_cc, &h->dec_y, &h->dec_s, &h->dec_gs, &h->dec_part, &h->dec_col};
    for (DevBuf* b : bufs) release(*b);
    for (DevBuf& b : h->stage) release(b);
    for (int s = 0; s < pgl_context::NEV; ++s)
        for (int i = 0; i < 4; ++i)
            if (h->evr[s][i]) (void)hipEventDestroy(h->evr[s][i]);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    if (h->pin_args) (void)hipHostFree(h->pin_args);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)hipStreamDestroy(h->aux_stream); }
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return PGL_OK;
}

int pgl_set_time_range(pgl_handle h, int64_t t_lo, int64_t t_hi)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (t_lo < 0 || t_hi > h->nT || t_lo >= t_hi) return fail(PGL_ERR_ARG, "bad time range");
    if (t_lo % 16 != 0) return fail(PGL_ERR_ARG, "t_lo must be a multiple of 16 bins");
    h->t_lo = t_lo;
    h->t_hi = t_hi;
    return PGL_OK;
}

int pgl_set_option(pgl_handle h, int option, int value)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    switch (option) {
    case PGL_OPT_FEATURE_F32: h->opt_f32 = (value == 1) ? 1 : 0; h->opt_img32 = (value == 2) ? 1 : 0; return PGL_OK;
    case 99: h->opt_dbg = value; return PGL_OK;
    case 98: h->opt_ptw = value; return PGL_OK;
    case 97: if (value < 0 || value > 16) return fail(PGL_ERR_ARG, "finalize waves: 0 (auto) .. 16"); h->opt_finw = value; return PGL_OK;
    case PGL_OPT_DECODE_CUT: if (value < 0 || value > 64) return fail(PGL_ERR_ARG, "decode cut: 0 .. 64"); h->opt_dec_cut = value; return PGL_OK;
    case 90: h->opt_tri_rows = value; return PGL_OK;        // dev: 1 = the triangular products of the dense-mass HMC on one workgroup per row (A/B)
    case 91: h->opt_pbmajor = value; return PGL_OK;          // dev: 1 = chunk-major grid for wide populations (A/B)
    case 92: h->opt_hlp = value; return PGL_OK;              // dev: 1 = no helper waves in the two-pass kernel (A/B)
    case 93: h->opt_slice_cols = value; return PGL_OK;      // dev: feature columns per slice of the 3-phase path (0 = 640)
    case 94: h->opt_sepf = value; return PGL_OK;            // dev: 2 = separable stimulus always by the tap-rate kernels, 3 = stimulus current through the slab, 4 = residual slab + k_sepf_bwd (no fused backward)
    case 95: h->opt_sb6 = value; return PGL_OK;              // dev: 2 = never the one-buffer / block-ring forms
    case PGL_OPT_RECORD_KERNELS: h->opt_record = value ? 1 : 0; h->last_kernels.clear(); return PGL_OK;
    case PGL_OPT_KERNEL: h->opt_kernel = value; return PGL_OK;
    case PGL_OPT_GIBBS_KERNEL: h->opt_gibbs = value; return PGL_OK;
    case PGL_OPT_EPI_F64: h->opt_epi64 = value ? 1 : 0; return PGL_OK;
    case PGL_OPT_TIMING: if (value < 0) return fail(PGL_ERR_ARG, "timing interval < 0"); h->opt_timing = value; h->call_no = 0; return PGL_OK;
    case PGL_OPT_BFGS_MERGE: if (value < 0) return fail(PGL_ERR_ARG, "merge threshold < 0"); h->opt_bfgs_merge = value; return PGL_OK;
    case PGL_OPT_NCHUNKS: if (value < 0) return fail(PGL_ERR_ARG, "nchunks < 0"); h->opt_nchunks = value; return PGL_OK;
    }
    return fail(PGL_ERR_ARG, "unknown option");
}

// per 16-row tile event windows of every neuron: lo = first event with s >= 16*tile - Rk,
// hi = first event with s >= 16*tile + 15 (events are sorted by time within a neuron)
static int upload_windows(pgl_handle h)
{
    const int N = h->N, nT16 = h->nT16;
    const std::vector<int>& ptr = h->h_ptr;
    const std::vector<int2>& ev = h->h_ev;
    std::vector<int> wlo((size_t)nT16 * N), whi((size_t)nT16 * N);
    for (int n = 0; n < N; ++n) {
        int lo = ptr[n], hi = ptr[n];
        const int end = ptr[n + 1];
        for (int tile = 0; tile < nT16; ++tile) {
            const int64_t klo = (int64_t)16 * tile - h->Rk;
            const int64_t khi = (int64_t)16 * tile + 15;
            while (lo < end && ev[(size_t)lo].x < klo) ++lo;
            while (hi < end && ev[(size_t)hi].x < khi) ++hi;
            wlo[(size_t)tile * N + n] = lo;
            whi[(size_t)tile * N + n] = hi;
        }
    }
    ENSURE(h->wlo, wlo.size() * 4);
    ENSURE(h->whi, whi.size() * 4);
    HIPCHK(hipMemcpyAsync(h->wlo.p, wlo.data(), wlo.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->whi.p, whi.data(), whi.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));          // the host vectors die with this frame
    return PGL_OK;
}

// Build the spike-event index from the dense count matrix and upload everything.
static int upload_spikes(pgl_handle h, const uint8_t* S)
{
    HIPCHK(hipSetDevice(h->device));
    const int N = h->N;
    const int64_t nT = h->nT;
    // two passes over the nT x N counts (77 MB at C3), each on up to 16 host threads over slabs of time: per-slab event
    // counts of every neuron, a prefix over (neuron, slab) = every slab's write position in a neuron's list, then the
    // slabs fill their own pieces -- the lists stay time-sorted (single-threaded: 0.15 s of a 0.19 s upload at C3)
    const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, std::max(1u, std::thread::hardware_concurrency())),
                                                               nT / 65536));
    std::vector<int64_t> t0s(nth + 1);
    for (int i = 0; i <= nth; ++i) t0s[i] = nT * i / nth;
    std::vector<std::vector<int>> slab((size_t)nth, std::vector<int>((size_t)N, 0));
    auto run = [&](auto&& fn) {
        std::vector<std::thread> th;
        for (int i = 1; i < nth; ++i) th.emplace_back(fn, i);
        fn(0);
        for (auto& t : th) t.join();
    };
    run([&](const int i) {
        int* c = slab[(size_t)i].data();
        for (int64_t t = t0s[i]; t < t0s[i + 1]; ++t) {
            const uint8_t* row = S + t * N;
            for (int n = 0; n < N; ++n) c[n] += row[n] != 0;
        }
    });
    std::vector<int> cnt(N + 1, 0);
    for (int n = 0; n < N; ++n) {
        int tot = cnt[n];
        for (int i = 0; i < nth; ++i) {                    // slab[i][n] becomes the slab's first position in neuron n's list
            const int c = slab[(size_t)i][(size_t)n];
            slab[(size_t)i][(size_t)n] = tot;
            tot += c;
        }
        cnt[n + 1] = tot;
    }
    const int64_t nnz = cnt[N];
    std::vector<int2> ev((size_t)std::max<int64_t>(nnz, 1));
    run([&](const int i) {
        int* cur = slab[(size_t)i].data();
        for (int64_t t = t0s[i]; t < t0s[i + 1]; ++t) {
            const uint8_t* row = S + t * N;
            for (int n = 0; n < N; ++n)
                if (row[n]) ev[(size_t)cur[n]++] = make_int2((int)t, (int)row[n]);
        }
    });
    h->h_ptr = cnt;
    h->h_ev.swap(ev);
    const std::vector<int2>& evr = h->h_ev;
    // S is padded with zero rows up to the 16-row tile grid: the fused kernels read the counts of whole
    // tiles through incremented pointers, without clamping the row index
    const size_t s_rows = (size_t)h->nT16 * 16;
    ENSURE(h->S, s_rows * N);
    ENSURE(h->ST, (size_t)nT * N);
    ENSURE(h->spk, evr.size() * sizeof(int2));
    HIPCHK(hipMemsetAsync((uint8_t*)h->S.p + (size_t)nT * N, 0, (s_rows - (size_t)nT) * N, h->stream));
    HIPCHK(hipMemcpyAsync(h->S.p, S, (size_t)nT * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->spk.p, evr.data(), evr.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    {
        const int rc = upload_windows(h);
        if (rc) return rc;
    }
    dim3 grid((unsigned)((nT + 63) / 64), (unsigned)((N + 63) / 64));
    hipLaunchKernelGGL(k_transpose_u8, grid, dim3(256), 0, h->stream, (const uint8_t*)h->S.p,
                       (uint8_t*)h->ST.p, (long long)nT, N);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->nnz = nnz;
    h->have_spikes = true;
    h->gibbs_npost = -1;
    invalidate_images(h);
    h->gx_xs = 0;
    return PGL_OK;
}

int pgl_set_spikes_u8(pgl_handle h, const uint8_t* S)
{
    if (!h || !S) return fail(PGL_ERR_ARG, "null argument");
    return upload_spikes(h, S);
}

int pgl_set_spikes_f64(pgl_handle h, const double* S)
{
    if (!h || !S) return fail(PGL_ERR_ARG, "null argument");
    const size_t n = (size_t)h->nT * h->N;
    std::vector<uint8_t> u(n);
    for (size_t i = 0; i < n; ++i) {
        const double v = S[i];
        if (!(v >= 0.0 && v <= 255.0) || v != std::floor(v))
            return fail(PGL_ERR_ARG, "spike counts must be integers in 0..255");
        u[i] = (uint8_t)v;
    }
    return upload_spikes(h, u.data());
}

int pgl_set_basis(pgl_handle h, const double* ibasis)
{
    if (!h || !ibasis) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    // Trailing taps that are zero in every basis column contribute nothing (the raised-cosine
    // bases of the reference end before dt_max: basis.py:56-106 leaves the last ~10 % of the
    // 100-point grid at zero): the kernels run with Rk <= R taps and correspondingly shorter
    // event windows -- same sums, fewer events per tile.
    int Rk = 1;
    for (int d = 0; d < h->R; ++d)
        for (int b = 0; b < h->B; ++b)
            if (ibasis[(size_t)d * h->B + b] != 0.0) Rk = d + 1;
    std::vector<double> ph((size_t)h->B * Rk);
    for (int d = 0; d < Rk; ++d)
        for (int b = 0; b < h->B; ++b) ph[(size_t)b * Rk + d] = ibasis[(size_t)d * h->B + b];
    ENSURE(h->phi, ph.size() * 8);
    HIPCHK(hipMemcpyAsync(h->phi.p, ph.data(), ph.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (Rk != h->Rk) {
        h->Rk = Rk;
        if (h->have_spikes) {
            const int rc = upload_windows(h);
            if (rc) return rc;
        }
    }
    h->have_basis = true;
    h->gibbs_npost = -1;
    invalidate_images(h);
    h->gx_xs = 0;
    return PGL_OK;
}

int pgl_set_stim_features(pgl_handle h, const double* fstim, int Dstim)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (Dstim < 0 || (Dstim > 0 && !fstim)) return fail(PGL_ERR_ARG, "bad stimulus features");
    HIPCHK(hipSetDevice(h->device));
    h->Dstim = Dstim;
    h->Ktot = h->Kimp + Dstim;
    h->sep = false;
    h->dec_stim = false;
    h->gibbs_npost = -1;
    invalidate_images(h);
    h->gx_xs = 0;
    if (Dstim > 0) {
        const size_t bytes = (size_t)h->nT * Dstim * 8;
        ENSURE(h->fstim, bytes);
        HIPCHK(hipMemcpyAsync(h->fstim.p, fstim, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return PGL_OK;
}

int pgl_set_stimulus(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim,
                     const double* basis_x, int Bx, const double* basis_t, int Rt, int Bt, int layout)
{
    if (!h || !stim || !basis_t) return fail(PGL_ERR_ARG, "null argument");
    if (Tstim <= 0 || D <= 0 || Bx <= 0 || Rt <= 0 || Bt <= 0 || !(dt_stim > 0) || (layout != 0 && layout != 1))
        return fail(PGL_ERR_ARG, "bad stimulus description");
    if (!basis_x && Bx != D) return fail(PGL_ERR_ARG, "identity spatial basis needs Bx == D");
    const int Dstim = Bx * Bt;
    if ((size_t)(Rt + 256 + Rt * Bt) * 8 > 64 * 1024) return fail(PGL_ERR_UNSUPPORTED, "temporal basis too long");
    HIPCHK(hipSetDevice(h->device));
    DevBuf dstim, dbx, dbt, dzx;
    auto cleanup = [&]() { release(dstim); release(dbx); release(dbt); release(dzx); };
    int rc = ensure(dstim, (size_t)Tstim * D * 8);
    if (!rc) rc = ensure(dbt, (size_t)Rt * Bt * 8);
    if (!rc) rc = ensure(dzx, (size_t)h->nT * Bx * 8);
    if (!rc && basis_x) rc = ensure(dbx, (size_t)D * Bx * 8);
    if (!rc) rc = ensure(h->fstim, (size_t)h->nT * Dstim * 8);
    if (rc) { cleanup(); return rc; }
    hipError_t e = hipMemcpyAsync(dstim.p, stim, (size_t)Tstim * D * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dbt.p, basis_t, (size_t)Rt * Bt * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && basis_x)
        e = hipMemcpyAsync(dbx.p, basis_x, (size_t)D * Bx * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        const long long total = (long long)h->nT * Bx;
        const int blocks = (int)std::min<long long>((total + 255) / 256, 65535);
        hipLaunchKernelGGL(k_stim_project, dim3(blocks), dim3(256), 0, h->stream, (const double*)dstim.p,
                           (long long)Tstim, D, dt_stim, h->dt, basis_x ? (const double*)dbx.p : nullptr,
                           Bx, (double*)dzx.p, (long long)h->nT);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        dim3 grid((unsigned)((h->nT + 255) / 256), (unsigned)Bx);
        hipLaunchKernelGGL(k_stim_conv, grid, dim3(256), (size_t)(Rt + 256 + Rt * Bt) * 8, h->stream,
                           (const double*)dzx.p, (const double*)dbt.p, Rt, Bt, Bx, layout,
                           (double*)h->fstim.p, (long long)h->nT);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    cleanup();
    if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("pgl_set_stimulus: ") + hipGetErrorString(e));
    // what pgl_decode_* needs of a 'basis' stimulus: its temporal basis
    h->dec_stim = !basis_x && layout == 1;
    if (h->dec_stim) {
        ENSURE(h->dec_basis, (size_t)Rt * Bt * 8);
        HIPCHK(hipMemcpyAsync(h->dec_basis.p, basis_t, (size_t)Rt * Bt * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->dec_Rt = Rt; h->dec_B = Bt; h->dec_D = D;
    }
    h->Dstim = Dstim;
    h->Ktot = h->Kimp + Dstim;
    h->sep = false;
    h->gibbs_npost = -1;
    invalidate_images(h);
    h->gx_xs = 0;
    return PGL_OK;
}

// Frame-rate coefficient table of the separable stimulus (k_sepf_fwd): for bin t = q F + o, base = max(F - M, 0),
//   C[t][j][bt] = sum_{tau = 1 .. min(Rt, t)} basis_t[tau-1][bt] * (weight of frame base + j in np.interp at bin t - tau)
// for t < q (M + 1); later bins repeat the rows q M + o.  np.interp between frames f = s / q and f + 1 at bin s
// weighs them (1 - a, a) with a = (s % q) / q (bkgd.py:303-340 interpolates on the dt grid; the clamp behind the
// last frame is an index clamp in the kernels).  Only when dt_stim is an integer multiple of dt and J <= 8, Bt <= 4.
static int build_frame_table(pgl_handle h, const double* basis_t, int Rt, int Bt, double dt_stim)
{
    h->sepf = false;
    const double ratio = dt_stim / h->dt;
    const long long q = llround(ratio);
    if (q < 1 || std::fabs(ratio - (double)q) > 1e-9 * ratio) return PGL_OK;
    const long long M = (Rt + q - 1) / q, J = M + 2;
    if (J > 8 || Bt > 4) return PGL_OK;
    const int Jp = (J <= 5 && Bt <= 3) ? 5 : 8, BTp = (J <= 5 && Bt <= 3) ? 3 : 4;
    const long long rows = q * (M + 1);
    if (rows * Jp * BTp > (1ll << 24)) return PGL_OK;
    std::vector<double> C((size_t)rows * Jp * BTp, 0.0);
    for (long long t = 0; t < rows; ++t) {
        const long long F = t / q, base = std::max<long long>(F - M, 0);
        double* row = C.data() + (size_t)t * Jp * BTp;
        for (long long tau = 1; tau <= std::min<long long>(Rt, t); ++tau) {
            const long long sb = t - tau, f = sb / q;
            const double a = (double)(sb % q) / (double)q;
            for (int bt = 0; bt < Bt; ++bt) {
                const double b = basis_t[(size_t)(tau - 1) * Bt + bt];
                row[(f - base) * BTp + bt] += b * (1.0 - a);
                if (a != 0.0) row[(f + 1 - base) * BTp + bt] += b * a;
            }
        }
    }
    ENSURE(h->sepC, C.size() * 8);
    HIPCHK(hipMemcpyAsync(h->sepC.p, C.data(), C.size() * 8, hipMemcpyHostToDevice, h->stream));
    // A fragments of the fused forward (k_fused7<.., XIO = 2>): for a 16-bin tile that starts at bin t0 (frame F0, base =
    // max(F0 - M, 0)) the coefficient of bin t0 + i on column (j', bt) of [w_t (x) z][base + j'] is
    // C[row(t0 + i)][j' - (base(F_i) - base)][bt]; it depends on t0 only through t0 mod q once F0 >= M (phases of
    // gcd(q, 16) bins), the tiles before that get their own entries.  MFMA A layout: lane l holds row l & 15, column
    // 4 s + (l >> 4) of k-step s.  (J + 1) Bt <= 18 columns = five k-steps; q >= 16 so that a tile spans two frames at most.
    h->sepA_ok = false;
    if (Jp == 5 && BTp == 3 && q >= 16 && (J + 1) * Bt <= 18) {
        int gs = 0;
        while (gs < 4 && (q % (2 << gs)) == 0) ++gs;                   // gcd(q, 16) = 1 << gs
        const long long g = 1ll << gs, NH = (q * M + 15) / 16, NP = q / g;
        std::vector<double> A((size_t)(NH + NP) * 5 * 64, 0.0);
        for (long long e = 0; e < NH + NP; ++e) {
            // a representative first bin: the tile itself in the head, else the first tile behind the head with this phase
            long long t0 = 16 * e;
            if (e >= NH) {
                const long long o0 = (e - NH) * g;
                t0 = -1;
                for (long long c = NH; c < NH + 2 * q; ++c)
                    if ((16 * c) % q == o0) { t0 = 16 * c; break; }
                if (t0 < 0) continue;                                   // (phase never occurs)
            }
            const long long F0 = t0 / q, base0 = std::max<long long>(F0 - M, 0);
            for (int i = 0; i < 16; ++i) {
                const long long t = t0 + i, F = t / q, o = t - F * q, dlt = std::max<long long>(F - M, 0) - base0;
                const double* crow = C.data() + (size_t)((std::min(F, M)) * q + o) * Jp * BTp;
                for (long long j = 0; j < J; ++j)
                    for (int bt = 0; bt < Bt; ++bt) {
                        const long long k = (j + dlt) * 3 + bt;          // column (j', bt), j' = j + dlt <= J
                        A[((size_t)e * 5 + k / 4) * 64 + (k % 4) * 16 + i] = crow[j * BTp + bt];
                    }
            }
        }
        // ... and the A^T fragments of the fused backward (k_fused7<.., 3>): D[(j', bt)][n] += sum_i A[i][(j', bt)] r[i][n] as
        // eight MFMAs (two accumulator tiles of 16 columns x four k-steps of four bins); lane l of fragment 4 mt + ks holds
        // column 16 mt + (l & 15) of bin 4 ks + (l >> 4)
        std::vector<double> AT((size_t)(NH + NP) * 8 * 64, 0.0);
        for (long long e = 0; e < NH + NP; ++e)
            for (int k = 0; k < 18; ++k)
                for (int i = 0; i < 16; ++i) {
                    const double v = A[((size_t)e * 5 + k / 4) * 64 + (k % 4) * 16 + i];
                    AT[((size_t)e * 8 + (k / 16) * 4 + i / 4) * 64 + (i % 4) * 16 + (k % 16)] = v;
                }
        ENSURE(h->sepA, A.size() * 8);
        HIPCHK(hipMemcpyAsync(h->sepA.p, A.data(), A.size() * 8, hipMemcpyHostToDevice, h->stream));
        ENSURE(h->sepAT, AT.size() * 8);
        HIPCHK(hipMemcpyAsync(h->sepAT.p, AT.data(), AT.size() * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->sepNH = (int)NH; h->sepGs = gs;
        h->sepA_ok = true;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sepq = (int)q; h->sepM = (int)M; h->sepJ = Jp; h->sepBTp = BTp;
    h->sepf = true;
    return PGL_OK;
}

int pgl_set_stimulus_separable(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim,
                               const double* basis_x, int Bx, const double* basis_t, int Rt, int Bt)
{
    if (!h || !stim || !basis_t) return fail(PGL_ERR_ARG, "null argument");
    if (Tstim <= 0 || D <= 0 || Bx <= 0 || Rt <= 0 || Bt <= 0 || !(dt_stim > 0))
        return fail(PGL_ERR_ARG, "bad stimulus description");
    if (!basis_x && Bx != D) return fail(PGL_ERR_ARG, "identity spatial basis needs Bx == D");
    if ((size_t)(2 * Rt + 2 * PGL_SEP_TB) * 8 > 64 * 1024) return fail(PGL_ERR_UNSUPPORTED, "temporal basis too long");
    HIPCHK(hipSetDevice(h->device));
    ENSURE(h->zf, (size_t)Tstim * Bx * 8);
    ENSURE(h->zfT, (size_t)Tstim * Bx * 8);
    ENSURE(h->sbt, (size_t)Rt * Bt * 8);
    HIPCHK(hipMemcpyAsync(h->sbt.p, basis_t, (size_t)Rt * Bt * 8, hipMemcpyHostToDevice, h->stream));
    // z = stim . basis_x at the stimulus frame rate (Tstim, Bx) and its transpose, both by the NT GEMM
    std::vector<double> bxT((size_t)Bx * D, 0.0);
    for (int d = 0; d < D; ++d)
        for (int b = 0; b < Bx; ++b) bxT[(size_t)b * D + d] = basis_x ? basis_x[(size_t)d * Bx + b] : (d == b ? 1.0 : 0.0);
    DevBuf dstim, dbxT;
    int rc = ensure(dstim, (size_t)Tstim * D * 8);
    if (!rc) rc = ensure(dbxT, (size_t)Bx * D * 8);
    if (rc) { release(dstim); release(dbxT); return rc; }
    hipError_t e = hipMemcpyAsync(dstim.p, stim, (size_t)Tstim * D * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dbxT.p, bxT.data(), (size_t)Bx * D * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        rc = launch_gemm_nt(h, (const double*)dstim.p, D, (const double*)dbxT.p, D, (double*)h->zf.p, Bx,
                            (int)Tstim, Bx, D);
        if (!rc) rc = launch_gemm_nt(h, (const double*)dbxT.p, D, (const double*)dstim.p, D, (double*)h->zfT.p,
                                     (int)Tstim, Bx, (int)Tstim, D);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    release(dstim);
    release(dbxT);
    if (rc) return rc;
    if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("pgl_set_stimulus_separable: ") + hipGetErrorString(e));
    h->sep = true;
    h->dec_stim = false;
    h->sepBt = Bt; h->sepBx = Bx; h->sepRt = Rt; h->sepT = Tstim; h->sep_dt_stim = dt_stim;
    {
        int rc2 = build_frame_table(h, basis_t, Rt, Bt, dt_stim);
        if (rc2) return rc2;
    }
    h->Dstim = Bt + Bx;                       // layout of a theta row; NOT feature columns of the fused kernels
    h->Ktot = h->Kimp;
    h->gibbs_npost = -1;
    invalidate_images(h);
    h->gx_xs = 0;
    return PGL_OK;
}

// separable stimulus, forward: X[t][j] += I_stim[t, n_lo + j] for the rows of d_theta (npost rows of P)
static int sep_forward(pgl_handle h, const double* d_theta, int npost, double* X, int xs, int64_t t_lo, int64_t t_hi,
                       SepParams& sp)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    const int P = 1 + h->Dstim + h->Kimp;
    ENSURE(h->Yf, (size_t)npost * h->sepT * 8);
    int rc = launch_gemm_nt(h, d_theta + 1 + h->sepBt, P, (const double*)h->zf.p, h->sepBx, (double*)h->Yf.p,
                            (int)h->sepT, npost, (int)h->sepT, h->sepBx);
    if (rc) return rc;
    sp.Yf = (const double*)h->Yf.p; sp.basis_t = (const double*)h->sbt.p; sp.theta = d_theta;
    sp.P = P; sp.Bt = h->sepBt; sp.Rt = h->sepRt; sp.npost = npost; sp.xs = xs;
    sp.Tstim = h->sepT; sp.nT = h->nT; sp.t_lo = t_lo; sp.t_hi = t_hi; sp.dt = h->dt; sp.dt_stim = h->sep_dt_stim;
    sp.X = X;
    const int nblk = (int)((t_hi - t_lo + PGL_SEP_TB - 1) / PGL_SEP_TB);
    hipLaunchKernelGGL(k_sep_conv_fwd, dim3(nblk, npost), dim3(256), (size_t)(2 * h->sepRt + PGL_SEP_TB) * 8,
                       h->stream, sp);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// separable stimulus, backward: X holds r = d ll / d x on [t_lo, t_hi) (zero behind t_hi); writes the w_t and
// w_x columns of d_grad
static int sep_backward(pgl_handle h, const SepParams& sp, double* d_grad)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    const int npost = sp.npost, Rt = h->sepRt;
    const int nblk = (int)((sp.t_hi - sp.t_lo + PGL_SEP_TB - 1) / PGL_SEP_TB);
    ENSURE(h->spart, (size_t)nblk * npost * Rt * 8);
    hipLaunchKernelGGL(k_sep_corr, dim3(nblk, npost), dim3(256), (size_t)(Rt + 2 * PGL_SEP_TB) * 8, h->stream, sp,
                       (double*)h->spart.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sep_wt_grad, dim3(npost), dim3(64), 0, h->stream, sp, (const double*)h->spart.p, nblk,
                       d_grad);
    HIPCHK(hipGetLastError());
    const long long s_lo = std::max<long long>(0, sp.t_lo - Rt), nS = sp.t_hi - s_lo;
    ENSURE(h->Qb, (size_t)npost * nS * 8);
    ENSURE(h->Qf, (size_t)npost * h->sepT * 8);
    const int nblk_s = (int)((nS + PGL_SEP_TB - 1) / PGL_SEP_TB);
    hipLaunchKernelGGL(k_sep_conv_bwd, dim3(nblk_s, npost), dim3(256), (size_t)(2 * Rt + PGL_SEP_TB) * 8, h->stream,
                       sp, (double*)h->Qb.p, s_lo, nS);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sep_interp_T, dim3((unsigned)((h->sepT + 255) / 256), npost), dim3(256), 0, h->stream, sp,
                       (const double*)h->Qb.p, s_lo, nS, (double*)h->Qf.p);
    HIPCHK(hipGetLastError());
    return launch_gemm_nt(h, (const double*)h->Qf.p, (int)h->sepT, (const double*)h->zfT.p, (int)h->sepT,
                          d_grad + 1 + h->sepBt, sp.P, npost, h->sepBx, (int)h->sepT);
}

static int launch_gemm_mfma(pgl_handle h, const double* A, long long sam, long long sak, const double* B,
                            long long sbn, long long sbk, double* C, long long scm, long long scn, int M, int N, int K)
{
    // operands whose m / n index is the contiguous one load whole 128-byte lines per 16-lane group; a k-contiguous
    // operand costs a line per lane (pick A for it: one tile per wave against NT of B)
    const int mb = (M + 15) / 16;
    if ((long long)mb * ((N + 63) / 64) >= 128)         // 16 x 64 per wave; else 16 x 16 (more workgroups)
        return launch_gemm_mfma_nt<4>(h, A, sam, sak, 0, B, sbn, sbk, 0, C, scm, scn, 0, M, N, K, 1);
    return launch_gemm_mfma_nt<1>(h, A, sam, sak, 0, B, sbn, sbk, 0, C, scm, scn, 0, M, N, K, 1);
}

static int launch_sepf_any(pgl_handle h, int which, const SepfParams& sp)
{
    if (h->sepJ == 5 && h->sepBTp == 3) launch_sepf<5, 3>(which, sp, h->stream);
    else launch_sepf<8, 4>(which, sp, h->stream);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// separable stimulus at the frame rate, forward: the slab Xbuf[tile - tile0][post tile][r][lane] = I_stim of the
// npost rows of d_theta on the plan's tile range
static int sepf_forward(pgl_handle h, const Plan& pl, const double* d_theta, SepfParams& sp, bool fused_fwd)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    const int P = 1 + h->Dstim + h->Kimp, ldy = pl.nPT * 16;
    ENSURE(h->YfT, (size_t)h->sepT * ldy * 8);
    // z_n[f] = (stim . basis_x)[f, :] . w_x[n]  ->  YfT[f][n]
    int rc = PGL_OK;
    const double* wx = d_theta + 1 + h->sepBt;
    if (gemm_aligned(h->zf.p, h->sepBx) && gemm_aligned(wx, P)) {      // m = f, n = n, k = x (even): both operands k-contiguous
        rc = launch_gemm_kc<4, 1, 8>(h, (const double*)h->zf.p, (long long)h->sepBx, wx, (long long)P, (double*)h->YfT.p,
                                     (long long)ldy, 1LL, (int)h->sepT, pl.npost, h->sepBx);
    } else {                                                           // m = n, n = f, k = x
        rc = launch_gemm_mfma(h, wx, P, 1, (const double*)h->zfT.p, 1, h->sepT, (double*)h->YfT.p, 1, ldy, pl.npost,
                              (int)h->sepT, h->sepBx);
    }
    if (rc) return rc;
    sp.Ctab = (const double*)h->sepC.p; sp.YfT = (const double*)h->YfT.p; sp.theta = d_theta;
    sp.X = (double*)h->Xbuf.p; sp.Hb = nullptr; sp.wpart = nullptr; sp.QvT = nullptr; sp.grad = nullptr;
    sp.D = nullptr; sp.B0 = sp.B1 = 0; sp.SL = 0; sp.tilesPerChunk = 0;
    sp.P = P; sp.Bt = h->sepBt; sp.M = h->sepM; sp.q = h->sepq; sp.npost = pl.npost; sp.nPT = pl.nPT; sp.ldy = ldy;
    sp.tile0 = pl.tile0; sp.nTiles = pl.nTiles; sp.Tstim = h->sepT;
    const long long tb = (long long)pl.tile0 * 16, te = tb + (long long)pl.nTiles * 16;
    sp.F0 = tb / h->sepq; sp.F1 = (te - 1) / h->sepq;
    if (fused_fwd) return PGL_OK;               // the stimulus current is five k-steps of the fused kernel (k_fused7<.., 2>)
    return launch_sepf_any(h, 0, sp);
}

// backward: the slab holds r = d ll / d x (fused_bwd: the fused kernel left the per-base pieces sp.D instead); writes the
// w_x columns of d_grad and the w_t columns -- fused_bwd: their block partials sp.wpart, nwt of them, which the trailing
// blocks of k_finalize sum
static int sepf_backward(pgl_handle h, SepfParams& sp, double* d_grad, bool fused_bwd = false, int* nwt = nullptr)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    const long long nF = sp.F1 - sp.F0 + 1;
    ENSURE(h->QvT, (size_t)h->sepT * sp.ldy * 8);
    int rc = PGL_OK;
    if (fused_bwd) {
        const int nblk = (int)((h->sepT + 15) / 16);
        ENSURE(h->wpart, (size_t)nblk * 3 * sp.ldy * 8);
        sp.wpart = (double*)h->wpart.p; sp.QvT = (double*)h->QvT.p; sp.grad = d_grad;
        hipLaunchKernelGGL(k_sepf_finish_d, dim3((unsigned)nblk), dim3(1024), 0, h->stream, sp);
        HIPCHK(hipGetLastError());
        if (nwt) *nwt = nblk;
    } else {
        ENSURE(h->Hb, (size_t)nF * h->sepJ * sp.ldy * 8);
        ENSURE(h->wpart, (size_t)nF * h->sepBTp * sp.ldy * 8);
        sp.Hb = (double*)h->Hb.p; sp.wpart = (double*)h->wpart.p; sp.QvT = (double*)h->QvT.p; sp.grad = d_grad;
        rc = launch_sepf_any(h, 1, sp);
        if (!rc) rc = launch_sepf_any(h, 2, sp);
    }
    if (rc) return rc;
    // d ll / d w_x[n][x] = sum_f (stim . basis_x)[f][x] QvT[f][n]
    if (gemm_aligned(h->zfT.p, h->sepT)) {                             // m = x (rows of zfT: f contiguous), n = n, k = f
        return launch_gemm_kc<1, 0, 16>(h, (const double*)h->zfT.p, (long long)h->sepT, (const double*)h->QvT.p,
                                        (long long)sp.ldy, d_grad + 1 + h->sepBt, 1LL, (long long)sp.P, h->sepBx, sp.npost,
                                        (int)h->sepT);
    }
    return launch_gemm_mfma(h, (const double*)h->zf.p, 1, h->sepBx, (const double*)h->QvT.p, 1, sp.ldy,
                            d_grad + 1 + h->sepBt, 1, sp.P, h->sepBx, sp.npost, (int)h->sepT);
}

int pgl_sta(pgl_handle h, const double* stim, int64_t Tstim, int D, double dt_stim, int L,
            const int* neurons, int n_sel, double* A_out)
{
    if (!h || !stim) return fail(PGL_ERR_ARG, "null argument");
    if (!h->have_spikes) return fail(PGL_ERR_STATE, "pgl_set_spikes_* has not been called");
    if (Tstim <= 0 || D <= 0 || L <= 0 || !(dt_stim > 0)) return fail(PGL_ERR_ARG, "bad stimulus description");
    const int nSel = neurons ? n_sel : h->N;
    if (nSel <= 0 || nSel > 65535) return fail(PGL_ERR_ARG, "bad neuron selection");
    std::vector<int> eoff((size_t)2 * nSel);
    for (int i = 0; i < nSel; ++i) {
        const int n = neurons ? neurons[i] : i;
        if (n < 0 || n >= h->N) return fail(PGL_ERR_ARG, "neuron index out of range");
        eoff[2 * i] = h->h_ptr[n];
        eoff[2 * i + 1] = h->h_ptr[n + 1];
    }
    const long long LD = (long long)L * D;
    const long long xb = (LD + 255) / 256;
    if (xb > 0x7fffffffLL) return fail(PGL_ERR_UNSUPPORTED, "L*D too large");
    // enough blocks to fill the chip when the output is small: split each neuron's events
    int echunks = (int)std::min<long long>(64, std::max<long long>(1, 4096 / (xb * nSel)));
    HIPCHK(hipSetDevice(h->device));
    DevBuf dstim, distim, deoff, dpart, dA;
    auto cleanup = [&]() { release(dstim); release(distim); release(deoff); release(dpart); release(dA); };
    // A_out == NULL: the averages stay on the device for pgl_leading_singular_pairs (157 MB for 64 neurons x 300 lags x 1024
    // pixels would otherwise cross PCIe twice)
    auto keep = [&]() {
        release(h->staA);
        h->staA = dA;
        dA = DevBuf();
        h->sta_n = nSel; h->sta_L = L; h->sta_D = D;
    };
    // frame-rate form (k_sta_weights + one thin GEMM): dt_stim an integer multiple of dt, an even number of frames (the
    // GEMM's 16-byte loads), a weight matrix of at most 2 GB; dev option 94 = 7: the bin-rate form
    const double ratio = dt_stim / h->dt;
    const long long q = llround(ratio);
    const bool frame_rate = q >= 1 && std::fabs(ratio - (double)q) <= 1e-9 * ratio && (Tstim % 2) == 0 && Tstim >= 2 &&
                            (long long)nSel * L * Tstim <= (1ll << 28) && h->opt_sepf != 7;
    int rc = ensure(dstim, (size_t)Tstim * D * 8);
    if (!rc && !frame_rate) rc = ensure(distim, (size_t)h->nT * D * 8);
    if (!rc) rc = ensure(deoff, eoff.size() * sizeof(int));
    if (!rc && !frame_rate) rc = ensure(dpart, (size_t)echunks * nSel * LD * 8);
    if (!rc) rc = ensure(dA, (size_t)nSel * LD * 8);
    if (rc) { cleanup(); return rc; }
    hipError_t e = hipMemcpyAsync(dstim.p, stim, (size_t)Tstim * D * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(deoff.p, eoff.data(), eoff.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
    if (frame_rate && e == hipSuccess) {
        DevBuf dW, dscale;
        std::vector<double> scale((size_t)nSel);
        for (int i = 0; i < nSel; ++i) {
            double cnt = 0.0;
            for (int j = eoff[2 * i]; j < eoff[2 * i + 1]; ++j) cnt += (double)h->h_ev[j].y;
            scale[i] = (h->dt / dt_stim) / cnt;                   // 0 spikes: inf -> NaN rows, like the reference's 0 / 0
        }
        rc = ensure(dW, (size_t)nSel * L * Tstim * 8);
        if (!rc) rc = ensure(dscale, (size_t)nSel * 8);
        if (rc) { release(dW); release(dscale); cleanup(); return rc; }
        e = hipMemcpyAsync(dscale.p, scale.data(), (size_t)nSel * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_sta_weights, dim3((unsigned)((Tstim + 255) / 256), (unsigned)L, (unsigned)nSel), dim3(256), 0,
                               h->stream, (const int2*)h->spk.p, (const int*)deoff.p, (const double*)dscale.p, L,
                               (long long)Tstim, (int)q, (double*)dW.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {                                    // A (nSel L, D) = Wt (nSel L, Tstim) . stim (Tstim, D)
            const int Mrows = nSel * L;
            if (launch_gemm_kc<1, 0, 16>(h, (const double*)dW.p, (long long)Tstim, (const double*)dstim.p, (long long)D,
                                         (double*)dA.p, (long long)D, 1LL, Mrows, D, (int)Tstim))
                e = hipErrorLaunchFailure;
        }
        if (e == hipSuccess && A_out)
            e = hipMemcpyAsync(A_out, dA.p, (size_t)nSel * LD * 8, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        release(dW); release(dscale);
        if (e == hipSuccess && !A_out) keep();
        cleanup();
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("pgl_sta: ") + hipGetErrorString(e));
        return PGL_OK;
    }
    if (e == hipSuccess) {
        const long long total = (long long)h->nT * D;
        const int blocks = (int)std::min<long long>((total + 255) / 256, 65535);
        hipLaunchKernelGGL(k_stim_project, dim3(blocks), dim3(256), 0, h->stream, (const double*)dstim.p,
                           (long long)Tstim, D, dt_stim, h->dt, (const double*)nullptr, D,
                           (double*)distim.p, (long long)h->nT);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sta, dim3((unsigned)xb, (unsigned)nSel, (unsigned)echunks), dim3(256), 0,
                           h->stream, (const int2*)h->spk.p, (const int*)deoff.p, (const double*)distim.p,
                           D, L, (double*)dpart.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sta_finish, dim3((unsigned)xb, (unsigned)nSel), dim3(256), 0, h->stream,
                           (const double*)dpart.p, (const int2*)h->spk.p, (const int*)deoff.p, LD, echunks,
                           h->dt / dt_stim, (double*)dA.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess && A_out)
        e = hipMemcpyAsync(A_out, dA.p, (size_t)nSel * LD * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && !A_out) keep();
    cleanup();
    if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("pgl_sta: ") + hipGetErrorString(e));
    return PGL_OK;
}

int pgl_get_stim_features(pgl_handle h, double* fstim_out)
{
    if (h && h->sep) return fail(PGL_ERR_STATE, "a separable stimulus has no dense feature matrix");
    if (!h || !fstim_out) return fail(PGL_ERR_ARG, "null argument");
    if (h->Dstim <= 0) return fail(PGL_ERR_STATE, "no stimulus features on the device");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(fstim_out, h->fstim.p, (size_t)h->nT * h->Dstim * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

static int check_ready(pgl_handle h)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!h->have_spikes) return fail(PGL_ERR_STATE, "pgl_set_spikes_* has not been called");
    if (!h->have_basis) return fail(PGL_ERR_STATE, "pgl_set_basis has not been called");
    return PGL_OK;
}

static void fill_params(pgl_handle h, const Plan& pl, const Slice& sl, int n_lo, bool want_grad,
                        int mode, FusedParams& fp)
{
    fp.nT = h->nT; fp.N = sl.Ns; fp.B = h->B; fp.R = h->Rk; fp.nlin = h->nlin;
    fp.Dstim = sl.Ds; fp.Kimp = sl.Ns * h->B; fp.Ktot = fp.Kimp + sl.Ds; fp.dt = h->dt;
    fp.Nall = h->N; fp.np0 = sl.np0; fp.DsAll = h->Dstim; fp.ds0 = sl.ds0;
    fp.mode = mode; fp.Xbuf = (double*)h->Xbuf.p; fp.xstride = pl.nPT * 16;
    fp.sepA = nullptr; fp.sepZ = nullptr; fp.sepTheta = nullptr; fp.sepT = 0;
    fp.sepLdy = fp.sepQ = fp.sepM = fp.sepNH = fp.sepG = fp.sepBt = 0;
    fp.sepAT = nullptr; fp.sepD = nullptr; fp.sepB0 = 0; fp.sepSL = 0;
    fp.spk = (const int2*)h->spk.p; fp.wlo = (const int*)h->wlo.p; fp.whi = (const int*)h->whi.p;
    fp.S = (const uint8_t*)h->S.p; fp.fstim = (const double*)h->fstim.p; fp.phi = (const double*)h->phi.p;
    fp.Wfrag = (const double*)h->Wfrag.p; fp.bias = (const double*)h->bias.p;
    fp.n_lo = n_lo; fp.npost = pl.npost; fp.nPT = pl.nPT;
    fp.nT16 = h->nT16; fp.tilesPerChunk = pl.tilesPerChunk; fp.nChunks = pl.nChunks; fp.nTiles = pl.nTiles;
    fp.pb_major = pl.pb_major;
    fp.rsf = pl.rsf;
    fp.RP = pl.RP;
    fp.Gpart = (double*)h->Gpart.p; fp.llpart = (double*)h->llpart.p; fp.gbpart = (double*)h->gbpart.p;
    fp.tile0 = pl.tile0;
    fp.t_hi = h->t_hi;
    fp.want_grad = want_grad ? 1 : 0;
    fp.dbg = h->opt_dbg;
    fp.Fimg = (const unsigned char*)h->imgs[h->img_cur].buf.p;
    fp.img_tile0 = h->imgs[h->img_cur].tile0;
    fp.pidx = h->cur_pidx;
    fp.theta = nullptr; fp.Weff = nullptr; fp.P = 1 + h->Dstim + h->Kimp;
    fp.epi64 = h->opt_epi64 ? 2 : 0;
}

// kernels with register-resident Wmat fragments read theta / Weff themselves (no k_prep_w launch)
static bool plan_reads_theta(const Plan& pl)
{
    return pl.version == 6 || (pl.version == 7 && pl.KS <= PGL_WREG_MAX);
}

static int launch_prep(pgl_handle h, const Plan& pl, const Slice& sl, int n_lo, const double* d_theta,
                       const double* d_Weff)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    ENSURE(h->Wfrag, (size_t)pl.nPT * pl.KS * 64 * 8);
    ENSURE(h->bias, (size_t)pl.nPT * 16 * 8);
    const long long total = (long long)pl.nPT * pl.KS * 64;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(k_prep_w, dim3(blocks), dim3(256), 0, h->stream, d_theta, d_Weff,
                       (double*)h->Wfrag.p, (double*)h->bias.p, sl.Ns, h->B, sl.Ds, sl.Ns * h->B,
                       sl.Ns * h->B + sl.Ds, pl.KS, n_lo, pl.npost, pl.nPT, 1,
                       h->N, sl.np0, h->Dstim, sl.ds0, h->cur_pidx);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

static int launch_finalize_grad(pgl_handle h, const Plan& pl, const Slice& sl, int n_lo,
                                const double* d_Weff, double* d_ll, double* d_grad, bool with_ll = false,
                                int kt0 = 0, int nkt = -1, hipStream_t stream = nullptr,
                                const double* wtpart = nullptr, int nwt = 0, int ldy = 0)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    if (nkt < 0) nkt = pl.KT;
    if (!stream) stream = h->stream;
    const long long nfrag = (long long)pl.nPT * nkt * 256;
    // one block per 64-element fragment, its waves share the chunks (>= 32 chunks = 16 KB per wave, at most 8 waves)
    // (measured round 3, tools/step_bench.py + rocprofv3 timeline: the reduction of a SMALL population -- 20 blocks at
    //  C1 -- takes 20 us whatever the number of waves per fragment or loads in flight per lane (8 -> 16 of either):
    //  it is not the latency chain of its loads; 1024-thread blocks cost the 1/8-recording shard of C3 +25 us)
    int nwf = h->opt_finw > 0 ? h->opt_finw : std::max(4, std::min(8, pl.nChunks / 32));
    if (with_ll) nwf = std::max(nwf, 4);                  // the ll blocks reduce with 256 threads (pgl_reduce_ll)
    int blocks = (int)((nfrag + 63) / 64);
    if (with_ll) blocks += pl.npost;                      // trailing blocks (one per neuron) reduce ll and d ll / d bias
    if (with_ll && wtpart) blocks += h->sepBt;            // ... and the w_t partials of the fused stimulus backward
    hipLaunchKernelGGL(k_finalize, dim3(blocks), dim3(64 * nwf), 0, stream, (const double*)h->Gpart.p,
                       (const double*)h->llpart.p, (const double*)h->gbpart.p, d_Weff, d_ll, d_grad,
                       sl.Ns, h->B, sl.Ds, sl.Ns * h->B, sl.Ns * h->B + sl.Ds, pl.KT, n_lo, pl.npost,
                       pl.nPT, pl.nChunks, h->N, sl.np0, h->Dstim, sl.ds0, with_ll ? pl.KSPLIT : 0, kt0,
                       nkt, h->cur_pidx, wtpart, nwt, ldy, h->sepBt);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// Resident feature tiles (k_build_fimg) of the evaluated time range [tile0, tile0 + ntiles) for the
// column split (ktl, kth): built on first use and after every change of spikes / basis / stimulus
// features / time range.  A time-sharded rank (pgl_set_time_range) therefore builds and keeps only its
// own 1/G of the recording.
static int ensure_feature_images(pgl_handle h, int ktl, int kth, int tile0, int ntiles, const Slice* sl = nullptr,
                                 int slice_no = 0, int blk = 0)
{
    if (g_dry) return PGL_OK;                     // (dry run of the dispatch: no device)
    // kth == 0: one image per tile holding all ktl k-tiles (k_fused6; blk: as 2 KB blocks, k_fused8); else the L / H pair
    // of k_fused5.  sl: the images of ONE column slice of a wide population (key carries the slice number)
    const int key = (sl ? (slice_no + 1) << 16 : 0) | (blk ? img_key6(ktl, blk) : ktl << 8 | kth);
    int slot = find_img(h, key, tile0, ntiles);
    if (slot >= 0) {
        h->img_cur = slot;
        h->imgs[slot].stamp = ++h->img_clock;
        return PGL_OK;
    }
    // an empty / stale slot first, else the least recently used one
    slot = 0;
    for (int i = 0; i < pgl_context::NIMG; ++i)
        if (h->imgs[i].key == 0) { slot = i; break; }
        else if (h->imgs[i].stamp < h->imgs[slot].stamp) slot = i;
    pgl_context::ImgSlot& im = h->imgs[slot];
    im.key = 0;
    const size_t bytes = (size_t)ntiles * (kth ? img_pair_bytes(ktl, kth) : img_bytes6(ktl, blk));
    if (bytes > im.buf.cap) {
        // make room before allocating: the other slots' stale buffers go first
        for (int i = 0; i < pgl_context::NIMG; ++i)
            if (i != slot && h->imgs[i].key == 0) release(h->imgs[i].buf);
    }
    ENSURE(im.buf, bytes);
    dim3 grid((unsigned)ntiles, kth ? 2 : 1);
    hipLaunchKernelGGL(k_build_fimg, grid, dim3(256), (size_t)h->B * h->Rk * 8, h->stream,
                       (const int2*)h->spk.p, (const int*)h->wlo.p, (const int*)h->whi.p,
                       (const double*)h->phi.p, (const double*)h->fstim.p, (long long)h->nT, sl ? sl->Ns : h->N, h->B,
                       h->Rk, sl ? sl->Ds : (h->sep ? 0 : h->Dstim), ktl, kth, tile0, (unsigned char*)im.buf.p,
                       h->N, sl ? sl->np0 : 0, h->Dstim, sl ? sl->ds0 : 0, blk);
    HIPCHK(hipGetLastError());
    im.key = key;
    im.tile0 = tile0;
    im.ntiles = ntiles;
    im.stamp = ++h->img_clock;
    h->img_cur = slot;
    return PGL_OK;
}


// PGL_OPT_RECORD_KERNELS: the fused launches of one evaluation go to h->last_kernels while this lives
struct KernelRecord {
    explicit KernelRecord(pgl_context* h)
    {
        if (h->opt_record && !g_dry) {
            h->last_kernels.clear();
            g_rec = &h->last_kernels;
        }
    }
    ~KernelRecord() { g_rec = nullptr; }
};
// the batched Gibbs entry points (pgl_gibbs_ll_cols / pgl_gibbs_update_cols) APPEND the names of their launches, in launch
// order: several calls can follow one another between two reads of pgl_last_kernels (setting the option clears the record)
static inline void record_gibbs(pgl_context* h, const char* name)
{
    if (h->opt_record) h->last_kernels.push_back(name);
}

// Enqueue one evaluation on the handle's stream.  All pointers are device pointers.
//  * one slice (N <= 128 and N*B + Dstim <= 640): prep + fused kernel + finalize;
//  * otherwise the 3-phase path: per slice a forward-only launch accumulating the currents in
//    Xbuf (nT x 16*nPT doubles), one elementwise pass Xbuf -> (ll, r), per slice a backward-only
//    launch.  Same kernels, the F tile is simply generated twice per slice.
// RULE: pgl_plan_kernels runs enqueue_ll_grad, enqueue_hvp_prepare / _apply and enqueue_gibbs_forward with g_dry set on a
// context that has no device, no stream and null buffers -- also inside processes that do have a GPU.  Every device operation
// on these paths must therefore be skipped under g_dry, and the guards live in the steps the evaluations are made of, not in
// the evaluations: launch_kernel (pglm_launch.h) and launch_behind (the k_rescale_* / k_pw_* / k_rw_* launches behind a
// forward pass) record and return, ensure() allocates nothing, the steps below and
// launch_prep, ensure_feature_images, launch_finalize_grad, sep_* / sepf_* return at their top or test g_dry at their one
// device call.  What is left in the enqueue_* functions themselves: the timing events (never recorded by the dry run, whose
// context has opt_timing = 0), the sepD sizing of the fused stimulus backward and the k_hvp_curv launch, each under its own
// test of g_dry.  A device call added to an evaluation belongs in a step with such a guard.

// ---- the steps of an evaluation ----
// per-chunk partial buffers of the fused launches (a forward-only launch still writes its -- unused -- ll partials)
static int ensure_partials(pgl_handle h, const std::vector<Plan>& plans, bool with_G)
{
    size_t maxG = 0, maxLL = 0;
    for (const Plan& pl : plans) {
        maxG = std::max(maxG, (size_t)pl.nChunks * pl.nPT * pl.KT * 256 * 8);
        maxLL = std::max(maxLL, (size_t)pl.nChunks * pl.nPT * pl.KSPLIT * 64 * 8);
    }
    ENSURE(h->llpart, maxLL);
    ENSURE(h->gbpart, maxLL);
    if (with_G) ENSURE(h->Gpart, maxG);
    return PGL_OK;
}

// rows of a row-major slab (nT x xs) the time tiles of a plan cover: [row0, row1), row1 past t_hi inside the last tile
struct RowRange {
    int xs;
    long long row0, row1;
};
static RowRange row_range(const pgl_context* h, const Plan& p0)
{
    return RowRange{p0.nPT * 16, (long long)p0.tile0 * 16, std::min<long long>(h->nT, (long long)(p0.tile0 + p0.nTiles) * 16)};
}
static int zero_slab(pgl_handle h, double* X, const RowRange& rr)
{
    if (g_dry) return PGL_OK;
    HIPCHK(hipMemsetAsync(X + rr.row0 * rr.xs, 0, (size_t)(rr.row1 - rr.row0) * rr.xs * 8, h->stream));
    return PGL_OK;
}

// residual slab of the two-pass kernels (tile-major: 256 doubles per time and post tile)
static int ensure_tile_slab(pgl_handle h, const Plan& pl)
{
    const size_t need = (size_t)pl.nTiles * pl.nPT * 256 * 8;
    const bool fresh = need > h->Xbuf.cap || !h->Xbuf.p;
    ENSURE(h->Xbuf, need);
    // first touch of a fresh allocation costs ~8 % of an evaluation: pay it here, once
    if (fresh && !g_dry) HIPCHK(hipMemsetAsync(h->Xbuf.p, 0, need, h->stream));
    return PGL_OK;
}

// the resident feature tiles a single-slice plan reads: the L / H pair of k_fused5, one-part images of k_fused6 / 7 / 8
static int ensure_plan_images(pgl_handle h, const Plan& pl)
{
    if (pl.version == 5) return ensure_feature_images(h, pl.ktl, pl.kth, pl.tile0, pl.nTiles);
    if (pl.version == 6 || pl.version == 7)
        return ensure_feature_images(h, pl.KT, 0, pl.tile0, pl.nTiles, nullptr, 0, (pl.version == 6 && pl.sb6 == 2) ? 1 + pl.img32 : 0);
    return PGL_OK;
}

// ll (and d ll / d bias, when d_grad) from the per-chunk partials of an evaluation without a gradient
static int launch_finalize_ll(pgl_handle h, const Plan& pl, double* d_ll, double* d_grad)
{
    if (g_dry) return PGL_OK;
    hipLaunchKernelGGL(k_finalize_ll, dim3(pl.npost), dim3(256), 0, h->stream, (const double*)h->llpart.p,
                       (const double*)h->gbpart.p, d_ll, d_grad, 1 + h->Dstim + h->Kimp, pl.npost, pl.nPT, pl.nChunks, pl.KSPLIT);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// phase 1 of the 3-phase path: X += F_s . W_s, one forward-only launch per column slice into the slab X of row stride xs
static int forward_slices(pgl_handle h, const std::vector<Slice>& slices, const std::vector<Plan>& plans, int n_lo,
                          const double* d_theta, const double* d_Weff, double* X, int xs, const char* what)
{
    for (size_t i = 0; i < slices.size(); ++i) {
        int rc = launch_prep(h, plans[i], slices[i], n_lo, d_theta, d_Weff);
        if (rc) return rc;
        FusedParams fp;
        fill_params(h, plans[i], slices[i], n_lo, false, 1, fp);
        fp.Xbuf = X;
        fp.xstride = xs;
        hipError_t e = launch_plan(plans[i], fp, h->stream);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string(what) + hipGetErrorString(e));
    }
    return PGL_OK;
}

// phase 2: one elementwise pass over the rows of h->Xbuf in blocks of 512 rows -- X -> (ll, r) (k_rows_epilogue), or with the
// curvature rows c of a Hessian-vector product r = c * (u + v_bias) (k_hvp_rows_mul) --, the rows past t_hi of the last tile
// zeroed, the per-block sums reduced into d_ll and the bias component of d_out
static int row_pass(pgl_handle h, const Plan& p0, const RowRange& rr, int n_lo, const double* c, double* d_ll, double* d_out)
{
    if (g_dry) return PGL_OK;
    const int rows = 512;
    const long long nrows = h->t_hi - h->t_lo;
    const int nblk = (int)((nrows + rows - 1) / rows);
    ENSURE(h->tmpA, (size_t)nblk * p0.npost * 8);
    ENSURE(h->tmpB, (size_t)nblk * p0.npost * 8);
    const dim3 grid((unsigned)nblk, (unsigned)((p0.npost + 255) / 256));
    if (c)
        hipLaunchKernelGGL(k_hvp_rows_mul, grid, dim3(256), 0, h->stream, (double*)h->Xbuf.p, c, rr.xs, (const double*)h->bias.p,
                           p0.npost, (long long)h->t_lo, (long long)h->t_hi, rows, (double*)h->tmpA.p, (double*)h->tmpB.p);
    else
        hipLaunchKernelGGL(k_rows_epilogue, grid, dim3(256), 0, h->stream, (double*)h->Xbuf.p, rr.xs, (const double*)h->bias.p,
                           (const uint8_t*)h->S.p, h->N, n_lo, p0.npost, (long long)h->t_lo, (long long)h->t_hi, rows, h->nlin,
                           h->dt, (double*)h->tmpA.p, (double*)h->tmpB.p, h->cur_pidx);
    HIPCHK(hipGetLastError());
    if (rr.row1 > h->t_hi) {
        hipLaunchKernelGGL(k_rows_zero, dim3(64), dim3(256), 0, h->stream, (double*)h->Xbuf.p, rr.xs, (long long)h->t_hi, rr.row1);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rows_reduce, dim3(p0.npost), dim3(64), 0, h->stream, (const double*)h->tmpA.p,
                       (const double*)h->tmpB.p, nblk, p0.npost, 1 + h->Dstim + h->Kimp, d_ll, d_out);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// phase 3: G_s = F_s^T . r, per column slice a backward-only launch (d_theta: geometry / bias only) and its reduction
static int backward_slices(pgl_handle h, const std::vector<Slice>& slices, const std::vector<Plan>& plans, int n_lo,
                           const double* d_theta, const double* d_Weff, double* d_ll, double* d_out)
{
    for (size_t i = 0; i < slices.size(); ++i) {
        int rc = launch_prep(h, plans[i], slices[i], n_lo, d_theta, d_Weff);
        if (rc) return rc;
        FusedParams fp;
        fill_params(h, plans[i], slices[i], n_lo, true, 2, fp);
        hipError_t e = launch_plan(plans[i], fp, h->stream);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("backward launch: ") + hipGetErrorString(e));
        rc = launch_finalize_grad(h, plans[i], slices[i], n_lo, d_Weff, d_ll, d_out);
        if (rc) return rc;
    }
    return PGL_OK;
}

static int enqueue_ll_grad(pgl_handle h, int n_lo, int n_hi, const double* d_theta,
                           const double* d_Weff, double* d_ll, double* d_grad)
{
    KernelRecord record(h);
    std::vector<Slice> slices;
    std::vector<Plan> plans;
    bool sepf = false, sliced = false, wide = false;
    {
        int rc = select_plans(h, n_lo, n_hi, slices, plans, sepf, sliced, &wide);
        if (rc) return rc;
    }
    {
        int rc = ensure_partials(h, plans, d_grad != nullptr);
        if (rc) return rc;
    }

    // HIP events of this evaluation (pgl_last_timing / pgl_timing_summary): every PGL_OPT_TIMING-th call only -- an
    // event between two kernels of a stream costs ~6 us of GPU idle time (the next dispatch waits for the marker:
    // rocprofv3 timeline, pass 1 -> pass 2 without an event between them start back to back)
    const bool rec = h->opt_timing > 0 && (h->call_no++ % h->opt_timing) == 0;
    if (rec) {
        h->ev = h->evr[h->ev_launches % pgl_context::NEV];
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
    }
    if (sepf) {
        const Plan& pl = plans[0];
        const bool direct = plan_reads_theta(pl);
        int rc = direct ? PGL_OK : launch_prep(h, pl, slices[0], n_lo, d_theta, d_Weff);
        if (rc) return rc;
        ENSURE(h->Xbuf, (size_t)pl.nTiles * pl.nPT * 256 * 8);
        rc = ensure_plan_images(h, pl);
        if (rc) return rc;
        if (rec) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        SepfParams sp{};
        // up to four post tiles with the (5, 3) table: the stimulus current rides in the forward contraction
        // (where that form is built, fused7_built: up to 13 k-tiles -- slab form beyond)
        const bool fused_fwd = pl.version == 7 && fused7_built(pl.KT, pl.nw7, 2) && h->sepA_ok && h->opt_sepf != 3;
        // ... and its backward too (k_fused7<.., 3>: no residual slab, no k_sepf_bwd) up to 12 k-tiles;
        // dev option 94 = 4 keeps the slab form
        const bool fused_bwd = fused_fwd && d_grad && fused7_built(pl.KT, pl.nw7, 3) && h->opt_sepf != 4;
        rc = sepf_forward(h, pl, d_theta, sp, fused_fwd);
        if (rc) return rc;
        if (fused_bwd && !g_dry) {
            // pieces of the stimulus backward: one per frame base and chunk that holds tiles of it
            const long long q = h->sepq, M = h->sepM;
            const long long tE = (long long)pl.tile0 + pl.nTiles - 1;
            sp.B0 = std::max<long long>(((long long)pl.tile0 * 16) / q - M, 0);
            sp.B1 = std::max<long long>((tE * 16) / q - M, 0);
            const long long span = ((M + 1) * q + 15) / 16 + 1;               // tiles of base 0, the longest
            sp.SL = (int)(span / pl.tilesPerChunk) + 2;
            sp.tilesPerChunk = pl.tilesPerChunk;
            ENSURE(h->sepD, (size_t)(sp.B1 - sp.B0 + 1) * sp.SL * pl.nPT * 320 * 8);
            sp.D = (const double*)h->sepD.p;
        }
        FusedParams fp;
        fill_params(h, pl, slices[0], n_lo, d_grad != nullptr, 0, fp);
        if (direct) {
            fp.theta = d_theta;
            fp.Weff = d_Weff;
        }
        if (fused_fwd) {
            fp.sepA = (const double*)h->sepA.p; fp.sepZ = sp.YfT; fp.sepTheta = d_theta; fp.sepT = h->sepT;
            fp.sepLdy = sp.ldy; fp.sepQ = h->sepq; fp.sepM = h->sepM; fp.sepNH = h->sepNH; fp.sepG = h->sepGs;
            fp.sepBt = h->sepBt;
        }
        if (fused_bwd) {
            fp.sepAT = (const double*)h->sepAT.p; fp.sepD = (double*)h->sepD.p; fp.sepB0 = sp.B0; fp.sepSL = sp.SL;
        }
        hipError_t e = hipSuccess;
        if (pl.version == 5) {                   // pass 1 (slab in, residuals out) and, for the gradient, pass 2
            e = launch_fused5(pl, fp, h->stream, 1, 1);
            if (e == hipSuccess && d_grad) e = launch_fused5(pl, fp, h->stream, 2);
        } else {
            e = launch_fused7(pl, fp, h->stream, fused_bwd ? 3 : (fused_fwd ? 2 : 1));
        }
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("fused launch: ") + hipGetErrorString(e));
        if (d_grad) {
            int nwt = 0;
            rc = sepf_backward(h, sp, d_grad, fused_bwd, &nwt);
            if (rc) return rc;
            if (rec) HIPCHK(hipEventRecord(h->ev[2], h->stream));
            rc = launch_finalize_grad(h, pl, slices[0], n_lo, d_Weff, d_ll, d_grad, true, 0, -1, nullptr,
                                      fused_bwd ? (const double*)h->wpart.p : nullptr, nwt, sp.ldy);
            if (rc) return rc;
        } else {
            if (rec) HIPCHK(hipEventRecord(h->ev[2], h->stream));
            rc = launch_finalize_ll(h, pl, d_ll, d_grad);
            if (rc) return rc;
        }
    } else if (!sliced) {
        const Plan& pl = plans[0];
        const bool direct = plan_reads_theta(pl);
        int rc = direct ? PGL_OK : launch_prep(h, pl, slices[0], n_lo, d_theta, d_Weff);
        if (rc) return rc;
        if ((pl.version == 4 || pl.version == 5) && d_grad) {
            rc = ensure_tile_slab(h, pl);
            if (rc) return rc;
        }
        rc = ensure_plan_images(h, pl);
        if (rc) return rc;
        FusedParams fp;
        fill_params(h, pl, slices[0], n_lo, d_grad != nullptr, 0, fp);
        if (direct) {
            fp.theta = d_theta;
            fp.Weff = d_Weff;
        }
        if (rec) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        // (the two-pass kernel on resident tiles: pass 1 | pass 2 | one reduction of all per-chunk partials.  Until round 3 the
        // first G half was reduced on a side stream "beside" pass 2: the dispatch timeline shows that reduction finishing ~14 us
        // AFTER pass 2 -- whatever the stream priority -- and holding up the second one, 42 us in all against 30 us for a single
        // streaming pass over both halves; at full size the difference is below the noise.)
        hipError_t e = launch_plan(pl, fp, h->stream);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("fused launch: ") + hipGetErrorString(e));
        if (rec) HIPCHK(hipEventRecord(h->ev[2], h->stream));
        // with a gradient one launch: G reduction + (trailing blocks) ll reduction
        rc = d_grad ? launch_finalize_grad(h, pl, slices[0], n_lo, d_Weff, d_ll, d_grad, true) : launch_finalize_ll(h, pl, d_ll, d_grad);
        if (rc) return rc;
    } else if (wide) {
        // a wide population on resident tiles: one image set, one set of Wmat fragments and up to three launches of the two-pass
        // kernel per column slice; currents and residuals travel in the slab
        const Plan& p0 = plans[0];
        const size_t S = slices.size();
        ENSURE(h->Xbuf, (size_t)p0.nTiles * p0.nPT * 256 * 8);
        std::vector<int> slot(S);
        for (size_t i = 0; i < S; ++i) {
            int rc = ensure_feature_images(h, plans[i].ktl, plans[i].kth, p0.tile0, p0.nTiles, &slices[i], (int)i);
            if (rc) return rc;
            slot[i] = h->img_cur;
        }
        if (rec) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        auto params = [&](const size_t i, FusedParams& fp) {
            h->img_cur = slot[i];
            fill_params(h, plans[i], slices[i], n_lo, d_grad != nullptr, 0, fp);
        };
        for (size_t i = 0; i < S; ++i) {                       // forward: the slices add up in the slab; the last one closes
            int rc = launch_prep(h, plans[i], slices[i], n_lo, d_theta, d_Weff);
            if (rc) return rc;
            FusedParams fp;
            params(i, fp);
            const bool last = i + 1 == S;
            hipError_t e = launch_fused5_wide(plans[i], fp, h->stream, last ? 2 : (i == 0 ? 0 : 1));
            if (e == hipSuccess && last && d_grad) e = launch_fused5_wide(plans[i], fp, h->stream, 3);
            if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("wide launch: ") + hipGetErrorString(e));
        }
        if (d_grad) {
            int rc = launch_finalize_grad(h, plans[S - 1], slices[S - 1], n_lo, d_Weff, d_ll, d_grad, true);
            if (rc) return rc;
            for (size_t i = 0; i + 1 < S; ++i) {               // the gradients of the earlier slices from the residuals
                FusedParams fp;
                params(i, fp);
                hipError_t e = launch_fused5_wide(plans[i], fp, h->stream, 4);
                if (e == hipSuccess) e = launch_fused5_wide(plans[i], fp, h->stream, 3);
                if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("wide backward launch: ") + hipGetErrorString(e));
                rc = launch_finalize_grad(h, plans[i], slices[i], n_lo, d_Weff, d_ll, d_grad);
                if (rc) return rc;
            }
        } else {
            int rc = launch_finalize_ll(h, plans[S - 1], d_ll, d_grad);
            if (rc) return rc;
        }
        if (rec) HIPCHK(hipEventRecord(h->ev[2], h->stream));
    } else {
        const Plan& p0 = plans[0];
        const RowRange rr = row_range(h, p0);
        ENSURE(h->Xbuf, (size_t)h->nT * rr.xs * 8);
        double* X = (double*)h->Xbuf.p;
        int rc = zero_slab(h, X, rr);
        if (rc) return rc;
        if (rec) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        SepParams sp;
        if (h->sep) {                                          // phase 0: X = I_stim (separable stimulus)
            if (h->cur_pidx) return fail(PGL_ERR_UNSUPPORTED, "neuron lists with a separable stimulus");
            rc = sep_forward(h, d_theta, p0.npost, X, rr.xs, h->t_lo, h->t_hi, sp);
            if (rc) return rc;
        }
        rc = forward_slices(h, slices, plans, n_lo, d_theta, d_Weff, X, rr.xs, "forward launch: ");
        if (rc) return rc;
        rc = row_pass(h, p0, rr, n_lo, nullptr, d_ll, d_grad);                     // X -> (ll, r)
        if (rc) return rc;
        if (d_grad) {
            rc = backward_slices(h, slices, plans, n_lo, d_theta, d_Weff, d_ll, d_grad);
            if (rc) return rc;
            if (h->sep) {
                rc = sep_backward(h, sp, d_grad);
                if (rc) return rc;
            }
        }
        if (rec) HIPCHK(hipEventRecord(h->ev[2], h->stream));
    }
    if (rec) HIPCHK(hipEventRecord(h->ev[3], h->stream));
    h->timing_valid = rec;
    if (rec) ++h->ev_launches;
    return PGL_OK;
}

int pgl_ll_grad_dev(pgl_handle h, int n_lo, int n_hi, const double* d_theta, const double* d_Weff,
                    double* d_ll, double* d_grad)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_theta || !d_Weff || !d_ll) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    return enqueue_ll_grad(h, n_lo, n_hi, d_theta, d_Weff, d_ll, d_grad);
}

int pgl_ll_grad_list_dev(pgl_handle h, const int* d_idx, int count, const double* d_theta,
                         const double* d_Weff, double* d_ll, double* d_grad)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_idx || !d_theta || !d_Weff || !d_ll) return fail(PGL_ERR_ARG, "null argument");
    if (count <= 0 || count > h->N) return fail(PGL_ERR_ARG, "bad neuron count");
    HIPCHK(hipSetDevice(h->device));
    h->cur_pidx = d_idx;
    rc = enqueue_ll_grad(h, 0, count, d_theta, d_Weff, d_ll, d_grad);
    h->cur_pidx = nullptr;
    return rc;
}


// ---- Hessian-vector products of ll (hessian_rop_wrt_list, pyglm/utils/grads.py:68-95; the hessp of map.py:38-45) ----
// (hvp_select, pglm_plan.h, picks the path; the g_dry RULE above enqueue_ll_grad holds on these paths too)

// theta -> c[t, n] of the rows [n_lo, n_hi) (or of the list h->cur_pidx) over the handle's time range, kept in h->Cbuf
static int enqueue_hvp_prepare(pgl_handle h, int n_lo, int n_hi, const double* d_theta, const double* d_Weff)
{
    KernelRecord record(h);
    std::vector<Slice> slices;
    std::vector<Plan> plans;
    bool fused = false;
    int rc = hvp_select(h, n_lo, n_hi, slices, plans, fused);
    if (rc) return rc;
    rc = ensure_partials(h, plans, false);
    if (rc) return rc;
    const Plan& p0 = plans[0];
    const RowRange rr = row_range(h, p0);
    long long total = 0;
    double* cb = nullptr;
    if (fused) {
        total = (long long)p0.nTiles * p0.nPT * 256;
        ENSURE(h->Cbuf, (size_t)total * 8);
        cb = (double*)h->Cbuf.p;
        rc = launch_prep(h, p0, slices[0], n_lo, d_theta, d_Weff);
        if (rc) return rc;
        rc = ensure_plan_images(h, p0);
        if (rc) return rc;
        FusedParams fp;
        fill_params(h, p0, slices[0], n_lo, false, 0, fp);
        fp.Xbuf = cb;
        hipError_t e = launch_hvp5(p0, fp, nullptr, h->stream, 1);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("curvature forward launch: ") + hipGetErrorString(e));
    } else {
        total = (rr.row1 - rr.row0) * rr.xs;
        ENSURE(h->Cbuf, (size_t)h->nT * rr.xs * 8);
        cb = (double*)h->Cbuf.p + rr.row0 * rr.xs;
        rc = zero_slab(h, (double*)h->Cbuf.p, rr);
        if (rc) return rc;
        rc = forward_slices(h, slices, plans, n_lo, d_theta, d_Weff, (double*)h->Cbuf.p, rr.xs, "curvature forward launch: ");
        if (rc) return rc;
    }
    if (!g_dry) {                                              // x -> c in place
        const int blocks = (int)std::min<long long>((total + 255) / 256, 8 * 1024);
        hipLaunchKernelGGL(k_hvp_curv, dim3(blocks), dim3(256), 0, h->stream, cb, (const double*)h->bias.p,
                           (const uint8_t*)h->S.p, h->N, n_lo, p0.npost, h->cur_pidx, rr.xs, rr.row0, (long long)h->t_hi, total,
                           fused ? 1 : 0, h->nlin, h->dt);
        HIPCHK(hipGetLastError());
    }
    h->hvp_fused = fused;
    return PGL_OK;
}

// H . v of the prepared rows: d_hv (count, P) in the theta layout
static int enqueue_hvp_apply(pgl_handle h, const double* d_v, double* d_hv)
{
    KernelRecord record(h);
    const int n_lo = h->hvp_list ? 0 : h->hvp_n_lo, n_hi = n_lo + h->hvp_count;
    const double* d_Weff = (const double*)h->hvp_Weff.p;
    std::vector<Slice> slices;
    std::vector<Plan> plans;
    bool fused = false;
    int rc = hvp_select(h, n_lo, n_hi, slices, plans, fused);
    if (rc) return rc;
    if (fused != h->hvp_fused) return fail(PGL_ERR_STATE, "the dispatch changed since pgl_hvp_prepare_*: prepare again");
    rc = ensure_partials(h, plans, true);
    if (rc) return rc;
    ENSURE(h->hvp_ll, (size_t)h->hvp_count * 8);               // (the reductions write an "ll" beside the bias component)
    double* d_ll = (double*)h->hvp_ll.p;
    const Plan& p0 = plans[0];
    if (fused) {
        rc = ensure_tile_slab(h, p0);
        if (rc) return rc;
        rc = launch_prep(h, p0, slices[0], n_lo, d_v, d_Weff);
        if (rc) return rc;
        rc = ensure_plan_images(h, p0);
        if (rc) return rc;
        FusedParams fp;
        fill_params(h, p0, slices[0], n_lo, true, 0, fp);
        // u = F . v, r = c * u, the L columns of F^T . r | the H columns from the residual slab | reduction of the partials
        hipError_t e = launch_hvp5(p0, fp, (const double*)h->Cbuf.p, h->stream, 0);
        if (e == hipSuccess) e = launch_fused5(p0, fp, h->stream, 2);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("apply launch: ") + hipGetErrorString(e));
        return launch_finalize_grad(h, p0, slices[0], n_lo, d_Weff, d_ll, d_hv, true);
    }
    // the 3-phase path: u += F_s . V_s | r = c * (u + v_bias) | (H v)_s = F_s^T . r
    const RowRange rr = row_range(h, p0);
    ENSURE(h->Xbuf, (size_t)h->nT * rr.xs * 8);
    double* X = (double*)h->Xbuf.p;
    rc = zero_slab(h, X, rr);
    if (rc) return rc;
    rc = forward_slices(h, slices, plans, n_lo, d_v, d_Weff, X, rr.xs, "forward launch: ");
    if (rc) return rc;
    rc = row_pass(h, p0, rr, n_lo, (const double*)h->Cbuf.p, d_ll, d_hv);
    if (rc) return rc;
    return backward_slices(h, slices, plans, n_lo, d_v, d_Weff, d_ll, d_hv);
}

static int hvp_prepare_common(pgl_handle h, const int* d_idx, int n_lo, int count, const double* d_theta, const double* d_Weff)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_theta || !d_Weff) return fail(PGL_ERR_ARG, "null argument");
    if (h->sep)
        return fail(PGL_ERR_UNSUPPORTED, "Hessian-vector products with a separable stimulus (pgl_set_stimulus_separable): "
                                         "the current is not linear in (w_t, w_x)");
    HIPCHK(hipSetDevice(h->device));
    h->hvp_ok = false;
    h->hvp_host.clear();
    // the apply has no Weff / list argument: the handle keeps its own copies
    ENSURE(h->hvp_Weff, (size_t)h->N * h->N * 8);
    HIPCHK(hipMemcpyAsync(h->hvp_Weff.p, d_Weff, (size_t)h->N * h->N * 8, hipMemcpyDeviceToDevice, h->stream));
    if (d_idx) {
        ENSURE(h->hvp_idx, (size_t)count * 4);
        HIPCHK(hipMemcpyAsync(h->hvp_idx.p, d_idx, (size_t)count * 4, hipMemcpyDeviceToDevice, h->stream));
        h->cur_pidx = (const int*)h->hvp_idx.p;
    }
    rc = enqueue_hvp_prepare(h, n_lo, n_lo + count, d_theta, (const double*)h->hvp_Weff.p);
    h->cur_pidx = nullptr;
    if (rc) return rc;
    h->hvp_list = d_idx != nullptr;
    h->hvp_n_lo = n_lo;
    h->hvp_count = count;
    h->hvp_t_lo = h->t_lo;
    h->hvp_t_hi = h->t_hi;
    h->hvp_ok = true;
    return PGL_OK;
}

int pgl_hvp_prepare_dev(pgl_handle h, int n_lo, int n_hi, const double* d_theta, const double* d_Weff)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    return hvp_prepare_common(h, nullptr, n_lo, n_hi - n_lo, d_theta, d_Weff);
}

int pgl_hvp_prepare_list_dev(pgl_handle h, const int* d_idx, int count, const double* d_theta, const double* d_Weff)
{
    if (!h || !d_idx) return fail(PGL_ERR_ARG, "null argument");
    if (count <= 0 || count > h->N) return fail(PGL_ERR_ARG, "bad neuron count");
    return hvp_prepare_common(h, d_idx, 0, count, d_theta, d_Weff);
}

int pgl_hvp_apply_dev(pgl_handle h, const double* d_v, double* d_hv)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_v || !d_hv) return fail(PGL_ERR_ARG, "null argument");
    if (!h->hvp_ok) return fail(PGL_ERR_STATE, "pgl_hvp_prepare_* has not been called (or the data changed since)");
    if (h->hvp_t_lo != h->t_lo || h->hvp_t_hi != h->t_hi)
        return fail(PGL_ERR_STATE, "the time range changed since pgl_hvp_prepare_*");
    HIPCHK(hipSetDevice(h->device));
    h->cur_pidx = h->hvp_list ? (const int*)h->hvp_idx.p : nullptr;
    rc = enqueue_hvp_apply(h, d_v, d_hv);
    h->cur_pidx = nullptr;
    return rc;
}

int pgl_hvp(pgl_handle h, int n_lo, int n_hi, const double* theta, const double* v, const double* Weff, double* hv_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !v || !Weff || !hv_out) return fail(PGL_ERR_ARG, "null argument");
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    HIPCHK(hipSetDevice(h->device));
    const size_t np = (size_t)(n_hi - n_lo), nP = np * (1 + (size_t)h->Dstim + h->Kimp), nW = (size_t)h->N * h->N;
    PASS(stage_up(h, 0, v, nP * 8));
    PASS(stage_up(h, 1, nullptr, nP * 8));
    // the products of one CG solve share theta: the curvature of an identical (range, time range, theta, Weff) is kept
    const bool same = h->hvp_ok && !h->hvp_list && h->hvp_n_lo == n_lo && h->hvp_count == (int)np && h->hvp_t_lo == h->t_lo &&
                      h->hvp_t_hi == h->t_hi && h->hvp_host.size() == nP + nW &&
                      std::memcmp(h->hvp_host.data(), theta, nP * 8) == 0 &&
                      std::memcmp(h->hvp_host.data() + nP, Weff, nW * 8) == 0;
    if (!same) {
        h->hvp_host.clear();
        PASS(upload_rows(h, h->theta, n_lo, n_hi, theta, Weff));
        PASS(pgl_hvp_prepare_dev(h, n_lo, n_hi, (const double*)h->theta.p, (const double*)h->Weff.p));
        h->hvp_host.assign(theta, theta + nP);
        h->hvp_host.insert(h->hvp_host.end(), Weff, Weff + nW);
    }
    PASS(pgl_hvp_apply_dev(h, (const double*)h->stage[0].p, (double*)h->stage[1].p));
    PASS(stage_down(h, hv_out, h->stage[1].p, nP * 8));
    return stage_end(h);
}

// ---- dense Hessians of ll (hessian_wrt_list, pyglm/utils/grads.py:30-66) ----
// H_n = sum_t c[t, n] f_t f_t^T of the prepared rows, from the curvature the last prepare left in h->Cbuf: per launch of
// hess_plan's rows the Gram contraction k_hess into chunk partials, then k_hess_reduce (chunk order, Weff, theta layout, both
// triangles).  The g_dry RULE above enqueue_ll_grad holds here too.
static int enqueue_hess(pgl_handle h, double* d_H, int ld)
{
    KernelRecord record(h);
    HessPlan hp;
    int rc = hess_plan(h, h->hvp_count, hp);
    if (rc) return rc;
    ENSURE(h->hess_part, hp.partBytes);
    HessParams kp{};
    kp.nT = h->nT; kp.t_hi = h->t_hi;
    kp.N = h->N; kp.B = h->B; kp.R = h->Rk; kp.RP = hp.RP; kp.Dstim = h->Dstim; kp.Kimp = h->Kimp;
    kp.K = h->Kimp + h->Dstim + 1;
    kp.spk = (const int2*)h->spk.p; kp.wlo = (const int*)h->wlo.p; kp.whi = (const int*)h->whi.p;
    kp.fstim = (const double*)h->fstim.p; kp.phi = (const double*)h->phi.p;
    kp.C = (const double*)h->Cbuf.p;
    kp.cxs = 16 * ((h->hvp_count + 15) / 16);
    kp.tile0 = (int)(h->t_lo / 16);
    kp.nTiles = (int)((h->t_hi + 15) / 16) - kp.tile0;
    kp.nChunks = hp.nChunks; kp.tilesPerChunk = hp.tilesPerChunk;
    kp.nPairs = hp.nPairs;
    kp.part = (double*)h->hess_part.p;
    for (int r0 = 0; r0 < h->hvp_count; r0 += hp.rowsPerLaunch) {
        kp.r0 = r0;
        kp.count = std::min(hp.rowsPerLaunch, h->hvp_count - r0);
        kp.nGroups = (kp.count + 7) / 8;
        const long long blocks = (long long)kp.nPairs * kp.nGroups * kp.nChunks;
        if (blocks > 0x7fffffffLL) return fail(PGL_ERR_UNSUPPORTED, "dense Hessian: grid too large");
        hipError_t e = launch_hess(kp, h->hvp_fused ? 1 : 0, (unsigned)blocks, hp.lds, h->stream);
        if (e != hipSuccess) return fail(PGL_ERR_HIP, std::string("Hessian launch: ") + hipGetErrorString(e));
        if (!g_dry) {
            hipLaunchKernelGGL(k_hess_reduce, dim3(kp.nPairs, kp.count), dim3(256), 0, h->stream, kp,
                               (const double*)h->hvp_Weff.p, h->hvp_list ? (const int*)h->hvp_idx.p : nullptr, h->hvp_n_lo, d_H, ld);
            HIPCHK(hipGetLastError());
        }
    }
    return PGL_OK;
}

int pgl_hess_dev(pgl_handle h, double* d_H, int ld)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_H) return fail(PGL_ERR_ARG, "null argument");
    if (h->sep)
        return fail(PGL_ERR_UNSUPPORTED, "dense Hessians with a separable stimulus (pgl_set_stimulus_separable): "
                                         "the current is not linear in (w_t, w_x)");
    if (!h->hvp_ok) return fail(PGL_ERR_STATE, "pgl_hvp_prepare_* has not been called (or the data changed since)");
    if (h->hvp_t_lo != h->t_lo || h->hvp_t_hi != h->t_hi)
        return fail(PGL_ERR_STATE, "the time range changed since pgl_hvp_prepare_*");
    if (ld < 1 + h->Dstim + h->Kimp) return fail(PGL_ERR_ARG, "ld < P");
    HIPCHK(hipSetDevice(h->device));
    return enqueue_hess(h, d_H, ld);
}

int pgl_hess(pgl_handle h, int n_lo, int n_hi, const double* theta, const double* Weff, double* H_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff || !H_out) return fail(PGL_ERR_ARG, "null argument");
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    HIPCHK(hipSetDevice(h->device));
    const size_t P = 1 + (size_t)h->Dstim + h->Kimp, bytes = (size_t)(n_hi - n_lo) * P * P * 8;
    PASS(upload_rows(h, h->theta, n_lo, n_hi, theta, Weff));
    PASS(pgl_hvp_prepare_dev(h, n_lo, n_hi, (const double*)h->theta.p, (const double*)h->Weff.p));
    PASS(stage_up(h, 0, nullptr, bytes));
    PASS(pgl_hess_dev(h, (double*)h->stage[0].p, (int)P));
    PASS(stage_down(h, H_out, h->stage[0].p, bytes));
    return stage_end(h);
}

// the lock-step entry points, BFGS bookkeeping through proximal gradient (inside extern "C")
#include "pglm_capi_rows.h"

int pgl_sync(pgl_handle h)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

int pgl_ll_grad(pgl_handle h, int n_lo, int n_hi, const double* theta, const double* Weff,
                double* ll_out, double* grad_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff || !ll_out) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (n_lo < 0 || n_hi > h->N || n_lo >= n_hi) return fail(PGL_ERR_ARG, "bad neuron range");
    const size_t np = (size_t)(n_hi - n_lo), gb = np * (1 + (size_t)h->Dstim + h->Kimp) * 8;
    PASS(upload_rows(h, h->theta, n_lo, n_hi, theta, Weff));
    ENSURE(h->ll, np * 8);
    if (grad_out) ENSURE(h->grad, gb);
    PASS(enqueue_ll_grad(h, n_lo, n_hi, (const double*)h->theta.p, (const double*)h->Weff.p,
                         (double*)h->ll.p, grad_out ? (double*)h->grad.p : nullptr));
    PASS(stage_down(h, ll_out, h->ll.p, np * 8));
    PASS(stage_down(h, grad_out, h->grad.p, gb));
    return stage_end(h);
}

int pgl_last_timing(pgl_handle h, double* fused_ms, double* total_ms)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!h->timing_valid) return fail(PGL_ERR_STATE, "the last pgl_ll_grad call recorded no events (none yet, or PGL_OPT_TIMING skipped it)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev[3]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, h->ev[1], h->ev[2]));
    HIPCHK(hipEventElapsedTime(&b, h->ev[0], h->ev[3]));
    if (fused_ms) *fused_ms = a;
    if (total_ms) *total_ms = b;
    return PGL_OK;
}

int pgl_timing_summary(pgl_handle h, int reset, int* n_launches, double* mean_fused_ms, double* mean_total_ms)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long n = std::min<long long>(h->ev_launches, pgl_context::NEV);
    double sa = 0, sb = 0;
    for (long long i = 0; i < n; ++i) {
        hipEvent_t* ev = h->evr[(h->ev_launches - 1 - i) % pgl_context::NEV];
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, ev[1], ev[2]));
        HIPCHK(hipEventElapsedTime(&b, ev[0], ev[3]));
        sa += a;
        sb += b;
    }
    if (n_launches) *n_launches = (int)n;
    if (mean_fused_ms) *mean_fused_ms = n ? sa / n : 0.0;
    if (mean_total_ms) *mean_total_ms = n ? sb / n : 0.0;
    if (reset) h->ev_launches = 0;
    return PGL_OK;
}

int pgl_set_stream(pgl_handle h, void* stream)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));          // drain work queued on the previous stream
    h->stream = stream ? (hipStream_t)stream : h->own_stream;
    h->ev_launches = 0;
    h->timing_valid = false;
    return PGL_OK;
}

static int enqueue_gibbs_forward(pgl_handle h);
static int enqueue_rescale(pgl_handle h, double* d_tau, const long long* d_off, double* d_stats, bool corr = false,
                           unsigned long long seed = 0, long long draw = 0);
static int enqueue_pointwise(pgl_handle h, int block_chunks, double* d_ll_blk, double* d_acc, long long draw);
static int enqueue_rate_windows(pgl_handle h, long long win, double* d_lam, double* d_obs, double* d_acc, long long draw);
static int enqueue_decode_prepare(pgl_handle h);
static int enqueue_decode_eval(pgl_handle h, const double* d_u, int64_t Tu, int q, const PglDecPrior& prior, double* d_F,
                               double* d_grad_u);
static int enqueue_decode_hvp(pgl_handle h, const double* d_v, double* d_hv);
static int enqueue_acf(pgl_handle h, const double* d_tau, const int64_t* d_run_off, const int64_t* d_seg_run, int64_t M, int max_lag,
                       double* d_out, double* d_scores);

int pgl_last_kernels(pgl_handle h, char* out, int cap)
{
    if (!h || !out || cap <= 0) return fail(PGL_ERR_ARG, "null argument");
    if (!h->opt_record) return fail(PGL_ERR_STATE, "kernel recording is off (PGL_OPT_RECORD_KERNELS)");
    std::string all;
    for (const std::string& n : h->last_kernels) all += n + "\n";
    if ((int)all.size() + 1 > cap) return fail(PGL_ERR_ARG, "output buffer too small");
    std::memcpy(out, all.c_str(), all.size() + 1);
    return PGL_OK;
}

// Dry run of the dispatch, no device needed: the fused kernel instantiations (names as in the code object) that an
// ll(+grad) evaluation of `count` neurons starting at n_lo -- a range, or a list -- of a population of this shape would
// launch, one per line in `out`.  stim: 0 none / dense stimulus columns (Dstim of them), 1 separable stimulus by the
// tap-rate kernels, 2 separable at the frame rate with the stimulus current inside the fused forward where that form
// exists, 3 at the frame rate through the slab.  path: 0 ll+grad, 1 ll only, 2 the forward launches of pgl_gibbs_prepare_all,
// 3 the launches of pgl_hvp_prepare_*, 4 those of pgl_hvp_apply_dev after such a prepare (k_hvp5 and the fused kernels around
// it; stim >= 1: PGL_ERR_UNSUPPORTED, as the real call), 5 the k_hess launches of pgl_hess_dev after such a prepare,
// 6 the launches of pgl_rescale_dev (the forward launches of path 2, then the k_rescale_* kernels), 7 those of
// pgl_pointwise_dev (the forward launches of path 2, then k_pw_chunk and k_pw_block), 8 those of pgl_rate_windows_dev (the
// forward launches of path 2, then k_rw_piece and k_rw_window), 9 those of pgl_rescale_corr_dev (the forward launches of path 2,
// then k_rcorr_chunk, k_rescale_scan and k_rcorr_finish), 10 the launch of pgl_rescale_acf_dev alone (no forward pass: the
// shape is ignored), 11 the launches of pgl_decode_prepare_dev and a pgl_decode_eval_dev with a gradient behind it, 12 those of
// pgl_decode_hvp_dev behind them (Dstim read as one stimulus dimension of Dstim basis functions over R taps).
int pgl_plan_kernels(int N, int B, int R, int Dstim, long long nT, int stim, int n_lo, int count, int path, int opt_kernel,
                     int opt_f32, char* out, int cap)
{
    if (!out || cap <= 0) return fail(PGL_ERR_ARG, "null argument");
    if (N <= 0 || B <= 0 || B > PGL_MAXB || R <= 0 || nT <= 0 || Dstim < 0 || count <= 0 || n_lo < 0 || n_lo + count > N)
        return fail(PGL_ERR_ARG, "bad shape");
    pgl_context c;
    c.N = N; c.B = B; c.R = R; c.Rk = R; c.nT = nT; c.Dstim = Dstim; c.Kimp = N * B;
    c.nT16 = (int)((nT + 15) / 16); c.t_lo = 0; c.t_hi = nT; c.numCU = 256;
    c.sep = stim >= 1; c.sepf = stim >= 2; c.sepA_ok = stim == 2; c.opt_sepf = 0;
    c.Ktot = c.Kimp + (c.sep ? 0 : Dstim);
    c.opt_kernel = opt_kernel; c.opt_f32 = (opt_f32 == 1) ? 1 : 0; c.opt_img32 = (opt_f32 == 2) ? 1 : 0;
    c.opt_timing = 0;
    // the evaluation itself, enqueued on the device-less context: the launch sequence is the one a real call takes
    std::vector<std::string> names;
    double dummy = 0;
    int rc = PGL_OK;
    if (path == 3 || path == 4 || path == 5) {
        // pgl_hvp_prepare_* (3), pgl_hvp_apply_dev (4) / pgl_hess_dev (5) after such a prepare: they take range and path from it
        if (c.sep) return fail(PGL_ERR_UNSUPPORTED, "Hessian-vector products with a separable stimulus");
        std::vector<std::string> prep;
        g_dry = (path == 3) ? &names : &prep;
        rc = enqueue_hvp_prepare(&c, n_lo, n_lo + count, nullptr, nullptr);
        if (rc == PGL_OK && path != 3) {
            c.hvp_n_lo = n_lo;
            c.hvp_count = count;
            g_dry = &names;
            rc = (path == 4) ? enqueue_hvp_apply(&c, nullptr, &dummy) : enqueue_hess(&c, &dummy, 1 + Dstim + c.Kimp);
        }
    } else if (path == 11 || path == 12) {
        // pgl_decode_prepare_dev + pgl_decode_eval_dev (11), pgl_decode_hvp_dev behind them (12): Dstim basis functions of one
        // stimulus dimension over R taps
        if (c.sep) return fail(PGL_ERR_UNSUPPORTED, "stimulus decoding with a separable stimulus");
        if (Dstim < 1) return fail(PGL_ERR_UNSUPPORTED, "stimulus decoding needs a 'basis' stimulus");
        c.dec_stim = true; c.dec_Rt = R; c.dec_B = Dstim; c.dec_D = 1;
        const PglDecPrior prior = {0.0, 1.0, 0.0};
        std::vector<std::string> before;
        g_dry = (path == 11) ? &names : &before;
        rc = enqueue_decode_prepare(&c);
        if (rc == PGL_OK) rc = enqueue_decode_eval(&c, &dummy, 1, 1, prior, &dummy, &dummy);
        g_dry = &names;
        if (rc == PGL_OK && path == 12) rc = enqueue_decode_hvp(&c, &dummy, &dummy);
    } else {
        g_dry = &names;
        rc = (path == 10) ? enqueue_acf(&c, &dummy, nullptr, nullptr, 1, 1, &dummy, &dummy)
           : (path == 2 || path == 6 || path == 7 || path == 8 || path == 9) ? enqueue_gibbs_forward(&c)
                         : enqueue_ll_grad(&c, n_lo, n_lo + count, nullptr, nullptr, &dummy, path == 0 ? &dummy : nullptr);
    }
    if (rc == PGL_OK && path == 6) rc = enqueue_rescale(&c, &dummy, nullptr, &dummy);
    if (rc == PGL_OK && path == 7) rc = enqueue_pointwise(&c, 1, &dummy, nullptr, 0);
    if (rc == PGL_OK && path == 8) rc = enqueue_rate_windows(&c, 50, &dummy, nullptr, nullptr, 0);
    if (rc == PGL_OK && path == 9) rc = enqueue_rescale(&c, &dummy, nullptr, &dummy, true);
    g_dry = nullptr;
    // (under g_dry nothing but a dispatch (pglm_launch.h) without an instantiation for the plan fails with PGL_ERR_HIP)
    if (rc == PGL_ERR_HIP) return fail(PGL_ERR_UNSUPPORTED, "no kernel instantiation for this plan");
    if (rc) return rc;
    std::string all;
    for (const std::string& n : names) all += n + "\n";
    if ((int)all.size() + 1 > cap) return fail(PGL_ERR_ARG, "output buffer too small");
    std::memcpy(out, all.c_str(), all.size() + 1);
    return PGL_OK;
}

int pgl_info(pgl_handle h, int n_lo, int n_hi, double* info, int n_info)
{
    if (!h || !info) return fail(PGL_ERR_ARG, "null argument");
    std::vector<Slice> slices;
    // the stimulus path an evaluation would take: 0 none / dense feature columns, 1 separable by the tap-rate kernels on
    // the 3-phase path, 2 separable at the frame rate (k_sepf_*, impulse columns on resident tiles)
    std::vector<Plan> plans;
    bool sepf = false, sliced = false, wide = false;
    int rc = select_plans(h, n_lo, n_hi, slices, plans, sepf, sliced, &wide);
    if (rc) return rc;
    const int stim_path = sepf ? 2 : (h->sep ? 1 : 0);
    const Plan& pl = plans[0];
    const double P = 1.0 + h->Dstim + h->Kimp;
    double v[13];
    v[12] = stim_path;
    v[9] = pl.version;                       // 1 4-wave, 2 K-split, 3 K-split f32, 4 two-pass, 5 two-pass on resident feature tiles
    v[10] = (pl.version == 5) ? (double)pl.nTiles * (double)img_pair_bytes(pl.ktl, pl.kth)
            : (pl.version == 6 || pl.version == 7) ? (double)pl.nTiles * (double)img_bytes6(pl.KT, (pl.version == 6 && pl.sb6 == 2) ? 1 + pl.img32 : 0) : 0.0;   // resident feature bytes
    // HBM bytes the hot kernels stream per evaluation beyond the algorithmic ones (feature tiles read in
    // pass 1 and the H part again in pass 2, residual slab written and read)
    v[11] = (pl.version == 5) ? v[10] + (double)pl.nTiles * pgl_img_bytes(pl.kth) + 2.0 * (double)pl.nTiles * pl.nPT * 2048.0
            : (pl.version == 4) ? 2.0 * (double)pl.nTiles * pl.nPT * 2048.0
            : (pl.version == 6 || pl.version == 7) ? v[10] * pl.nPB : 0.0;
    if (wide) {                              // every column slice has its image set; each post block streams all of them
        v[10] = v[11] = 0.0;
        for (const Plan& q : plans) {
            const double b = (double)q.nTiles * (double)img_pair_bytes(q.ktl, q.kth);
            v[10] += b;
            v[11] += 2.0 * b * q.nPB;
        }
        v[11] += 2.0 * (double)plans.size() * (double)pl.nTiles * pl.nPT * 2048.0;
    }
    v[0] = pl.blocks; v[1] = pl.threads; v[2] = pl.nChunks; v[3] = pl.KT; v[4] = (double)pl.lds;
    v[5] = 16;
    const double nrows = (double)(h->t_hi - h->t_lo);
    v[6] = 4.0 * nrows * (double)h->Ktot * (double)pl.npost;
    // nT*N*1 (u8 counts) + nT*Dstim*8 + params in + (ll+grad) out
    v[7] = nrows * h->N + (h->sep ? (double)h->sepT * h->sepBx * 8.0 : nrows * h->Dstim * 8.0) + 8.0 * pl.npost * P +
           8.0 * pl.npost * (1.0 + P);          // separable: the projected stimulus at its frame rate
    v[8] = (double)h->nnz;
    for (int i = 0; i < n_info && i < 13; ++i) info[i] = v[i];
    return PGL_OK;
}

int pgl_features(pgl_handle h, double* fS_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!fS_out) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->nT * h->Kimp * 8;
    ENSURE(h->tmpA, bytes);
    hipLaunchKernelGGL(k_features, dim3(h->nT16), dim3(256), (size_t)h->B * h->Rk * 8, h->stream,
                       (const int2*)h->spk.p, (const int*)h->wlo.p, (const int*)h->whi.p,
                       (const double*)h->phi.p, (double*)h->tmpA.p, (long long)h->nT, h->N, h->B, h->Rk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fS_out, h->tmpA.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

// I_impT (N,nT) on device for impulse weights d_w (N,B)
static int enqueue_impulse_T(pgl_handle h, const double* d_w)
{
    ENSURE(h->IimpT, (size_t)h->N * h->nT * 8);
    const int blocks = (int)((h->nT + 63) / 64);
    const size_t lds = ((size_t)h->B * h->Rk + (size_t)h->N * h->B) * 8;
    hipLaunchKernelGGL(k_impulse_T, dim3(blocks), dim3(256), lds, h->stream, (const int2*)h->spk.p,
                       (const int*)h->wlo.p, (const int*)h->whi.p, (const double*)h->phi.p, d_w,
                       (double*)h->IimpT.p, (long long)h->nT, h->nT16, h->N, h->B, h->Rk);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_impulse_currents(pgl_handle h, const double* w, double* I_imp_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!w || !I_imp_out) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    ENSURE(h->wsmall, (size_t)h->Kimp * 8);
    HIPCHK(hipMemcpyAsync(h->wsmall.p, w, (size_t)h->Kimp * 8, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_impulse_T(h, (const double*)h->wsmall.p);
    if (rc) return rc;
    h->gibbs_npost = -1;
    std::vector<double> T((size_t)h->N * h->nT);
    HIPCHK(hipMemcpyAsync(T.data(), h->IimpT.p, T.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int n = 0; n < h->N; ++n)
        for (int64_t t = 0; t < h->nT; ++t) I_imp_out[(size_t)t * h->N + n] = T[(size_t)n * h->nT + t];
    return PGL_OK;
}

int pgl_gibbs_prepare(pgl_handle h, int n_post, const double* theta_n, const double* Weff_col)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta_n || !Weff_col) return fail(PGL_ERR_ARG, "null argument");
    if (n_post < 0 || n_post >= h->N) return fail(PGL_ERR_ARG, "n_post out of range");
    HIPCHK(hipSetDevice(h->device));
    const size_t P = 1 + (size_t)h->Dstim + h->Kimp;
    ENSURE(h->thetan, P * 8);
    ENSURE(h->wcol, (size_t)h->N * 8);
    ENSURE(h->Inet, (size_t)h->nT * 8);
    ENSURE(h->Istim, (size_t)h->nT * 8);
    HIPCHK(hipMemcpyAsync(h->thetan.p, theta_n, P * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->wcol.p, Weff_col, (size_t)h->N * 8, hipMemcpyHostToDevice, h->stream));
    const double* d_th = (const double*)h->thetan.p;
    rc = enqueue_impulse_T(h, d_th + 1 + h->Dstim);
    if (rc) return rc;
    hipLaunchKernelGGL(k_inet, dim3(1024), dim3(256), 0, h->stream, (const double*)h->IimpT.p,
                       (const double*)h->wcol.p, (const double*)h->fstim.p, d_th + 1,
                       (double*)h->Inet.p, (double*)h->Istim.p, (long long)h->nT, h->N, h->sep ? 0 : h->Dstim);
    HIPCHK(hipGetLastError());
    if (h->sep) {                                 // I_stim of this neuron by the separable path
        SepParams sp;
        rc = sep_forward(h, d_th, 1, (double*)h->Istim.p, 1, 0, h->nT, sp);
        if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->gibbs_npost = n_post;
    h->gibbs_bias = theta_n[0];
    return PGL_OK;
}

// events of neuron n inside the handle's time range [t_lo, t_hi): indices into spk, from the host copy of the event lists
static void event_range(const pgl_context* h, int n, int& lo, int& hi)
{
    const int2* evb = h->h_ev.data();
    const auto before = [](const int2& e, int64_t t) { return (int64_t)e.x < t; };
    const int2* b = evb + h->h_ptr[n];
    const int2* e = evb + h->h_ptr[n + 1];
    lo = (int)(std::lower_bound(b, e, h->t_lo, before) - evb);
    hi = (int)(std::lower_bound(b, e, h->t_hi, before) - evb);
}

static int run_ll_current(pgl_handle h, const double* d_base, const double* d_stim,
                          const double* d_col, int n_post, double bias, double aw_cur,
                          const double* w, int K, double* ll_out)
{
    // blocks of the streaming part; the spike-bin part writes one more partial row
    // the sums run over the evaluated time range [t_lo, t_hi) (pgl_set_time_range)
    const int nblocks = (int)std::min<int64_t>(1024, (h->t_hi - h->t_lo + 255) / 256);
    int e_lo, e_hi;
    event_range(h, n_post, e_lo, e_hi);
    const int sblocks = std::max(1, std::min(256, (e_hi - e_lo + 255) / 256));
    ENSURE(h->part, (size_t)(nblocks + sblocks) * PGL_KMAX * 8);
    ENSURE(h->outK, PGL_KMAX * 8);
    if (!h->pin_out) HIPCHK(hipHostMalloc((void**)&h->pin_out, PGL_KMAX * 8, hipHostMallocDefault));
    for (int k0 = 0; k0 < K; k0 += PGL_KMAX) {
        const int kk = std::min(PGL_KMAX, K - k0);
        PglWeights wv;
        for (int k = 0; k < PGL_KMAX; ++k) wv.w[k] = (k < kk) ? w[k0 + k] : 0.0;
        hipLaunchKernelGGL(k_ll_current, dim3(nblocks), dim3(256), 0, h->stream, d_base, d_stim,
                           d_col, bias, aw_cur, wv, kk, h->nlin, h->dt,
                           (long long)h->t_lo, (long long)h->t_hi, (double*)h->part.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ll_current_spikes, dim3(sblocks), dim3(256), 0, h->stream,
                           (const int2*)h->spk.p, e_lo, e_hi, d_base, d_stim, d_col, bias, aw_cur,
                           wv, kk, h->nlin,
                           (double*)h->part.p + (size_t)nblocks * PGL_KMAX);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_reduce_parts, dim3(kk), dim3(64), 0, h->stream, (const double*)h->part.p,
                           nblocks + sblocks, kk, (double*)h->outK.p);
        HIPCHK(hipGetLastError());
        // results through a pinned buffer: a pageable destination makes the copy a staged, slower one
        // (a single launch with a last-ticket reduction into host memory measured the same 56 us:
        // its agent-scope fences cost what the two launches do)
        HIPCHK(hipMemcpyAsync(h->pin_out, h->outK.p, (size_t)kk * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        std::memcpy(ll_out + k0, h->pin_out, (size_t)kk * 8);
    }
    return PGL_OK;
}

int pgl_gibbs_ll(pgl_handle h, int n_pre, double aw_cur, const double* w, int K, double* ll_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->gibbs_npost < 0) return fail(PGL_ERR_STATE, "pgl_gibbs_prepare has not been called");
    if (!w || !ll_out || K <= 0) return fail(PGL_ERR_ARG, "bad argument");
    if (n_pre < 0 || n_pre >= h->N) return fail(PGL_ERR_ARG, "n_pre out of range");
    HIPCHK(hipSetDevice(h->device));
    const double* col = (const double*)h->IimpT.p + (size_t)n_pre * h->nT;
    return run_ll_current(h, (const double*)h->Inet.p, (const double*)h->Istim.p, col,
                          h->gibbs_npost, h->gibbs_bias, aw_cur, w, K, ll_out);
}

int pgl_gibbs_update(pgl_handle h, int n_pre, double delta)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->gibbs_npost < 0) return fail(PGL_ERR_STATE, "pgl_gibbs_prepare has not been called");
    if (n_pre < 0 || n_pre >= h->N) return fail(PGL_ERR_ARG, "n_pre out of range");
    HIPCHK(hipSetDevice(h->device));
    const double* col = (const double*)h->IimpT.p + (size_t)n_pre * h->nT;
    hipLaunchKernelGGL(k_axpy, dim3(1024), dim3(256), 0, h->stream, (double*)h->Inet.p, col, delta,
                       (long long)h->nT);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// ---- batched column Gibbs: all post-synaptic columns on the device at once ----------------------
// host theta (N, P) / Weff (N, N) of one draw -> h->gtheta / h->Weff, the device is current
static int upload_draw(pgl_handle h, const double* theta, const double* Weff)
{
    PASS(upload_rows(h, h->gtheta, 0, h->N, theta, Weff));
    // pgl_gibbs_prepare_all returns with the work enqueued, and the caller's (pageable) theta / Weff may be temporaries that
    // die then: the uploads must have left host memory, whatever the runtime does with pageable sources
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

int pgl_gibbs_prepare_all(pgl_handle h, const double* theta, const double* Weff)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    rc = upload_draw(h, theta, Weff);
    if (rc) return rc;
    return enqueue_gibbs_forward(h);
}

// forward-only launches of the K-split kernel: GX[t][n] = sum_slices F_s . W_s (stimulus columns
// included), the same phase 1 as the sliced ll+grad path; theta / Weff already in h->gtheta / h->Weff.
// The dry run of the dispatch runs this too: the RULE above enqueue_ll_grad holds here.
static int enqueue_gibbs_forward(pgl_handle h)
{
    KernelRecord record(h);
    const int N = h->N;
    int rc = PGL_OK;
    const std::vector<Slice> slices = make_slices(h);
    std::vector<Plan> plans(slices.size());
    for (size_t i = 0; i < slices.size(); ++i) {
        rc = make_plan(h, 0, N, slices[i], plans[i], false);
        if (rc) return rc;
    }
    rc = ensure_partials(h, plans, false);
    if (rc) return rc;
    const RowRange rr = row_range(h, plans[0]);
    ENSURE(h->GX, (size_t)h->nT * rr.xs * 8);
    rc = zero_slab(h, (double*)h->GX.p, rr);
    if (rc) return rc;
    if (h->sep) {
        SepParams sp;
        rc = sep_forward(h, (const double*)h->gtheta.p, N, (double*)h->GX.p, rr.xs, h->t_lo, h->t_hi, sp);
        if (rc) return rc;
    }
    rc = forward_slices(h, slices, plans, 0, (const double*)h->gtheta.p, (const double*)h->Weff.p, (double*)h->GX.p, rr.xs,
                        "forward launch: ");
    if (rc) return rc;
    h->gx_xs = rr.xs;
    h->gx_t_lo = h->t_lo;
    h->gx_t_hi = h->t_hi;
    return PGL_OK;
}

static int check_cols(const pgl_context* h, int ncols, const int* n_post, const int* n_pre, const double* w)
{
    if (h->gx_xs == 0) return fail(PGL_ERR_STATE, "pgl_gibbs_prepare_all has not been called");
    if (h->gx_t_lo != h->t_lo || h->gx_t_hi != h->t_hi)
        return fail(PGL_ERR_STATE, "time range changed since pgl_gibbs_prepare_all");
    if (ncols <= 0 || !n_post || !n_pre || !w) return fail(PGL_ERR_ARG, "bad argument");
    for (int c = 0; c < ncols; ++c)
        if (n_post[c] < 0 || n_post[c] >= h->N || n_pre[c] < 0 || n_pre[c] >= h->N)
            return fail(PGL_ERR_ARG, "neuron index out of range");
    return PGL_OK;
}

// device copies of the column arguments (stage_cols)
struct ColsArgs {
    const int *cols, *pre, *elo, *ehi;   // elo / ehi: the events of every n_post inside the time range (null unless asked for)
    const double *aw, *w;
    int max_ev;                          // largest ehi - elo
};

// stage the column arguments in one pinned block, one H2D copy: [cols | pre | aw | w | elo | ehi]; the block holds at least
// out_bytes, for the results of the call
static int stage_cols(pgl_handle h, int ncols, const int* n_post, const int* n_pre, const double* aw, const double* w, int nw,
                      bool with_events, size_t out_bytes, ColsArgs& a)
{
    const size_t o_pre = (size_t)ncols * 4, o_aw = ((o_pre + (size_t)ncols * 4 + 7) / 8) * 8;
    const size_t o_w = o_aw + (size_t)ncols * 8, o_elo = o_w + (size_t)ncols * nw * 8;
    const size_t o_ehi = o_elo + (size_t)ncols * 4;
    const size_t bytes = with_events ? ((o_ehi + (size_t)ncols * 4 + 7) / 8) * 8 : o_elo;
    const size_t need = std::max(bytes, out_bytes);
    if (need > h->pin_args_cap) {
        if (h->pin_args) (void)hipHostFree(h->pin_args);
        h->pin_args = nullptr;
        h->pin_args_cap = 0;
        HIPCHK(hipHostMalloc((void**)&h->pin_args, need * 2, hipHostMallocDefault));
        h->pin_args_cap = need * 2;
    }
    ENSURE(h->gargs, bytes);
    std::memcpy(h->pin_args, n_post, (size_t)ncols * 4);
    std::memcpy(h->pin_args + o_pre, n_pre, (size_t)ncols * 4);
    for (int c = 0; c < ncols; ++c) reinterpret_cast<double*>(h->pin_args + o_aw)[c] = aw ? aw[c] : 0.0;
    std::memcpy(h->pin_args + o_w, w, (size_t)ncols * nw * 8);
    a.max_ev = 0;
    if (with_events) {
        int* lo = reinterpret_cast<int*>(h->pin_args + o_elo);
        int* hi = reinterpret_cast<int*>(h->pin_args + o_ehi);
        for (int c = 0; c < ncols; ++c) {
            event_range(h, n_post[c], lo[c], hi[c]);
            a.max_ev = std::max(a.max_ev, hi[c] - lo[c]);
        }
    }
    HIPCHK(hipMemcpyAsync(h->gargs.p, h->pin_args, bytes, hipMemcpyHostToDevice, h->stream));
    const unsigned char* d = (const unsigned char*)h->gargs.p;
    a.cols = (const int*)d; a.pre = (const int*)(d + o_pre); a.aw = (const double*)(d + o_aw); a.w = (const double*)(d + o_w);
    a.elo = with_events ? (const int*)(d + o_elo) : nullptr;
    a.ehi = with_events ? (const int*)(d + o_ehi) : nullptr;
    return PGL_OK;
}

// what the k_gibbs_* kernels read of the handle, the staged arguments and the plan; the launchers add their own buffers
static GibbsColsParams cols_params(const pgl_context* h, const ColsArgs& a, int ncols, int nw, const PglGibbsPlan& pl)
{
    GibbsColsParams gp{};
    gp.GX = (const double*)h->GX.p; gp.xs = h->gx_xs; gp.S = (const uint8_t*)h->S.p;
    gp.N = h->N; gp.B = h->B; gp.R = h->Rk; gp.P = 1 + h->Dstim + h->Kimp; gp.woff = 1 + h->Dstim;
    gp.spk = (const int2*)h->spk.p; gp.wlo = (const int*)h->wlo.p; gp.whi = (const int*)h->whi.p;
    gp.phi = (const double*)h->phi.p; gp.theta = (const double*)h->gtheta.p;
    gp.cols = a.cols; gp.pre = a.pre; gp.aw = a.aw; gp.w = a.w; gp.elo = a.elo; gp.ehi = a.ehi;
    gp.ncols = ncols; gp.K = nw; gp.nlin = h->nlin; gp.dt = h->dt;
    gp.t_lo = h->t_lo; gp.t_hi = h->t_hi;
    gp.CP = pl.CP; gp.rows = pl.rows; gp.gtb = pl.gtb;
    gp.nsplit = pl.nsplit; gp.nloop = pl.nloop; gp.hs_region = pl.hs_region; gp.fs_stride = pl.fs_stride;
    gp.nblkR = pl.nblk; gp.nygR = pl.ygroups; gp.nblkS = pl.sblk;
    gp.dbg = pl.dbg;
    return gp;
}

static void record_geometry(pgl_context* h, const PglGibbsPlan& pl)
{
    if (h->opt_record) pgl_gibbs_plan_report(&pl, h->gibbs_geo);
}

// regime-split path: the impulse responses of the pairs, the shared presynaptic features where every column has the same
// n_pre, then rate and spike workgroups in ONE launch, the spike workgroups (short chains of dependent loads: 87 us as a launch
// of their own) dispatched last: they fill the slots the rate workgroups free at the end.  (On a side stream beside the rate
// kernel -- two event hops -- they cost more than in line: 1.365 against 1.295 ms.)
static int launch_ll_cols_regime(pgl_handle h, const ColsArgs& a, int ncols, int K, int n_pre0, PglGibbsPlan& pl, double* ll_out)
{
    hipError_t e = ensure_dyn_lds(k_gibbs_rate_cols, pl.lds);
    if (e != hipSuccess) return fail(PGL_ERR_HIP, hipGetErrorString(e));
    pgl_gibbs_plan_loop(&pl, ncols, h->opt_dbg, (long long)gibbs_rate_wg_per_cu(pl.lds) * h->numCU);
    ENSURE(h->gpart, (size_t)(pl.nblk + pl.sblk) * ncols * PGL_KMAX * 8);
    ENSURE(h->ghs, (size_t)ncols * h->Rk * 8);
    if (pl.same_pre) ENSURE(h->gfs, (size_t)h->B * pl.fs_stride * 8);
    GibbsColsParams gp = cols_params(h, a, ncols, K, pl);
    gp.part = (double*)h->gpart.p;
    gp.partS = gp.part + (size_t)pl.nblk * ncols * PGL_KMAX;
    gp.hs = (double*)h->ghs.p;
    if (pl.same_pre) gp.fs = (const double*)h->gfs.p;
    record_geometry(h, pl);
    const long long nrows = h->t_hi - h->t_lo;
    record_gibbs(h, "k_gibbs_cols_setup");
    hipLaunchKernelGGL(k_gibbs_cols_setup, dim3((ncols * h->Rk + 255) / 256), dim3(256), 0, h->stream, gp);
    HIPCHK(hipGetLastError());
    if (pl.same_pre) {
        record_gibbs(h, "k_gibbs_pre_features");
        hipLaunchKernelGGL(k_gibbs_pre_features, dim3((unsigned)((nrows + 255) / 256)), dim3(256), (size_t)h->B * h->Rk * 8,
                           h->stream, gp, n_pre0, (double*)h->gfs.p);
        HIPCHK(hipGetLastError());
    }
    record_gibbs(h, "k_gibbs_rate_cols");
    hipLaunchKernelGGL(k_gibbs_rate_cols, dim3(pl.grid), dim3(256), pl.lds, h->stream, gp);
    HIPCHK(hipGetLastError());
    record_gibbs(h, "k_gibbs_reduce_cols2");
    hipLaunchKernelGGL(k_gibbs_reduce_cols2, dim3(ncols, K), dim3(64), 0, h->stream, (const double*)gp.part, pl.nblk,
                       (const double*)gp.partS, pl.sblk, ncols, K, h->dt, (double*)h->pin_args);
    HIPCHK(hipGetLastError());
    // the results land in the pinned host block directly (its argument bytes were consumed by the upload
    // that precedes the kernels on the stream): no device-to-host copy call
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memcpy(ll_out, h->pin_args, (size_t)ncols * K * 8);
    return PGL_OK;
}

// all-f64 path: one kernel over (time blocks, column groups), a reduction into gout, one copy into the pinned block
static int launch_ll_cols_f64(pgl_handle h, const ColsArgs& a, int ncols, int K, const PglGibbsPlan& pl, double* ll_out)
{
    ENSURE(h->gpart, (size_t)pl.nblk * ncols * PGL_KMAX * 8);
    ENSURE(h->gout, (size_t)ncols * K * 8);
    GibbsColsParams gp = cols_params(h, a, ncols, K, pl);
    gp.part = (double*)h->gpart.p;
    hipError_t e = ensure_dyn_lds(k_gibbs_ll_cols, pl.lds);
    if (e != hipSuccess) return fail(PGL_ERR_HIP, hipGetErrorString(e));
    record_geometry(h, pl);
    record_gibbs(h, "k_gibbs_ll_cols");
    hipLaunchKernelGGL(k_gibbs_ll_cols, dim3(pl.nblk, pl.ygroups), dim3(256), pl.lds, h->stream, gp);
    HIPCHK(hipGetLastError());
    record_gibbs(h, "k_gibbs_reduce_cols");
    hipLaunchKernelGGL(k_gibbs_reduce_cols, dim3(ncols), dim3(64), 0, h->stream, (const double*)h->gpart.p,
                       pl.nblk, ncols, K, (double*)h->gout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->pin_args, h->gout.p, (size_t)ncols * K * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memcpy(ll_out, h->pin_args, (size_t)ncols * K * 8);
    return PGL_OK;
}

// check, stage, plan (pglm_gibbs_plan.h), launch.  Staging comes before the plan because it finds the event ranges of the
// listed columns, whose largest the plan needs; which path runs (and so whether the ranges are wanted) is known before both.
int pgl_gibbs_ll_cols(pgl_handle h, int ncols, const int* n_post, const int* n_pre,
                      const double* aw_cur, const double* w, int K, double* ll_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (K <= 0 || K > PGL_KMAX || !ll_out) return fail(PGL_ERR_ARG, "K must be in 1..16");
    HIPCHK(hipSetDevice(h->device));
    rc = check_cols(h, ncols, n_post, n_pre, w);
    if (rc) return rc;
    const int explinear = h->nlin == PGL_NLIN_EXPLINEAR;
    const bool regime = pgl_gibbs_path(explinear, h->opt_gibbs, h->Rk) == PGL_GIBBS_REGIME;
    ColsArgs a;
    rc = stage_cols(h, ncols, n_post, n_pre, aw_cur, w, K, regime, (size_t)ncols * K * 8, a);
    if (rc) return rc;
    // every column with the same presynaptic neuron (a sweep step): its filtered spike train once per launch
    const bool pre_equal = std::all_of(n_pre, n_pre + ncols, [&](int j) { return j == n_pre[0]; });
    PglGibbsPlan pl;
    pgl_gibbs_plan_shape(&pl, ncols, K, pre_equal, h->t_hi - h->t_lo, a.max_ev, explinear, h->opt_gibbs, h->opt_dbg, h->B, h->Rk,
                         h->numCU);
    return regime ? launch_ll_cols_regime(h, a, ncols, K, n_pre[0], pl, ll_out) : launch_ll_cols_f64(h, a, ncols, K, pl, ll_out);
}

int pgl_gibbs_last_geometry(pgl_handle h, int* out, int n)
{
    if (!h || !out || n < 10) return fail(PGL_ERR_ARG, "bad argument");
    if (!h->opt_record) return fail(PGL_ERR_STATE, "kernel recording is off (PGL_OPT_RECORD_KERNELS)");
    if (h->gibbs_geo[0] < 0) return fail(PGL_ERR_STATE, "no pgl_gibbs_ll_cols call has been recorded");
    std::copy(h->gibbs_geo, h->gibbs_geo + 10, out);
    return PGL_OK;
}

int pgl_gibbs_update_cols(pgl_handle h, int ncols, const int* n_post, const int* n_pre, const double* delta)
{
    int rc = check_ready(h);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    for (int a = 0; a < ncols; ++a)                       // two deltas for one post neuron would race
        for (int b = a + 1; b < ncols; ++b)
            if (n_post && n_post[a] == n_post[b]) return fail(PGL_ERR_ARG, "duplicate post-synaptic column");
    rc = check_cols(h, ncols, n_post, n_pre, delta);
    if (rc) return rc;
    ColsArgs a;
    rc = stage_cols(h, ncols, n_post, n_pre, nullptr, delta, 1, false, 0, a);
    if (rc) return rc;
    PglGibbsPlan pl;
    pgl_gibbs_plan_update(&pl, ncols, h->t_hi - h->t_lo, h->B, h->Rk);
    const GibbsColsParams gp = cols_params(h, a, ncols, 1, pl);
    record_gibbs(h, "k_gibbs_update_cols");
    hipLaunchKernelGGL(k_gibbs_update_cols, dim3(pl.nblk, pl.ygroups), dim3(256), pl.lds, h->stream, gp, (double*)h->GX.p);
    HIPCHK(hipGetLastError());
    // the column arguments were staged in the handle's pinned block: the next call refills it, so the
    // asynchronous upload must have happened before this one returns
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

int pgl_gibbs_currents(pgl_handle h, int n_post, double* x_out)
{
    if (!h || !x_out) return fail(PGL_ERR_ARG, "null argument");
    if (h->gx_xs == 0) return fail(PGL_ERR_STATE, "pgl_gibbs_prepare_all has not been called");
    if (n_post < 0 || n_post >= h->N) return fail(PGL_ERR_ARG, "n_post out of range");
    HIPCHK(hipSetDevice(h->device));
    const long long nrows = h->gx_t_hi - h->gx_t_lo;
    HIPCHK(hipMemcpy2DAsync(x_out, 8, (const double*)h->GX.p + h->gx_t_lo * h->gx_xs + n_post,
                            (size_t)h->gx_xs * 8, 8, (size_t)nrows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

int pgl_ll_from_current(pgl_handle h, int n_post, double I_bias, const double* I_stim,
                        const double* I_other, const double* I_col, const double* w, int K,
                        double* ll_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!h->have_spikes) return fail(PGL_ERR_STATE, "pgl_set_spikes_* has not been called");
    if (!I_other || !I_col || !w || !ll_out || K <= 0) return fail(PGL_ERR_ARG, "bad argument");
    if (n_post < 0 || n_post >= h->N) return fail(PGL_ERR_ARG, "n_post out of range");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->nT * 8;
    ENSURE(h->tmpA, bytes);
    ENSURE(h->tmpB, bytes);
    HIPCHK(hipMemcpyAsync(h->tmpA.p, I_other, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->tmpB.p, I_col, bytes, hipMemcpyHostToDevice, h->stream));
    const double* d_stim = nullptr;
    if (I_stim) {
        ENSURE(h->tmpC, bytes);
        HIPCHK(hipMemcpyAsync(h->tmpC.p, I_stim, bytes, hipMemcpyHostToDevice, h->stream));
        d_stim = (const double*)h->tmpC.p;
    }
    return run_ll_current(h, (const double*)h->tmpA.p, d_stim, (const double*)h->tmpB.p, n_post,
                          I_bias, 0.0, w, K, ll_out);
}

namespace {
struct UniformStream {
    const double* buf;
    int64_t n, pos;
    uint64_t state;
    double next()
    {
        if (buf && pos < n) return buf[pos++];
        uint64_t z = (state += 0x9e3779b97f4a7c15ULL);        // splitmix64
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        z ^= z >> 31;
        return ((z >> 11) + 0.5) * (1.0 / 9007199254740992.0); // (0,1)
    }
};
inline double host_nlin(double x, int nlin)
{
    return nlin == 1 ? std::fmax(x, 0.0) + std::log1p(std::exp(-std::fabs(x))) : std::exp(x);
}
}  // namespace

int pgl_simulate(int N, int64_t nT, int R, int nlin, double dt, double* X, const double* AW,
                 const double* uniforms, int64_t n_uniforms, uint64_t seed, double* S,
                 int64_t* n_exceptions_out)
{
    if (N <= 0 || nT <= 0 || R <= 0 || !X || !AW || !S) return fail(PGL_ERR_ARG, "bad argument");
    if (nlin != PGL_NLIN_EXP && nlin != PGL_NLIN_EXPLINEAR) return fail(PGL_ERR_ARG, "unknown nonlinearity");
    UniformStream u{uniforms, uniforms ? n_uniforms : 0, 0, seed};
    std::vector<double> acc(N, 0.0), thr(N);
    std::vector<char> spk(N);
    for (int n = 0; n < N; ++n) thr[n] = -std::log(u.next());             // population.py:293
    std::memset(S, 0, sizeof(double) * (size_t)nT * N);
    int64_t n_exc = 0;
    for (int64_t t = 0; t < nT; ++t) {
        double* Xt = X + (size_t)t * N;
        double* St = S + (size_t)t * N;
        int n_spk = 0;
        for (int n = 0; n < N; ++n) {
            acc[n] += host_nlin(Xt[n], nlin) * dt;                       // population.py:317-318
            spk[n] = acc[n] > thr[n];
            if (spk[n]) { St[n] += 1.0; ++n_spk; }
        }
        const int64_t t_imp = std::min<int64_t>(nT - t - 1, R);          // population.py:326
        while (n_spk > 0) {
            bool capped = false;
            for (int n = 0; n < N; ++n) capped = capped || (St[n] >= 10.0);
            if (capped) { ++n_exc; break; }                              // population.py:345-349
            for (int np = 0; np < N; ++np) {
                if (!spk[np]) continue;
                const double* aw = AW + (size_t)np * R * N;
                for (int64_t tau = 0; tau < t_imp; ++tau) {              // population.py:351-353
                    double* xr = X + (size_t)(t + 1 + tau) * N;
                    const double* ar = aw + (size_t)tau * N;
                    for (int n = 0; n < N; ++n) xr[n] += ar[n];
                }
            }
            for (int n = 0; n < N; ++n) {                                // population.py:355-360
                if (spk[n]) acc[n] -= thr[n];
                if (acc[n] < 0) acc[n] = 0;
            }
            for (int n = 0; n < N; ++n)
                if (spk[n]) thr[n] = -std::log(u.next());
            n_spk = 0;
            for (int n = 0; n < N; ++n) {
                spk[n] = acc[n] > thr[n];
                if (spk[n]) { St[n] += 1.0; ++n_spk; }
            }
        }
    }
    if (n_exceptions_out) *n_exceptions_out = n_exc;
    return PGL_OK;
}

// ---- batched simulation on per-neuron threshold streams (pglm_simulate.hip.h; the stream rule: include/pyglm_hip.h) ----
// Host reference of one replicate: pgl_simulate's loop, the thresholds from the stateless streams.
int pgl_simulate_streams(int N, int64_t nT, int R, int nlin, double dt, double* X, const double* AW, int rep,
                         uint64_t seed, uint8_t* S, int64_t* n_exceptions_out, double* closest_call_out)
{
    if (N <= 0 || nT <= 0 || R <= 0 || rep < 0 || !X || !AW || !S) return fail(PGL_ERR_ARG, "bad argument");
    if (nlin != PGL_NLIN_EXP && nlin != PGL_NLIN_EXPLINEAR) return fail(PGL_ERR_ARG, "unknown nonlinearity");
    std::vector<double> acc(N, 0.0), thr(N);
    std::vector<unsigned long long> key(N), k(N, 1);
    std::vector<char> spk(N);
    for (int n = 0; n < N; ++n) {
        key[n] = pgl_sim_key(seed, (unsigned long long)rep, (unsigned long long)n);
        thr[n] = -std::log(pgl_sim_uniform(key[n], 0));
    }
    std::memset(S, 0, (size_t)nT * N);
    int64_t n_exc = 0;
    double closest = __builtin_huge_val();
    const auto compare = [&](int n) {                                    // acc > thr, and how close the call was
        const double m = std::fabs(acc[n] - thr[n]) / thr[n];
        if (m < closest) closest = m;
        return acc[n] > thr[n];
    };
    for (int64_t t = 0; t < nT; ++t) {
        double* Xt = X + (size_t)t * N;
        uint8_t* St = S + (size_t)t * N;
        int n_spk = 0;
        for (int n = 0; n < N; ++n) {
            acc[n] += host_nlin(Xt[n], nlin) * dt;
            spk[n] = compare(n);
            if (spk[n]) { St[n] += 1; ++n_spk; }
        }
        const int64_t t_imp = std::min<int64_t>(nT - t - 1, R);
        while (n_spk > 0) {
            bool capped = false;
            for (int n = 0; n < N; ++n) capped = capped || (St[n] >= 10);
            if (capped) { ++n_exc; break; }
            for (int np = 0; np < N; ++np) {
                if (!spk[np]) continue;
                const double* aw = AW + (size_t)np * R * N;
                for (int64_t i = 0; i < t_imp * N; ++i) Xt[N + i] += aw[i];
            }
            for (int n = 0; n < N; ++n) {
                if (spk[n]) {
                    acc[n] -= thr[n];
                    thr[n] = -std::log(pgl_sim_uniform(key[n], k[n]++));
                }
                if (acc[n] < 0) acc[n] = 0;
            }
            n_spk = 0;
            for (int n = 0; n < N; ++n) {
                spk[n] = compare(n);
                if (spk[n]) { St[n] += 1; ++n_spk; }
            }
        }
    }
    if (n_exceptions_out) *n_exceptions_out = n_exc;
    if (closest_call_out) *closest_call_out = closest;
    return PGL_OK;
}

static int sim_check(int N, int64_t nT, int R, int nlin, double dt, int n_rep, int rep0)
{
    if (N <= 0 || nT <= 0 || R <= 0 || n_rep <= 0 || rep0 < 0 || !(dt > 0)) return fail(PGL_ERR_ARG, "bad argument");
    if (N > PGL_SIM_MAXN) return fail(PGL_ERR_ARG, "N > 1024 neurons");
    if ((long long)R * N > (1 << 27)) return fail(PGL_ERR_ARG, "R * N too large");
    if (nlin != PGL_NLIN_EXP && nlin != PGL_NLIN_EXPLINEAR) return fail(PGL_ERR_ARG, "unknown nonlinearity");
    return PGL_OK;
}

int pgl_simulate_batch_plan(int N, int R, int flags, int* ring_in_lds, long long* workspace_bytes_per_rep)
{
    if (N <= 0 || N > PGL_SIM_MAXN || R <= 0 || (long long)R * N > (1 << 27)) return fail(PGL_ERR_ARG, "bad argument");
    const long long bytes = (long long)R * N * 8;
    const bool lds = !(flags & 1) && bytes <= PGL_SIM_LDS_MAX;
    if (ring_in_lds) *ring_in_lds = lds ? 1 : 0;
    if (workspace_bytes_per_rep) *workspace_bytes_per_rep = lds ? 0 : bytes;
    return PGL_OK;
}

static int sim_device(int device)
{
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(PGL_ERR_HIP, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(PGL_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    return PGL_OK;
}

int pgl_simulate_batch_dev(int device, int N, int64_t nT, int R, int nlin, double dt, const double* d_X0,
                           const double* d_AW, int n_rep, int rep0, uint64_t seed, int flags, uint8_t* d_S, double* d_X,
                           int64_t* d_counts, int64_t* d_exceptions, double* d_workspace, void* stream)
{
    int rc = sim_check(N, nT, R, nlin, dt, n_rep, rep0);
    if (rc) return rc;
    if (!d_X0 || !d_AW || !d_counts || !d_exceptions) return fail(PGL_ERR_ARG, "null argument");
    int lds = 0;
    long long ws = 0;
    pgl_simulate_batch_plan(N, R, flags, &lds, &ws);
    if (!lds && !d_workspace) return fail(PGL_ERR_ARG, "the ring of this shape lives in global memory: d_workspace is NULL");
    rc = sim_device(device);
    if (rc) return rc;
    SimParams sp;
    sp.X0 = d_X0; sp.AW = d_AW; sp.ws = d_workspace; sp.S = d_S; sp.X = d_X;
    sp.counts = (long long*)d_counts; sp.exc = (long long*)d_exceptions;
    sp.nT = nT; sp.N = N; sp.R = R; sp.rep0 = rep0; sp.seed = seed; sp.dt = dt;
    // threads: one per neuron at least; the scatter of a spike (R N additions) is shared by all of them
    const int threads = (N <= 256 && (long long)R * N <= 16384) ? 256 : PGL_SIM_MAXN;
    const size_t ring = (size_t)R * N * 8;
    hipStream_t s = (hipStream_t)stream;
    if (nlin == PGL_NLIN_EXPLINEAR)
        return lds ? sim_launch<1, true>(sp, n_rep, threads, ring, s) : sim_launch<1, false>(sp, n_rep, threads, 0, s);
    return lds ? sim_launch<0, true>(sp, n_rep, threads, ring, s) : sim_launch<0, false>(sp, n_rep, threads, 0, s);
}

int pgl_simulate_batch(int device, int N, int64_t nT, int R, int nlin, double dt, const double* X0, const double* AW,
                       int n_rep, int rep0, uint64_t seed, int flags, uint8_t* S_out, double* X_out,
                       int64_t* counts_out, int64_t* exceptions_out)
{
    int rc = sim_check(N, nT, R, nlin, dt, n_rep, rep0);
    if (rc) return rc;
    if (!X0 || !AW || !counts_out || !exceptions_out) return fail(PGL_ERR_ARG, "null argument");
    rc = sim_device(device);
    if (rc) return rc;
    int lds = 0;
    long long ws = 0;
    pgl_simulate_batch_plan(N, R, flags, &lds, &ws);
    const size_t nx = (size_t)nT * N, naw = (size_t)N * R * N, nout = (size_t)n_rep * nx;
    DevBuf dX0, dAW, dS, dX, dC, dE, dW;
    const auto done = [&](int r) {
        release(dX0); release(dAW); release(dS); release(dX); release(dC); release(dE); release(dW);
        return r;
    };
    if (ensure(dX0, nx * 8) || ensure(dAW, naw * 8) || ensure(dC, (size_t)n_rep * N * 8) || ensure(dE, (size_t)n_rep * 8) ||
        (S_out && ensure(dS, nout)) || (X_out && ensure(dX, nout * 8)) || (!lds && ensure(dW, (size_t)n_rep * ws)))
        return done(PGL_ERR_HIP);
    if (hipMemcpy(dX0.p, X0, nx * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dAW.p, AW, naw * 8, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(PGL_ERR_HIP, "simulate_batch: upload failed"));
    rc = pgl_simulate_batch_dev(device, N, nT, R, nlin, dt, (const double*)dX0.p, (const double*)dAW.p, n_rep, rep0, seed,
                                flags, (uint8_t*)dS.p, (double*)dX.p, (int64_t*)dC.p, (int64_t*)dE.p, (double*)dW.p, nullptr);
    if (rc) return done(rc);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return done(fail(PGL_ERR_HIP, std::string("simulate_batch: ") + hipGetErrorString(e)));
    if (hipMemcpy(counts_out, dC.p, (size_t)n_rep * N * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(exceptions_out, dE.p, (size_t)n_rep * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        (S_out && hipMemcpy(S_out, dS.p, nout, hipMemcpyDeviceToHost) != hipSuccess) ||
        (X_out && hipMemcpy(X_out, dX.p, nout * 8, hipMemcpyDeviceToHost) != hipSuccess))
        return done(fail(PGL_ERR_HIP, "simulate_batch: download failed"));
    return done(PGL_OK);
}

// ---- clamped simulation: every neuron given the others' recorded spikes (pglm_condsim.h, pglm_condsim.hip.h) ----
static int cond_sim_check(int N, int64_t nT, int R, int nlin, double dt, int64_t win, int n_rep, int rep0);

// Host reference of one replicate: the chain rule of the header, neuron by neuron.
int pgl_simulate_cond_streams(int N, int64_t nT, int R, int nlin, double dt, const double* Xc, const double* AW, int rep,
                              uint64_t seed, uint8_t* S, int64_t* exceptions_out, double* closest_call_out)
{
    // (the shapes the device entries serve, so that every call they accept has its reference and no other)
    int rc = cond_sim_check(N, nT, R, nlin, dt, 1, 1, rep);
    if (rc) return rc;
    if (!Xc || !AW || !S) return fail(PGL_ERR_ARG, "null argument");
    std::vector<double> x((size_t)nT), h((size_t)R);
    double closest = __builtin_huge_val();
    for (int n = 0; n < N; ++n) {
        for (int64_t t = 0; t < nT; ++t) x[t] = Xc[(size_t)t * N + n];
        for (int tau = 0; tau < R; ++tau) h[tau] = AW[((size_t)n * R + tau) * N + n];
        const long long e = pgl_cs_chain(nT, R, nlin, dt, x.data(), h.data(), seed, (pgl_cs_u64)rep, (pgl_cs_u64)n, S + n, N,
                                         &closest);
        if (exceptions_out) exceptions_out[n] = e;
    }
    if (closest_call_out) *closest_call_out = closest;
    return PGL_OK;
}

static int cond_check(int N, int64_t nT, int R)
{
    if (N <= 0 || nT <= 0 || R <= 0) return fail(PGL_ERR_ARG, "bad argument");
    if (N > PGL_SIM_MAXN) return fail(PGL_ERR_ARG, "N > 1024 neurons");
    if ((long long)R * N > (1 << 27)) return fail(PGL_ERR_ARG, "R * N too large");
    return PGL_OK;
}

int pgl_cond_currents_dev(int device, int N, int64_t nT, int R, const double* d_X0, const double* d_AW, const int32_t* d_ev_pre,
                          const uint8_t* d_ev_cnt, const int64_t* d_bin_off, double* d_Xc, void* stream)
{
    int rc = cond_check(N, nT, R);
    if (rc) return rc;
    if (!d_X0 || !d_AW || !d_bin_off || !d_Xc) return fail(PGL_ERR_ARG, "null argument");
    rc = sim_device(device);
    if (rc) return rc;
    const long long n = (long long)nT * N;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(k_cond_currents, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_X0, d_AW, (const int*)d_ev_pre,
                       (const unsigned char*)d_ev_cnt, (const long long*)d_bin_off, d_Xc, (long long)nT, N, R);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// bin_off of a host caller: ascending from 0, every event of a neuron 0 .. N - 1 with a count >= 1, sorted by (bin, pre)
static int cond_events_check(int N, int64_t nT, const int32_t* ev_pre, const uint8_t* ev_cnt, const int64_t* bin_off)
{
    if (!bin_off || bin_off[0] != 0) return fail(PGL_ERR_ARG, "bin_off must start at 0");
    for (int64_t t = 0; t < nT; ++t) {
        if (bin_off[t + 1] < bin_off[t]) return fail(PGL_ERR_ARG, "bin_off must ascend");
        for (int64_t e = bin_off[t]; e < bin_off[t + 1]; ++e) {
            if (!ev_pre || !ev_cnt || ev_pre[e] < 0 || ev_pre[e] >= N || ev_cnt[e] == 0 || (e > bin_off[t] && ev_pre[e] <= ev_pre[e - 1]))
                return fail(PGL_ERR_ARG, "events must be sorted by (bin, pre) with pre in 0 .. N - 1 and counts >= 1");
        }
    }
    return PGL_OK;
}

int pgl_cond_currents(int device, int N, int64_t nT, int R, const double* X0, const double* AW, const int32_t* ev_pre,
                      const uint8_t* ev_cnt, const int64_t* bin_off, double* Xc_out)
{
    int rc = cond_check(N, nT, R);
    if (rc) return rc;
    if (!X0 || !AW || !bin_off || !Xc_out) return fail(PGL_ERR_ARG, "null argument");
    rc = cond_events_check(N, nT, ev_pre, ev_cnt, bin_off);
    if (rc) return rc;
    rc = sim_device(device);
    if (rc) return rc;
    const size_t nx = (size_t)nT * N, naw = (size_t)N * R * N, E = (size_t)bin_off[nT];
    DevBuf dX0, dAW, dP, dC, dO, dXc;
    const auto done = [&](int r) {
        release(dX0); release(dAW); release(dP); release(dC); release(dO); release(dXc);
        return r;
    };
    if (ensure(dX0, nx * 8) || ensure(dAW, naw * 8) || ensure(dP, (E + 1) * 4) || ensure(dC, E + 1) ||
        ensure(dO, (size_t)(nT + 1) * 8) || ensure(dXc, nx * 8))
        return done(PGL_ERR_HIP);
    if (hipMemcpy(dX0.p, X0, nx * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dAW.p, AW, naw * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (E && hipMemcpy(dP.p, ev_pre, E * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        (E && hipMemcpy(dC.p, ev_cnt, E, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(dO.p, bin_off, (size_t)(nT + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(PGL_ERR_HIP, "cond_currents: upload failed"));
    rc = pgl_cond_currents_dev(device, N, nT, R, (const double*)dX0.p, (const double*)dAW.p, (const int32_t*)dP.p,
                               (const uint8_t*)dC.p, (const int64_t*)dO.p, (double*)dXc.p, nullptr);
    if (rc) return done(rc);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return done(fail(PGL_ERR_HIP, std::string("cond_currents: ") + hipGetErrorString(e)));
    if (hipMemcpy(Xc_out, dXc.p, nx * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(PGL_ERR_HIP, "cond_currents: download failed"));
    return done(PGL_OK);
}

static int cond_sim_check(int N, int64_t nT, int R, int nlin, double dt, int64_t win, int n_rep, int rep0)
{
    int rc = sim_check(N, nT, R, nlin, dt, n_rep, rep0);
    if (rc) return rc;
    if (win <= 0) return fail(PGL_ERR_ARG, "win must be at least 1");
    if ((long long)rep0 + n_rep > 0x7fffffffLL) return fail(PGL_ERR_ARG, "rep0 + n_rep too large");
    // (one workgroup per (neuron, 64 replicates): the grid must fit its 32-bit dimension)
    if ((long long)N * (((long long)n_rep + 63) / 64) > 0x7fffffffLL) return fail(PGL_ERR_ARG, "N * ceil(n_rep / 64) workgroups exceed 2^31 - 1");
    if (R > PGL_CS_MAX_R) return fail(PGL_ERR_UNSUPPORTED, "R > 4096 taps of self-history");
    return PGL_OK;
}

long long pgl_simulate_cond_workspace(int N, int R, int n_rep)
{
    if (N <= 0 || R <= 0 || n_rep <= 0) return 0;
    return (long long)N * R * n_rep * 8;
}

int pgl_simulate_cond_dev(int device, int N, int64_t nT, int R, int nlin, double dt, const double* d_Xc, const double* d_AW,
                          const int64_t* d_obs, int64_t win, int n_rep, int rep0, uint64_t seed, int flags, int accumulate,
                          int64_t* d_acc, int64_t* d_exceptions, int64_t* d_counts, uint8_t* d_S, int64_t* d_fallbacks,
                          double* d_workspace, void* stream)
{
    int rc = cond_sim_check(N, nT, R, nlin, dt, win, n_rep, rep0);
    if (rc) return rc;
    if (!d_Xc || !d_AW || !d_obs || !d_acc || !d_exceptions || !d_workspace) return fail(PGL_ERR_ARG, "null argument");
    rc = sim_device(device);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    CondSimParams cp;
    cp.Xc = d_Xc; cp.AW = d_AW; cp.obs = (const long long*)d_obs; cp.ring = d_workspace; cp.acc = (long long*)d_acc;
    cp.exc = (long long*)d_exceptions; cp.counts = (long long*)d_counts; cp.S = d_S; cp.fallbacks = (long long*)d_fallbacks;
    cp.nT = nT; cp.win = win; cp.n_win = pgl_cs_windows(nT, win); cp.N = N; cp.R = R; cp.n_rep = n_rep; cp.rep0 = rep0;
    cp.flags = flags; cp.seed = seed; cp.dt = dt;
    if (!accumulate) {
        const long long plane = cp.n_win * N;
        hipLaunchKernelGGL(k_cond_acc_init, dim3((unsigned)((std::max<long long>(plane, N) + 255) / 256)), dim3(256), 0, s,
                           cp.acc, cp.exc, cp.fallbacks, plane, N);
        HIPCHK(hipGetLastError());
    }
    const unsigned blocks = (unsigned)N * (unsigned)((n_rep + 63) / 64);
    if (nlin == PGL_NLIN_EXPLINEAR)
        hipLaunchKernelGGL(k_simulate_cond<1>, dim3(blocks), dim3(64), (size_t)R * 8, s, cp);
    else
        hipLaunchKernelGGL(k_simulate_cond<0>, dim3(blocks), dim3(64), (size_t)R * 8, s, cp);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_simulate_cond(int device, int N, int64_t nT, int R, int nlin, double dt, const double* Xc, const double* AW,
                      const int64_t* obs, int64_t win, int n_rep, int rep0, uint64_t seed, int flags, int accumulate,
                      int64_t* acc, int64_t* exceptions, int64_t* counts_out, uint8_t* S_out, int64_t* fallbacks)
{
    int rc = cond_sim_check(N, nT, R, nlin, dt, win, n_rep, rep0);
    if (rc) return rc;
    if (!Xc || !AW || !obs || !acc || !exceptions) return fail(PGL_ERR_ARG, "null argument");
    rc = sim_device(device);
    if (rc) return rc;
    const size_t nx = (size_t)nT * N, naw = (size_t)N * R * N, nw = (size_t)pgl_cs_windows(nT, win) * N, nout = (size_t)n_rep * nx;
    DevBuf dXc, dAW, dO, dA, dE, dC, dS, dF, dW;
    const auto done = [&](int r) {
        release(dXc); release(dAW); release(dO); release(dA); release(dE); release(dC); release(dS); release(dF); release(dW);
        return r;
    };
    if (ensure(dXc, nx * 8) || ensure(dAW, naw * 8) || ensure(dO, nw * 8) || ensure(dA, PGL_CS_NACC * nw * 8) ||
        ensure(dE, (size_t)N * 8) || ensure(dF, 8) || ensure(dW, (size_t)pgl_simulate_cond_workspace(N, R, n_rep)) ||
        (counts_out && ensure(dC, (size_t)n_rep * N * 8)) || (S_out && ensure(dS, nout)))
        return done(PGL_ERR_HIP);
    if (hipMemcpy(dXc.p, Xc, nx * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dAW.p, AW, naw * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dO.p, obs, nw * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (accumulate && (hipMemcpy(dA.p, acc, PGL_CS_NACC * nw * 8, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(dE.p, exceptions, (size_t)N * 8, hipMemcpyHostToDevice) != hipSuccess ||
                        (fallbacks && hipMemcpy(dF.p, fallbacks, 8, hipMemcpyHostToDevice) != hipSuccess))))
        return done(fail(PGL_ERR_HIP, "simulate_cond: upload failed"));
    rc = pgl_simulate_cond_dev(device, N, nT, R, nlin, dt, (const double*)dXc.p, (const double*)dAW.p, (const int64_t*)dO.p, win,
                               n_rep, rep0, seed, flags, accumulate, (int64_t*)dA.p, (int64_t*)dE.p, (int64_t*)dC.p,
                               (uint8_t*)dS.p, fallbacks ? (int64_t*)dF.p : nullptr, (double*)dW.p, nullptr);
    if (rc) return done(rc);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return done(fail(PGL_ERR_HIP, std::string("simulate_cond: ") + hipGetErrorString(e)));
    if (hipMemcpy(acc, dA.p, PGL_CS_NACC * nw * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(exceptions, dE.p, (size_t)N * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        (fallbacks && hipMemcpy(fallbacks, dF.p, 8, hipMemcpyDeviceToHost) != hipSuccess) ||
        (counts_out && hipMemcpy(counts_out, dC.p, (size_t)n_rep * N * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
        (S_out && hipMemcpy(S_out, dS.p, nout, hipMemcpyDeviceToHost) != hipSuccess))
        return done(fail(PGL_ERR_HIP, "simulate_cond: download failed"));
    return done(PGL_OK);
}

// Leading singular pairs of a batch of (L x D) matrices (k_lsp_*, pglm_stim.hip.h).  Host arrays; everything in between on
// the device with the library's own kernels.
int pgl_leading_singular_pairs(pgl_handle h, const double* A, int n, int L, int D, double* U, double* sigma, double* V)
{
    if (!h || !U || !sigma || !V || n <= 0 || L <= 0 || D <= 0) return fail(PGL_ERR_ARG, "bad argument");
    if (!A && (!h->staA.p || h->sta_n != n || h->sta_L != L || h->sta_D != D))
        return fail(PGL_ERR_STATE, "A == NULL: no spike-triggered averages of this shape on the device (pgl_sta with A_out == NULL)");
    HIPCHK(hipSetDevice(h->device));
    const bool wide = L <= D;                              // Gram matrix of the smaller side
    const int m = wide ? L : D, big = wide ? D : L;
    const size_t na = (size_t)n * L * D, ng = (size_t)n * m * m;
    DevBuf dA, dG0, dG1, dx, dy, dn;
    auto done = [&](int rc) {
        release(dA); release(dG0); release(dG1); release(dx); release(dy); release(dn);
        return rc;
    };
    if (A) {
        if (ensure(dA, na * 8)) return done(PGL_ERR_HIP);
        if (hipMemcpyAsync(dA.p, A, na * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) return done(fail(PGL_ERR_HIP, "upload"));
    } else {                                               // the averages pgl_sta left on the device; consumed by this call
        dA = h->staA;
        h->staA = DevBuf();
        h->sta_n = h->sta_L = h->sta_D = 0;
    }
    if (ensure(dG0, ng * 8) || ensure(dG1, ng * 8) || ensure(dx, (size_t)n * m * 8) ||
        ensure(dy, (size_t)n * big * 8) || ensure(dn, (size_t)n * 8))
        return done(PGL_ERR_HIP);
    const double* a = (const double*)dA.p;
    const long long sa = (long long)L * D, sg = (long long)m * m;
    int launch_rc = PGL_OK;
    auto gemm = [&](const double* Am, long long sam, long long sak, long long sAb, const double* Bm, long long sbn, long long sbk,
                    long long sBb, double* C, long long scm, long long scn, long long sCb, int M, int N, int K) {
        if (N >= 64) launch_rc |= launch_gemm_mfma_nt<4>(h, Am, sam, sak, sAb, Bm, sbn, sbk, sBb, C, scm, scn, sCb, M, N, K, n);
        else launch_rc |= launch_gemm_mfma_nt<1>(h, Am, sam, sak, sAb, Bm, sbn, sbk, sBb, C, scm, scn, sCb, M, N, K, n);
    };
    // G = A A^T (wide) or A^T A (tall); element (i, j) of the small side
    if (wide) gemm(a, D, 1, sa, a, D, 1, sa, (double*)dG0.p, m, 1, sg, m, m, D);
    else gemm(a, 1, D, sa, a, 1, D, sa, (double*)dG0.p, m, 1, sg, m, m, L);
    double* g0 = (double*)dG0.p;
    double* g1 = (double*)dG1.p;
    hipLaunchKernelGGL(k_lsp_trace_scale, dim3(n), dim3(1024), 0, h->stream, g0, m, sg);
    for (int s = 0; s < 16; ++s) {                         // G <- G^2 / trace(G^2)  (G symmetric: G G^T): G^(2^16) in the end
        gemm(g0, m, 1, sg, g0, m, 1, sg, g1, m, 1, sg, m, m, m);
        hipLaunchKernelGGL(k_lsp_trace_scale, dim3(n), dim3(1024), 0, h->stream, g1, m, sg);
        std::swap(g0, g1);
    }
    double* x = (double*)dx.p;                             // (n, m): on the small side
    double* y = (double*)dy.p;                             // (n, big)
    hipLaunchKernelGGL(k_lsp_pick, dim3(n), dim3(1024), 0, h->stream, (const double*)g0, m, sg, x);
    // y = A^T x (wide: D-vector) or A x (tall: L-vector); x back from y
    auto to_big = [&]() {
        if (wide) gemm(a, 1, D, sa, x, 0, 1, m, y, 1, 0, big, D, 1, L);       // y[d] = sum_l A[l][d] x[l]
        else gemm(a, D, 1, sa, x, 0, 1, m, y, 1, 0, big, L, 1, D);            // y[l] = sum_d A[l][d] x[d]
    };
    auto to_small = [&]() {
        if (wide) gemm(a, D, 1, sa, y, 0, 1, big, x, 1, 0, m, L, 1, D);       // x[l] = sum_d A[l][d] y[d]
        else gemm(a, 1, D, sa, y, 0, 1, big, x, 1, 0, m, D, 1, L);            // x[d] = sum_l A[l][d] y[l]
    };
    for (int it = 0; it < 2; ++it) {
        to_big();
        hipLaunchKernelGGL(k_lsp_normalize, dim3(n), dim3(1024), 0, h->stream, y, big, (double*)nullptr);
        to_small();
        hipLaunchKernelGGL(k_lsp_normalize, dim3(n), dim3(1024), 0, h->stream, x, m, (double*)nullptr);
    }
    to_big();                                              // |A^T x| (wide) or |A x| (tall) = sigma_0
    hipLaunchKernelGGL(k_lsp_normalize, dim3(n), dim3(1024), 0, h->stream, y, big, (double*)dn.p);
    if (launch_rc || hipGetLastError() != hipSuccess) return done(fail(PGL_ERR_HIP, "leading singular pairs: launch failed"));
    double* Uo = wide ? x : y;
    double* Vo = wide ? y : x;
    bool ok = hipMemcpyAsync(U, Uo, (size_t)n * L * 8, hipMemcpyDeviceToHost, h->stream) == hipSuccess &&
              hipMemcpyAsync(V, Vo, (size_t)n * D * 8, hipMemcpyDeviceToHost, h->stream) == hipSuccess &&
              hipMemcpyAsync(sigma, dn.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream) == hipSuccess &&
              hipStreamSynchronize(h->stream) == hipSuccess;
    if (!ok) return done(fail(PGL_ERR_HIP, "leading singular pairs: copy failed"));
    // sign convention: the component of u_0 of largest magnitude is positive (the pair's sign is LAPACK's business in the
    // reference; the rank-1 filter u_0 v_0^T does not depend on it)
    for (int b = 0; b < n; ++b) {
        double* u = U + (size_t)b * L;
        double* v = V + (size_t)b * D;
        int j = 0;
        for (int i = 1; i < L; ++i)
            if (std::fabs(u[i]) > std::fabs(u[j])) j = i;
        if (u[j] < 0.0) {
            for (int i = 0; i < L; ++i) u[i] = -u[i];
            for (int i = 0; i < D; ++i) v[i] = -v[i];
        }
    }
    return done(PGL_OK);
}

// One thin GEMM on device operands through the launchers production uses (tests observe each instantiation on its own).
int pgl_gemm_dev(pgl_handle h, int kernel, const double* d_A, int64_t sam, int64_t sak, int64_t sAb, const double* d_B,
                 int64_t sbn, int64_t sbk, int64_t sBb, double* d_C, int64_t scm, int64_t scn, int64_t sCb, int M, int N, int K,
                 int batch)
{
    if (!h || !d_A || !d_B || !d_C) return fail(PGL_ERR_ARG, "pgl_gemm_dev: null argument");
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || batch > 65535) return fail(PGL_ERR_ARG, "pgl_gemm_dev: bad shape");
    if (sam < 0 || sak < 0 || sbn < 0 || sbk < 0 || scm < 0 || scn < 0 || sAb < 0 || sBb < 0 || sCb < 0)
        return fail(PGL_ERR_ARG, "pgl_gemm_dev: negative stride");
    const bool kc = kernel == PGL_GEMM_KC_4_1_8 || kernel == PGL_GEMM_KC_1_0_16;
    if ((kc || kernel == PGL_GEMM_NT) && batch != 1) return fail(PGL_ERR_ARG, "pgl_gemm_dev: this kernel takes no batch");
    HIPCHK(hipSetDevice(h->device));
    switch (kernel) {
    case PGL_GEMM_NT:
        if (sak != 1 || sbk != 1 || scn != 1) return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_nt needs unit k and n strides");
        if (sam > 0x7fffffffLL || sbn > 0x7fffffffLL || scm > 0x7fffffffLL)
            return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_nt takes int leading dimensions");
        return launch_gemm_nt(h, d_A, (int)sam, d_B, (int)sbn, d_C, (int)scm, M, N, K);
    case PGL_GEMM_MFMA_1:
        return launch_gemm_mfma_nt<1>(h, d_A, sam, sak, sAb, d_B, sbn, sbk, sBb, d_C, scm, scn, sCb, M, N, K, batch);
    case PGL_GEMM_MFMA_4:
        return launch_gemm_mfma_nt<4>(h, d_A, sam, sak, sAb, d_B, sbn, sbk, sBb, d_C, scm, scn, sCb, M, N, K, batch);
    case PGL_GEMM_KC_4_1_8:                               // both operands k-contiguous, 16-byte loads
        if ((K & 1) || sak != 1 || sbk != 1) return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_kc needs K even and unit k strides");
        if (!gemm_aligned(d_A, sam) || !gemm_aligned(d_B, sbn))
            return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_kc needs 16-byte aligned operands with even leading dimensions");
        return launch_gemm_kc<4, 1, 8>(h, d_A, sam, d_B, sbn, d_C, scm, scn, M, N, K);
    case PGL_GEMM_KC_1_0_16:                              // A k-contiguous (16-byte loads), B n-contiguous (8-byte loads)
        if ((K & 1) || sak != 1 || sbn != 1) return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_kc needs K even and unit strides");
        if (!gemm_aligned(d_A, sam))
            return fail(PGL_ERR_ARG, "pgl_gemm_dev: k_gemm_kc needs a 16-byte aligned A with an even leading dimension");
        return launch_gemm_kc<1, 0, 16>(h, d_A, sam, d_B, sbk, d_C, scm, scn, M, N, K);
    default:
        return fail(PGL_ERR_ARG, "pgl_gemm_dev: unknown kernel");
    }
}

// ---- time rescaling: integrated rate between consecutive events (pglm_rescale.hip.h) ---------------------------------
int pgl_rescale_count(pgl_handle h, int64_t* off_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!h->have_spikes) return fail(PGL_ERR_STATE, "pgl_set_spikes_* has not been called");
    if (!off_out) return fail(PGL_ERR_ARG, "null argument");
    off_out[0] = 0;
    for (int n = 0; n < h->N; ++n) {
        int lo, hi;
        event_range(h, n, lo, hi);
        off_out[n + 1] = off_out[n] + std::max(hi - lo - 1, 0);
    }
    return PGL_OK;
}

// ---- what the three consumers of GX below share: staging of a draw, launch geometry, launches behind a forward pass -----
// theta / Weff of a draw on the device -> h->gtheta / h->Weff (no copy where they are the handle's own buffers already), then
// the forward-only pass: GX of the handle's time range is on the stream
static int forward_from_dev(pgl_handle h, const double* d_theta, const double* d_Weff)
{
    HIPCHK(hipSetDevice(h->device));
    const size_t tb = (size_t)h->N * (1 + (size_t)h->Dstim + h->Kimp) * 8, wb = (size_t)h->N * h->N * 8;
    ENSURE(h->gtheta, tb);
    ENSURE(h->Weff, wb);
    if (d_theta != h->gtheta.p) HIPCHK(hipMemcpyAsync(h->gtheta.p, d_theta, tb, hipMemcpyDeviceToDevice, h->stream));
    if (d_Weff != h->Weff.p) HIPCHK(hipMemcpyAsync(h->Weff.p, d_Weff, wb, hipMemcpyDeviceToDevice, h->stream));
    return enqueue_gibbs_forward(h);
}

// chunks of PGL_RS_CHUNK bins of the handle's time range
static long long rs_chunks(const pgl_context* h) { return (h->t_hi - h->t_lo + PGL_RS_CHUNK - 1) / PGL_RS_CHUNK; }

// what the walking kernels read (pglm_binwalk.hip.h); the dry run's context has no forward pass behind it: its row stride is
// the padded N
static BinSource bin_source(const pgl_context* h)
{
    BinSource s;
    s.GX = (const double*)h->GX.p; s.theta = (const double*)h->gtheta.p;
    s.spk = (const int2*)h->spk.p; s.wlo = (const int*)h->wlo.p; s.whi = (const int*)h->whi.p;
    s.t_lo = h->t_lo; s.t_hi = h->t_hi;
    s.N = h->N; s.xs = g_dry ? 16 * ((h->N + 15) / 16) : h->gx_xs; s.P = 1 + h->Dstim + h->Kimp; s.nnz = (int)h->nnz;
    s.dt = h->dt;
    return s;
}

extern "C++" {                                   // (templates over the params struct)
// One launch behind a forward pass, `threads` a workgroup.  The dry run records the name and launches nothing -- the g_dry
// guard the RULE above enqueue_ll_grad asks for; PGL_OPT_RECORD_KERNELS appends it behind the forward launches.
template <typename Prm>
static int launch_behind(pgl_handle h, const std::string& name, void (*kern)(Prm), unsigned blocks, unsigned threads,
                         const Prm& p)
{
    struct Append {
        explicit Append(pgl_context* h) { if (h->opt_record && !g_dry) g_rec = &h->last_kernels; }
        ~Append() { g_rec = nullptr; }
    } record(h);
    if (g_dry || g_rec) (g_dry ? g_dry : g_rec)->push_back(name);
    if (g_dry) return PGL_OK;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, h->stream, p);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

// the same for a kernel over units x columns of GX (256 threads a workgroup); walk1 / walk0: the explinear / exp
// instantiations of a walking kernel `fam`
static unsigned gx_blocks(long long units, const BinSource& s) { return (unsigned)((units * s.xs + 255) / 256); }
template <typename Prm>
static int launch_walk(pgl_handle h, const char* fam, void (*walk1)(Prm), void (*walk0)(Prm), long long units, const Prm& p)
{
    const bool el = h->nlin == PGL_NLIN_EXPLINEAR;
    return launch_behind(h, std::string(fam) + (el ? "<1>" : "<0>"), el ? walk1 : walk0, gx_blocks(units, p.src), 256, p);
}
}  // extern "C++"

// the k_rescale_* launches behind a forward pass.  The dry run of the dispatch runs this too: see launch_behind.
// corr: the discrete-time corrected intervals (k_rcorr_chunk / k_rcorr_finish around the same scan).
static int enqueue_rescale(pgl_handle h, double* d_tau, const long long* d_off, double* d_stats, bool corr, unsigned long long seed,
                           long long draw)
{
    RescaleParams p;
    p.src = bin_source(h);
    p.nchunks = (int)rs_chunks(h);
    p.qev = nullptr; p.tail = nullptr; p.lam_row = nullptr; p.seed = seed; p.draw = draw;
    // the corrected variant walks the absolute chunk grid: one chunk more where t_lo lies inside a chunk
    p.c0 = h->t_lo / PGL_RS_CHUNK;
    p.nchunks_abs = (int)((h->t_hi + PGL_RS_CHUNK - 1) / PGL_RS_CHUNK - p.c0);
    const bool on_grid = h->t_lo % PGL_RS_CHUNK == 0;
    ENSURE(h->rs_pre, (size_t)std::max<int64_t>(h->nnz, 1) * 8);
    if (corr) {
        ENSURE(h->rs_qev, (size_t)std::max<int64_t>(h->nnz, 1) * 8);
        ENSURE(h->rs_tail, (size_t)p.nchunks_abs * p.src.xs * 8);
        p.qev = (double*)h->rs_qev.p;
        p.tail = (double*)h->rs_tail.p;
    }
    ENSURE(h->rs_tot, (size_t)std::max(p.nchunks, p.nchunks_abs) * p.src.xs * 8);
    ENSURE(h->rs_cum, (size_t)(p.nchunks + 1) * p.src.xs * 8);
    p.pre = (double*)h->rs_pre.p; p.tot = (double*)h->rs_tot.p; p.cum = (double*)h->rs_cum.p;
    p.off = d_off; p.tau = d_tau; p.stats = d_stats;
    p.lam_row = p.cum + (size_t)p.nchunks * p.src.xs;
    int rc;
    if (corr && !on_grid) {
        // a range that starts inside a chunk: the expected count of stats is pgl_rescale_dev's own sum over the chunks from
        // t_lo (a second read of the currents, for such ranges only), then the corrected intervals on the absolute grid
        rc = launch_walk(h, "k_rescale_chunk", k_rescale_chunk<1>, k_rescale_chunk<0>, p.nchunks, p);
        if (rc) return rc;
        rc = launch_behind(h, "k_rescale_scan", k_rescale_scan, (h->N + 15) / 16, 16 * PGL_RS_SEGS, p);
        if (rc) return rc;
        rc = launch_walk(h, "k_rcorr_chunk", k_rcorr_chunk<1>, k_rcorr_chunk<0>, p.nchunks_abs, p);
        if (rc) return rc;
        return launch_behind(h, "k_rcorr_finish", k_rcorr_finish, h->N, 256, p);
    }
    rc = corr ? launch_walk(h, "k_rcorr_chunk", k_rcorr_chunk<1>, k_rcorr_chunk<0>, p.nchunks_abs, p)
              : launch_walk(h, "k_rescale_chunk", k_rescale_chunk<1>, k_rescale_chunk<0>, p.nchunks, p);
    if (rc) return rc;
    rc = launch_behind(h, "k_rescale_scan", k_rescale_scan, (h->N + 15) / 16, 16 * PGL_RS_SEGS, p);
    if (rc) return rc;
    return corr ? launch_behind(h, "k_rcorr_finish", k_rcorr_finish, h->N, 256, p)
                : launch_behind(h, "k_rescale_finish", k_rescale_finish, h->N, 256, p);
}

static int rescale_host(pgl_handle h, const double* theta, const double* Weff, double* tau_out, double* stats_out, bool corr,
                        uint64_t seed, int64_t draw);

static int rescale_dev(pgl_handle h, const double* d_theta, const double* d_Weff, double* d_tau, const int64_t* d_off,
                       double* d_stats, bool corr, uint64_t seed, int64_t draw)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_theta || !d_Weff || !d_tau || !d_off || !d_stats) return fail(PGL_ERR_ARG, "null argument");
    if (draw < 0) return fail(PGL_ERR_ARG, "draw must not be negative");
    if (rs_chunks(h) > 0x7fffffff / 2048) return fail(PGL_ERR_UNSUPPORTED, "time range too long for the rescaling kernels");
    rc = forward_from_dev(h, d_theta, d_Weff);
    if (rc) return rc;
    return enqueue_rescale(h, d_tau, (const long long*)d_off, d_stats, corr, seed, draw);
}

int pgl_rescale_dev(pgl_handle h, const double* d_theta, const double* d_Weff, double* d_tau, const int64_t* d_off,
                    double* d_stats)
{
    return rescale_dev(h, d_theta, d_Weff, d_tau, d_off, d_stats, false, 0, 0);
}

// ---- the discrete-time corrected intervals and the KS distance of segmented samples (pglm_gof.h, pglm_gof.hip.h) ---------
int pgl_rescale_corr_dev(pgl_handle h, const double* d_theta, const double* d_Weff, uint64_t seed, int64_t draw, double* d_tau,
                         const int64_t* d_off, double* d_stats)
{
    return rescale_dev(h, d_theta, d_Weff, d_tau, d_off, d_stats, true, seed, draw);
}

int pgl_rescale_corr(pgl_handle h, const double* theta, const double* Weff, uint64_t seed, int64_t draw, double* tau_out,
                     double* stats_out)
{
    return rescale_host(h, theta, Weff, tau_out, stats_out, true, seed, draw);
}

int pgl_ks_uniform_dev(pgl_handle h, const double* d_tau, const int64_t* d_off, int64_t M, double* d_ks, double* d_zsorted)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!d_tau || !d_off || !d_ks) return fail(PGL_ERR_ARG, "null argument");
    if (pgl_gof_bad_count(M)) return fail(PGL_ERR_ARG, "pgl_ks_uniform_dev: M must lie in 1 .. 2^31 - 1");
    HIPCHK(hipSetDevice(h->device));
    if (!d_zsorted) {
        // the network sorts in place: room for every z.  The one place where the call waits for the device
        int64_t total = 0;
        HIPCHK(hipMemcpyAsync(&total, d_off + M, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (total < 0) return fail(PGL_ERR_ARG, "pgl_ks_uniform_dev: negative offsets");
        ENSURE(h->ks_work, (size_t)std::max<int64_t>(total, 1) * 8);
        d_zsorted = (double*)h->ks_work.p;
    }
    KsParams p;
    p.tau = d_tau; p.off = (const long long*)d_off; p.zs = d_zsorted; p.ks = d_ks;
    return launch_behind(h, "k_ks_segment", k_ks_segment, (unsigned)M, PGL_KS_THREADS, p);
}

int pgl_ks_uniform(pgl_handle h, const double* tau, const int64_t* off, int64_t M, double* ks_out, double* zsorted_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!tau || !off || !ks_out) return fail(PGL_ERR_ARG, "null argument");
    if (pgl_gof_bad_count(M)) return fail(PGL_ERR_ARG, "pgl_ks_uniform: M must lie in 1 .. 2^31 - 1");
    if (pgl_gof_bad_offsets((const long long*)off, M)) return fail(PGL_ERR_ARG, "pgl_ks_uniform: offsets must not decrease");
    HIPCHK(hipSetDevice(h->device));
    const size_t tb = (size_t)off[M] * 8, ob = (size_t)M * PGL_KS_NOUT * 8;
    PASS(stage_up(h, 0, tau, tb));
    PASS(stage_up(h, 1, off, ((size_t)M + 1) * 8));
    PASS(stage_up(h, 2, nullptr, ob));
    ENSURE(h->ks_work, std::max<size_t>(tb, 8));
    PASS(pgl_ks_uniform_dev(h, (const double*)h->stage[0].p, (const int64_t*)h->stage[1].p, M, (double*)h->stage[2].p,
                            (double*)h->ks_work.p));
    PASS(stage_down(h, ks_out, h->stage[2].p, ob));
    PASS(stage_down(h, zsorted_out, h->ks_work.p, tb));
    return stage_end(h);
}

// ---- the serial correlation of the normal scores of segmented, run-structured intervals (pglm_acf.h, pglm_acf.hip.h) ------
static int enqueue_acf(pgl_handle h, const double* d_tau, const int64_t* d_run_off, const int64_t* d_seg_run, int64_t M, int max_lag,
                       double* d_out, double* d_scores)
{
    AcfParams p;
    p.tau = d_tau; p.run_off = (const long long*)d_run_off; p.seg_run = (const long long*)d_seg_run;
    p.scores = d_scores; p.out = d_out; p.L = max_lag;
    return launch_behind(h, "k_acf_segment", k_acf_segment, (unsigned)M, PGL_ACF_THREADS, p);
}

int pgl_rescale_acf_dev(pgl_handle h, const double* d_tau, const int64_t* d_run_off, const int64_t* d_seg_run, int64_t M,
                        int max_lag, double* d_out, double* d_scores)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!d_tau || !d_run_off || !d_seg_run || !d_out || !d_scores) return fail(PGL_ERR_ARG, "null argument");
    if (pgl_gof_bad_count(M)) return fail(PGL_ERR_ARG, "pgl_rescale_acf_dev: M must lie in 1 .. 2^31 - 1");
    if (max_lag < 1 || max_lag > PGL_ACF_MAX_LAG) return fail(PGL_ERR_ARG, "pgl_rescale_acf_dev: max_lag must lie in 1 .. 64");
    HIPCHK(hipSetDevice(h->device));
    return enqueue_acf(h, d_tau, d_run_off, d_seg_run, M, max_lag, d_out, d_scores);
}

int pgl_rescale_acf(pgl_handle h, const double* tau, const int64_t* run_off, const int64_t* seg_run, int64_t M, int max_lag,
                    double* out, double* scores_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!tau || !run_off || !seg_run || !out) return fail(PGL_ERR_ARG, "null argument");
    if (pgl_gof_bad_count(M)) return fail(PGL_ERR_ARG, "pgl_rescale_acf: M must lie in 1 .. 2^31 - 1");
    if (max_lag < 1 || max_lag > PGL_ACF_MAX_LAG) return fail(PGL_ERR_ARG, "pgl_rescale_acf: max_lag must lie in 1 .. 64");
    // (the runs of the segments first: their count R is the last of seg_run)
    if (pgl_gof_bad_offsets((const long long*)seg_run, M) || pgl_gof_bad_offsets((const long long*)run_off, seg_run[M]))
        return fail(PGL_ERR_ARG, "pgl_rescale_acf: offsets must not decrease");
    HIPCHK(hipSetDevice(h->device));
    const size_t R = (size_t)seg_run[M], tb = (size_t)run_off[R] * 8, ob = (size_t)M * (PGL_ACF_NHEAD + max_lag) * 8;
    PASS(stage_up(h, 0, tau, tb));
    PASS(stage_up(h, 1, run_off, (R + 1) * 8));
    PASS(stage_up(h, 2, seg_run, ((size_t)M + 1) * 8));
    PASS(stage_up(h, 3, nullptr, ob));
    ENSURE(h->ks_work, std::max<size_t>(tb, 8));
    PASS(pgl_rescale_acf_dev(h, (const double*)h->stage[0].p, (const int64_t*)h->stage[1].p, (const int64_t*)h->stage[2].p, M, max_lag,
                             (double*)h->stage[3].p, (double*)h->ks_work.p));
    PASS(stage_down(h, out, h->stage[3].p, ob));
    PASS(stage_down(h, scores_out, h->ks_work.p, tb));
    return stage_end(h);
}

int pgl_rescale(pgl_handle h, const double* theta, const double* Weff, double* tau_out, double* stats_out)
{
    return rescale_host(h, theta, Weff, tau_out, stats_out, false, 0, 0);
}

static int rescale_host(pgl_handle h, const double* theta, const double* Weff, double* tau_out, double* stats_out, bool corr,
                        uint64_t seed, int64_t draw)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff || !tau_out || !stats_out) return fail(PGL_ERR_ARG, "null argument");
    if (draw < 0) return fail(PGL_ERR_ARG, "draw must not be negative");
    HIPCHK(hipSetDevice(h->device));
    const int N = h->N;
    std::vector<int64_t> off((size_t)N + 1);
    rc = pgl_rescale_count(h, off.data());
    if (rc) return rc;
    const size_t tb = (size_t)off[(size_t)N] * 8, sb = (size_t)N * 4 * 8;
    PASS(stage_up(h, 0, off.data(), ((size_t)N + 1) * 8));
    PASS(stage_up(h, 1, nullptr, tb));
    PASS(stage_up(h, 2, nullptr, sb));
    PASS(upload_draw(h, theta, Weff));
    PASS(rescale_dev(h, (const double*)h->gtheta.p, (const double*)h->Weff.p, (double*)h->stage[1].p,
                     (const int64_t*)h->stage[0].p, (double*)h->stage[2].p, corr, seed, draw));
    PASS(stage_down(h, tau_out, h->stage[1].p, tb));
    PASS(stage_down(h, stats_out, h->stage[2].p, sb));
    return stage_end(h);
}

// ---- pointwise log-likelihood: block sums of the ll terms of a draw (pglm_pointwise.hip.h) ------------------------------
int pgl_pointwise_count(pgl_handle h, int block_chunks, int64_t* n_blocks_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!n_blocks_out) return fail(PGL_ERR_ARG, "null argument");
    if (block_chunks < 1) return fail(PGL_ERR_ARG, "block_chunks must be at least 1");
    *n_blocks_out = (rs_chunks(h) + block_chunks - 1) / block_chunks;
    return PGL_OK;
}

// the k_pw_* launches behind a forward pass.  The dry run of the dispatch runs this too: see launch_behind.
static int enqueue_pointwise(pgl_handle h, int block_chunks, double* d_ll_blk, double* d_acc, long long draw)
{
    const long long nchunks = rs_chunks(h);
    PointwiseParams p;
    p.src = bin_source(h);
    ENSURE(h->pw_part, (size_t)nchunks * p.src.xs * 8);
    p.part = (double*)h->pw_part.p; p.ll_blk = d_ll_blk; p.acc = d_acc;
    p.draw = draw;
    p.nchunks = (int)nchunks;
    p.block_chunks = (int)std::min<long long>(block_chunks, nchunks);
    p.n_blocks = (int)((nchunks + block_chunks - 1) / block_chunks);
    const int rc = launch_walk(h, "k_pw_chunk", k_pw_chunk<1>, k_pw_chunk<0>, nchunks, p);
    if (rc) return rc;
    return launch_behind(h, "k_pw_block", k_pw_block, gx_blocks(p.n_blocks, p.src), 256, p);
}

int pgl_pointwise_dev(pgl_handle h, const double* d_theta, const double* d_Weff, int block_chunks, double* d_ll_blk,
                      double* d_acc, int64_t draw)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_theta || !d_Weff) return fail(PGL_ERR_ARG, "null argument");
    if (!d_ll_blk && !d_acc) return fail(PGL_ERR_ARG, "pointwise ll: neither d_ll_blk nor d_acc is given");
    if (block_chunks < 1) return fail(PGL_ERR_ARG, "block_chunks must be at least 1");
    if (draw < 0) return fail(PGL_ERR_ARG, "draw must not be negative");
    if (rs_chunks(h) > 0x7fffffff / 2048) return fail(PGL_ERR_UNSUPPORTED, "time range too long for the pointwise kernels");
    rc = forward_from_dev(h, d_theta, d_Weff);
    if (rc) return rc;
    return enqueue_pointwise(h, block_chunks, d_ll_blk, d_acc, (long long)draw);
}

int pgl_pointwise(pgl_handle h, const double* theta, const double* Weff, int block_chunks, double* ll_blk_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff || !ll_blk_out) return fail(PGL_ERR_ARG, "null argument");
    int64_t n_blocks = 0;
    rc = pgl_pointwise_count(h, block_chunks, &n_blocks);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n_blocks * h->N * 8;
    PASS(stage_up(h, 0, nullptr, bytes));
    PASS(upload_draw(h, theta, Weff));
    PASS(pgl_pointwise_dev(h, (const double*)h->gtheta.p, (const double*)h->Weff.p, block_chunks, (double*)h->stage[0].p,
                           nullptr, 0));
    PASS(stage_down(h, ll_blk_out, h->stage[0].p, bytes));
    return stage_end(h);
}

// ---- rate windows: expected and observed counts over time windows, folded over draws (pglm_ratewin.hip.h) ----------------
// (n_win, pieces) of the handle's time range at this window length
static void rate_windows_shape(const pgl_context* h, long long win, long long& n_win, long long& npieces)
{
    const long long n = h->t_hi - h->t_lo;
    n_win = pgl_rw_windows(n, win);
    npieces = (n_win - 1) * pgl_rw_pieces(win) + pgl_rw_pieces(n - (n_win - 1) * win);
}

int pgl_rate_windows_count(pgl_handle h, int64_t win, int64_t* n_win_out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!n_win_out) return fail(PGL_ERR_ARG, "null argument");
    if (win < 1) return fail(PGL_ERR_ARG, "win must be at least 1");
    *n_win_out = pgl_rw_windows(h->t_hi - h->t_lo, win);
    return PGL_OK;
}

// the k_rw_* launches behind a forward pass.  The dry run of the dispatch runs this too: see launch_behind.
static int enqueue_rate_windows(pgl_handle h, long long win, double* d_lam, double* d_obs, double* d_acc, long long draw)
{
    RateWinParams p;
    p.src = bin_source(h);
    p.win = std::min<long long>(win, h->t_hi - h->t_lo);      // (one window: its length is the range)
    rate_windows_shape(h, p.win, p.n_win, p.npieces);
    ENSURE(h->rw_part, (size_t)p.npieces * p.src.xs * 8);
    ENSURE(h->rw_cnt, (size_t)p.npieces * p.src.xs * 4);
    p.part = (double*)h->rw_part.p; p.cnt = (int*)h->rw_cnt.p; p.lam = d_lam; p.obs = d_obs; p.acc = d_acc;
    p.draw = draw;
    p.ppw = (int)pgl_rw_pieces(p.win);
    p.group = (p.ppw == 1) ? (int)std::max<long long>(PGL_RW_PIECE / p.win, 1) : 1;
    p.nunits = (p.npieces + p.group - 1) / p.group;
    const int rc = launch_walk(h, "k_rw_piece", k_rw_piece<1>, k_rw_piece<0>, p.nunits, p);
    if (rc) return rc;
    return launch_behind(h, "k_rw_window", k_rw_window, gx_blocks(p.n_win, p.src), 256, p);
}

int pgl_rate_windows_dev(pgl_handle h, const double* d_theta, const double* d_Weff, int64_t win, double* d_lam, double* d_obs,
                         double* d_acc, int64_t draw)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!d_theta || !d_Weff) return fail(PGL_ERR_ARG, "null argument");
    if (!d_lam && !d_obs && !d_acc) return fail(PGL_ERR_ARG, "rate windows: none of d_lam, d_obs and d_acc is given");
    if (win < 1) return fail(PGL_ERR_ARG, "win must be at least 1");
    if (draw < 0) return fail(PGL_ERR_ARG, "draw must not be negative");
    {
        // a property of the shape alone, so it is answered before the state of the handle: windows and pieces times the row
        // stride of the currents are indexed in 32 bits by the launch grids
        long long n_win, npieces;
        rate_windows_shape(h, std::min<long long>(win, h->t_hi - h->t_lo), n_win, npieces);
        const long long xs = 16 * (((long long)h->N + 15) / 16);
        if (n_win * xs > 0x7fffffffLL || npieces * xs > 0x7fffffffLL)
            return fail(PGL_ERR_UNSUPPORTED, "too many windows x neurons for the rate-window kernels: use a longer window or a shorter time range");
    }
    int rc = check_ready(h);
    if (rc) return rc;
    rc = forward_from_dev(h, d_theta, d_Weff);
    if (rc) return rc;
    return enqueue_rate_windows(h, (long long)win, d_lam, d_obs, d_acc, (long long)draw);
}

int pgl_rate_windows(pgl_handle h, const double* theta, const double* Weff, int64_t win, double* lam_out, double* obs_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff || !lam_out || !obs_out) return fail(PGL_ERR_ARG, "null argument");
    int64_t n_win = 0;
    rc = pgl_rate_windows_count(h, win, &n_win);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n_win * h->N * 8;
    PASS(stage_up(h, 0, nullptr, 2 * bytes));
    PASS(upload_draw(h, theta, Weff));
    double* d_lam = (double*)h->stage[0].p;
    double* d_obs = d_lam + (size_t)n_win * h->N;
    PASS(pgl_rate_windows_dev(h, (const double*)h->gtheta.p, (const double*)h->Weff.p, win, d_lam, d_obs, nullptr, 0));
    PASS(stage_down(h, lam_out, d_lam, bytes));
    PASS(stage_down(h, obs_out, d_obs, bytes));
    return stage_end(h);
}

// ---- PSIS-LOO of the columns of a pointwise matrix (pglm_psis.hip.h) ---------------------------------------------------
int pgl_psis_loo_dev(pgl_handle h, const double* d_ll, int64_t S, int64_t C, int64_t ld, double* d_out, double* d_lw)
{
    if (!h || !d_ll || !d_out || S < 2 || C < 1 || ld < C) return fail(PGL_ERR_ARG, "bad argument");
    if (C > 0x7fffffff) return fail(PGL_ERR_ARG, "at most 2^31 - 1 columns per call");
    if (S > PGL_PSIS_MAX_DRAWS)
        return fail(PGL_ERR_UNSUPPORTED, "PSIS-LOO: more than PGL_PSIS_MAX_DRAWS = " + std::to_string(PGL_PSIS_MAX_DRAWS) +
                                         " draws do not fit a workgroup's LDS");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_psis_column, dim3((unsigned)C), dim3(PGL_PSIS_THREADS), psis_lds_bytes(S), h->stream, d_ll,
                       (long long)S, (long long)C, (long long)ld, d_out, d_lw);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_psis_loo(pgl_handle h, const double* ll, int64_t S, int64_t C, double* out, double* lw)
{
    if (!h || !ll || !out || S < 2 || C < 1) return fail(PGL_ERR_ARG, "bad argument");
    if (S > PGL_PSIS_MAX_DRAWS) return pgl_psis_loo_dev(h, ll, S, C, C, out, lw);       // (its error, before any copy)
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)S * C * 8, obytes = (size_t)PGL_PSIS_NOUT * C * 8;
    PASS(stage_up(h, 0, ll, bytes));
    PASS(stage_up(h, 1, nullptr, obytes));
    if (lw) PASS(stage_up(h, 2, nullptr, bytes));
    PASS(pgl_psis_loo_dev(h, (const double*)h->stage[0].p, S, C, C, (double*)h->stage[1].p, lw ? (double*)h->stage[2].p : nullptr));
    PASS(stage_down(h, out, h->stage[1].p, obytes));
    PASS(stage_down(h, lw, h->stage[2].p, bytes));
    return stage_end(h);
}

// ---- Wald statistics of the coupling groups from the factor of the Laplace covariance (pglm_wald.hip.h) -------------------
static int wald_check(pgl_handle h, const void* W, int M, int P, int ld, const void* theta, int first, int G, int B, const void* c,
                      const void* info, const void* out)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!W || !theta || !c || !info || !out) return fail(PGL_ERR_ARG, "pgl_wald_groups: null argument");
    if (M <= 0 || G <= 0 || B <= 0 || P <= 0 || ld < P || first < 0 || (long long)first + (long long)G * B > P)
        return fail(PGL_ERR_ARG, "pgl_wald_groups: M, G, B >= 1, ld >= P, first >= 0 and first + G B <= P");
    if (B > PGL_WALD_MAX_B)
        return fail(PGL_ERR_UNSUPPORTED, "pgl_wald_groups: groups of more than PGL_WALD_MAX_B = " + std::to_string(PGL_WALD_MAX_B) +
                                         " weights");
    if (M > 65535) return fail(PGL_ERR_UNSUPPORTED, "pgl_wald_groups: at most 65535 rows per call");
    return PGL_OK;
}

int pgl_wald_groups_dev(pgl_handle h, const double* d_W, int M, int P, int ld, const double* d_theta, int first, int G, int B,
                        const double* d_c, const int* d_info, double* d_out, double* d_u)
{
    PASS(wald_check(h, d_W, M, P, ld, d_theta, first, G, B, d_c, d_info, d_out));
    HIPCHK(hipSetDevice(h->device));
    WaldParams p;
    p.W = d_W; p.theta = d_theta; p.c = d_c; p.info = d_info; p.out = d_out; p.u = d_u;
    p.P = P; p.ld = ld; p.M = M; p.first = first; p.G = G;
    wald_launch(B, p, h->stream);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_wald_groups(pgl_handle h, const double* W, int M, int P, int ld, const double* theta, int first, int G, int B, const double* c,
                    const int* info, double* out, double* u)
{
    PASS(wald_check(h, W, M, P, ld, theta, first, G, B, c, info, out));
    HIPCHK(hipSetDevice(h->device));
    const size_t wb = (size_t)M * P * ld * 8, tb = (size_t)M * P * 8, ob = (size_t)M * G * PGL_WALD_NOUT * 8, ub = (size_t)G * M * P * 8;
    PASS(stage_up(h, 0, W, wb));
    PASS(stage_up(h, 1, theta, tb));
    PASS(stage_up(h, 2, c, (size_t)B * 8));
    PASS(stage_up(h, 3, info, (size_t)M * 4));
    PASS(stage_up(h, 4, nullptr, ob));
    if (u) PASS(stage_up(h, 5, nullptr, ub));
    PASS(pgl_wald_groups_dev(h, (const double*)h->stage[0].p, M, P, ld, (const double*)h->stage[1].p, first, G, B,
                             (const double*)h->stage[2].p, (const int*)h->stage[3].p, (double*)h->stage[4].p,
                             u ? (double*)h->stage[5].p : nullptr));
    PASS(stage_down(h, out, h->stage[4].p, ob));
    PASS(stage_down(h, u, h->stage[5].p, ub));
    return stage_end(h);
}

// ---- convergence diagnostics of the columns of a samplers' tensor (pglm_diag.hip.h) ----------------------------------------
int pgl_chain_diag_dev(pgl_handle h, const double* d_x, int64_t n, int64_t C, int64_t K, int64_t ld, double* d_out)
{
    if (!h || !d_x || !d_out || n < PGL_DIAG_MIN_N || C < 1 || K < 1 || ld < K) return fail(PGL_ERR_ARG, "bad argument");
    if (K > 0x7fffffff) return fail(PGL_ERR_ARG, "at most 2^31 - 1 columns per call");
    if (n > PGL_DIAG_MAX_DRAWS || C > PGL_DIAG_MAX_DRAWS || n * C > PGL_DIAG_MAX_DRAWS)
        return fail(PGL_ERR_UNSUPPORTED, "chain diagnostics: more than PGL_DIAG_MAX_DRAWS = " + std::to_string(PGL_DIAG_MAX_DRAWS) +
                                         " pooled draws do not fit a workgroup's LDS");
    HIPCHK(hipSetDevice(h->device));
    const size_t lds = diag_lds_bytes(n, C);
    if (lds + PGL_DIAG_STATIC_LDS > 65536)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_diag_column), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    hipLaunchKernelGGL(k_diag_column, dim3((unsigned)K), dim3(PGL_DIAG_THREADS), lds, h->stream, d_x, (int)n, (int)C,
                       (long long)K, (long long)ld, d_out);
    HIPCHK(hipGetLastError());
    return PGL_OK;
}

int pgl_chain_diag(pgl_handle h, const double* x, int64_t n, int64_t C, int64_t K, double* out)
{
    if (!h || !x || !out || n < PGL_DIAG_MIN_N || C < 1 || K < 1) return fail(PGL_ERR_ARG, "bad argument");
    if (n > PGL_DIAG_MAX_DRAWS || C > PGL_DIAG_MAX_DRAWS || n * C > PGL_DIAG_MAX_DRAWS)
        return pgl_chain_diag_dev(h, x, n, C, K, K, out);                                // (its error, before any copy)
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n * C * K * 8, obytes = (size_t)PGL_DIAG_NOUT * K * 8;
    PASS(stage_up(h, 0, x, bytes));
    PASS(stage_up(h, 1, nullptr, obytes));
    PASS(pgl_chain_diag_dev(h, (const double*)h->stage[0].p, n, C, K, K, (double*)h->stage[1].p));
    PASS(stage_down(h, out, h->stage[1].p, obytes));
    return stage_end(h);
}

// ---- posterior bands of the filters from the samplers' draws (pglm_filters.hip.h) -----------------------------------------
static int filt_check(pgl_handle h, const void* x, int64_t n, int64_t C, int M, int P, int first, int G, int B, const void* basis,
                      int R, const void* c, double level, const void* out, const void* grp)
{
    if (!h) return fail(PGL_ERR_ARG, "null handle");
    if (!x || !basis || !c || !out || !grp) return fail(PGL_ERR_ARG, "pgl_filter_bands: null argument");
    if (n < 1 || C < 1 || M <= 0 || G <= 0 || B <= 0 || R <= 0 || P <= 0 || first < 0 || (long long)first + (long long)G * B > P)
        return fail(PGL_ERR_ARG, "pgl_filter_bands: n, C, M, G, B, R >= 1, first >= 0 and first + G B <= P");
    if (n == 1 && C == 1) return fail(PGL_ERR_ARG, "pgl_filter_bands: at least 2 pooled draws");
    if (n > PGL_FILT_MAX_DRAWS || C > PGL_FILT_MAX_DRAWS || n * C > PGL_FILT_MAX_DRAWS)
        return fail(PGL_ERR_UNSUPPORTED, "pgl_filter_bands: more than PGL_FILT_MAX_DRAWS = " + std::to_string(PGL_FILT_MAX_DRAWS) +
                                         " pooled draws do not fit a workgroup's LDS");
    if (!(level > 0.0 && level < 1.0)) return fail(PGL_ERR_ARG, "pgl_filter_bands: level in (0, 1)");
    if (B > PGL_FILT_MAX_B)
        return fail(PGL_ERR_UNSUPPORTED, "pgl_filter_bands: groups of more than PGL_FILT_MAX_B = " + std::to_string(PGL_FILT_MAX_B) +
                                         " weights");
    if (M > 65535) return fail(PGL_ERR_UNSUPPORTED, "pgl_filter_bands: at most 65535 rows per call");
    return PGL_OK;
}

int pgl_filter_bands_dev(pgl_handle h, const double* d_samples, int64_t n_keep, int64_t C, int M, int P, int first, int G, int B,
                         const double* d_basis, int R, const double* d_c, double level, double* d_out, double* d_grp)
{
    PASS(filt_check(h, d_samples, n_keep, C, M, P, first, G, B, d_basis, R, d_c, level, d_out, d_grp));
    HIPCHK(hipSetDevice(h->device));
    FiltParams p;
    p.x = d_samples; p.basis = d_basis; p.c = d_c; p.out = d_out; p.grp = d_grp; p.level = level;
    p.P = P; p.n = (int)n_keep; p.C = (int)C; p.M = M; p.first = first; p.G = G; p.R = R; p.Spad = 0; p.resident = 0;
    HIPCHK(filt_launch(B, p, h->stream));
    return PGL_OK;
}

int pgl_filter_bands(pgl_handle h, const double* samples, int64_t n_keep, int64_t C, int M, int P, int first, int G, int B,
                     const double* basis, int R, const double* c, double level, double* out, double* grp)
{
    PASS(filt_check(h, samples, n_keep, C, M, P, first, G, B, basis, R, c, level, out, grp));
    HIPCHK(hipSetDevice(h->device));
    const size_t xb = (size_t)n_keep * C * M * P * 8, ob = (size_t)M * G * R * PGL_FILT_NLAG * 8, gb = (size_t)M * G * PGL_FILT_NGRP * 8;
    PASS(stage_up(h, 0, samples, xb));
    PASS(stage_up(h, 1, basis, (size_t)R * B * 8));
    PASS(stage_up(h, 2, c, (size_t)B * 8));
    PASS(stage_up(h, 3, nullptr, ob));
    PASS(stage_up(h, 4, nullptr, gb));
    PASS(pgl_filter_bands_dev(h, (const double*)h->stage[0].p, n_keep, C, M, P, first, G, B, (const double*)h->stage[1].p, R,
                              (const double*)h->stage[2].p, level, (double*)h->stage[3].p, (double*)h->stage[4].p));
    PASS(stage_down(h, out, h->stage[3].p, ob));
    PASS(stage_down(h, grp, h->stage[4].p, gb));
    return stage_end(h);
}

// ---- stimulus decoding: F(u), its gradient and its Hessian-vector products with respect to the stimulus (pglm_decode.hip.h) ---
static int dec_served(const pgl_context* h)
{
    if (h->sep) return fail(PGL_ERR_UNSUPPORTED, "stimulus decoding with a separable stimulus");
    if (!h->dec_stim || h->Dstim == 0)
        return fail(PGL_ERR_UNSUPPORTED, "stimulus decoding needs a 'basis' stimulus (pgl_set_stimulus with the identity spatial "
                                         "basis in layout 1)");
    if (h->t_lo != 0 || h->t_hi != h->nT) return fail(PGL_ERR_UNSUPPORTED, "stimulus decoding of a time range");
    if ((long long)h->nT * std::max(h->N, h->dec_D) > (1LL << 38))
        return fail(PGL_ERR_UNSUPPORTED, "recording too long for the decoding kernels");
    return PGL_OK;
}
static unsigned dec_blocks(long long n) { return (unsigned)((n + 255) / 256); }
static DecAux dec_aux(const pgl_context* h, int64_t Tu, int q, const PglDecPrior& prior)
{
    DecAux a;
    a.a = a.b = nullptr; a.out = a.col = nullptr;
    a.nT = h->nT; a.Tu = Tu; a.nchunks = (h->nT + PGL_DEC_CHUNK - 1) / PGL_DEC_CHUNK;
    a.N = h->N; a.D = h->dec_D; a.B = h->dec_B; a.P = 1 + h->Dstim + h->Kimp; a.Rt = h->dec_Rt; a.q = q;
    a.xs = g_dry ? 16 * ((h->N + 15) / 16) : h->gx_xs;
    a.prior = prior; a.center = 0.0;
    return a;
}
static DecParams dec_params(const pgl_context* h)
{
    DecParams p;
    p.src = bin_source(h);
    p.K = (const double*)h->dec_K.p; p.c = (const double*)h->dec_c.p; p.s = (const double*)h->dec_s.p; p.yin = nullptr;
    p.r = (double*)h->dec_r.p; p.cc = (double*)h->dec_cc.p; p.y = (double*)h->dec_y.p; p.part = (double*)h->dec_part.p;
    p.gs = (double*)h->dec_gs.p;
    p.nT = h->nT; p.N = h->N; p.Rt = h->dec_Rt; p.D = h->dec_D; p.cut = std::max(h->opt_dec_cut, 1); p.dt = h->dt;
    return p;
}
static int dec_forward(pgl_handle h, int mode, const DecParams& p)
{
    const bool el = h->nlin == PGL_NLIN_EXPLINEAR;
    const long long nchunks = (h->nT + PGL_DEC_CHUNK - 1) / PGL_DEC_CHUNK, nslabs = (h->N + PGL_DEC_NS - 1) / PGL_DEC_NS;
    const unsigned blocks = (unsigned)((nchunks + p.cut - 1) / p.cut * nslabs);
    if (mode == 0)
        return launch_behind(h, el ? "k_dec_forward<1, 0>" : "k_dec_forward<0, 0>", el ? k_dec_forward<1, 0> : k_dec_forward<0, 0>,
                             blocks, 256, p);
    return launch_behind(h, el ? "k_dec_forward<1, 1>" : "k_dec_forward<0, 1>", el ? k_dec_forward<1, 1> : k_dec_forward<0, 1>, blocks,
                         256, p);
}
// g_s = K^T yin, then out (Tu, D) = L^T g_s + the prior's part at x
static int dec_backward(pgl_handle h, DecParams p, const double* yin, DecAux a, const double* x, double center, double* out)
{
    p.yin = yin;
    const long long ntiles = (h->nT + PGL_DEC_TB - 1) / PGL_DEC_TB;
    PASS(launch_behind(h, "k_dec_backward", k_dec_backward, (unsigned)((ntiles + p.cut - 1) / p.cut), 256, p));
    a.a = p.gs; a.b = x; a.out = out; a.center = center;
    return launch_behind(h, "k_dec_interp_t", k_dec_interp_t, dec_blocks(a.Tu * a.D), 256, a);
}

// theta / Weff of the draw in h->gtheta / h->Weff.  The dry run of the dispatch runs this too: see launch_behind.
static int enqueue_decode_prepare(pgl_handle h)
{
    PASS(dec_served(h));
    const int N = h->N, D = h->dec_D, Rt = h->dec_Rt;
    ENSURE(h->dec_K, (size_t)Rt * D * N * 8);
    ENSURE(h->dec_c, (size_t)h->nT * N * 8);
    const PglDecPrior none = {0.0, 1.0, 0.0};
    DecAux a = dec_aux(h, 1, 1, none);
    a.a = (const double*)h->dec_basis.p; a.b = (const double*)h->gtheta.p; a.out = (double*)h->dec_K.p;
    PASS(launch_behind(h, "k_dec_filters", k_dec_filters, dec_blocks((long long)Rt * D * N), 256, a));
    // the stimulus block of the handle's copy of theta written as zeros: the forward pass leaves the currents of the spikes
    if (!g_dry) HIPCHK(hipMemset2DAsync((char*)h->gtheta.p + 8, (size_t)a.P * 8, 0, (size_t)h->Dstim * 8, (size_t)N, h->stream));
    PASS(enqueue_gibbs_forward(h));
    a = dec_aux(h, 1, 1, none);                                             // (the row stride of GX is known now)
    a.a = (const double*)h->GX.p; a.b = (const double*)h->gtheta.p; a.out = (double*)h->dec_c.p;
    PASS(launch_behind(h, "k_dec_offset", k_dec_offset, dec_blocks((long long)h->nT * N), 256, a));
    h->dec_ok = true;
    h->dec_point = false;
    return PGL_OK;
}

static int enqueue_decode_eval(pgl_handle h, const double* d_u, int64_t Tu, int q, const PglDecPrior& prior, double* d_F,
                               double* d_grad_u)
{
    PASS(dec_served(h));
    if (!h->dec_ok) return fail(PGL_ERR_STATE, "pgl_decode_eval before pgl_decode_prepare (or after new spikes / basis / stimulus)");
    const size_t plane = (size_t)h->nT * h->N * 8, frames = (size_t)h->nT * h->dec_D * 8;
    DecAux a = dec_aux(h, Tu, q, prior);
    ENSURE(h->dec_s, frames);
    ENSURE(h->dec_gs, frames);
    ENSURE(h->dec_r, plane);
    ENSURE(h->dec_cc, plane);
    ENSURE(h->dec_part, (size_t)a.nchunks * h->N * 8);
    ENSURE(h->dec_col, (size_t)h->N * 8);
    a.a = d_u; a.out = (double*)h->dec_s.p;
    PASS(launch_behind(h, "k_dec_interp", k_dec_interp, dec_blocks((long long)h->nT * a.D), 256, a));
    const DecParams p = dec_params(h);
    PASS(dec_forward(h, 0, p));
    a.a = p.part; a.b = d_u; a.out = d_F; a.col = (double*)h->dec_col.p;
    PASS(launch_behind(h, "k_dec_sum", k_dec_sum, 1, 256, a));
    if (d_grad_u) PASS(dec_backward(h, p, p.r, a, d_u, prior.mu, d_grad_u));
    h->dec_Tu = Tu; h->dec_q = q; h->dec_prior = prior;
    h->dec_point = true;
    return PGL_OK;
}

static int enqueue_decode_hvp(pgl_handle h, const double* d_v, double* d_hv)
{
    PASS(dec_served(h));
    if (!h->dec_ok || !h->dec_point) return fail(PGL_ERR_STATE, "pgl_decode_hvp before pgl_decode_eval");
    DecAux a = dec_aux(h, h->dec_Tu, h->dec_q, h->dec_prior);
    ENSURE(h->dec_y, (size_t)h->nT * h->N * 8);
    a.a = d_v; a.out = (double*)h->dec_s.p;
    PASS(launch_behind(h, "k_dec_interp", k_dec_interp, dec_blocks((long long)h->nT * a.D), 256, a));
    const DecParams p = dec_params(h);
    PASS(dec_forward(h, 1, p));
    return dec_backward(h, p, p.y, a, d_v, 0.0, d_hv);
}

int pgl_decode_prepare_dev(pgl_handle h, const double* d_theta, const double* d_Weff)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_theta || !d_Weff) return fail(PGL_ERR_ARG, "null argument");
    PASS(dec_served(h));
    HIPCHK(hipSetDevice(h->device));
    const size_t tb = (size_t)h->N * (1 + (size_t)h->Dstim + h->Kimp) * 8, wb = (size_t)h->N * h->N * 8;
    ENSURE(h->gtheta, tb);
    ENSURE(h->Weff, wb);
    if (d_theta != h->gtheta.p) HIPCHK(hipMemcpyAsync(h->gtheta.p, d_theta, tb, hipMemcpyDeviceToDevice, h->stream));
    if (d_Weff != h->Weff.p) HIPCHK(hipMemcpyAsync(h->Weff.p, d_Weff, wb, hipMemcpyDeviceToDevice, h->stream));
    return enqueue_decode_prepare(h);
}

static int dec_eval_check(pgl_handle h, const void* u, int64_t Tu, int q, const pgl_decode_prior* prior, const void* F)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!u || !prior || !F) return fail(PGL_ERR_ARG, "null argument");
    if (Tu < 1 || q < 1) return fail(PGL_ERR_ARG, "stimulus decoding: Tu and q must be at least 1");
    if (!(prior->sigma > 0.0) || prior->mu != prior->mu || prior->rho != prior->rho)
        return fail(PGL_ERR_ARG, "stimulus decoding: the prior needs sigma > 0 and numbers for mu and rho");
    if (Tu > (1LL << 38) / std::max(h->dec_D, 1)) return fail(PGL_ERR_UNSUPPORTED, "stimulus too long for the decoding kernels");
    return dec_served(h);
}

int pgl_decode_eval_dev(pgl_handle h, const double* d_u, int64_t Tu, int q, const pgl_decode_prior* prior, double* d_F,
                        double* d_grad_u)
{
    PASS(dec_eval_check(h, d_u, Tu, q, prior, d_F));
    HIPCHK(hipSetDevice(h->device));
    const PglDecPrior pr = {prior->mu, prior->sigma, prior->rho};
    return enqueue_decode_eval(h, d_u, Tu, q, pr, d_F, d_grad_u);
}

int pgl_decode_hvp_dev(pgl_handle h, const double* d_v, double* d_hv)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!d_v || !d_hv) return fail(PGL_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return enqueue_decode_hvp(h, d_v, d_hv);
}

int pgl_decode_prepare(pgl_handle h, const double* theta, const double* Weff)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!theta || !Weff) return fail(PGL_ERR_ARG, "null argument");
    PASS(dec_served(h));
    HIPCHK(hipSetDevice(h->device));
    PASS(upload_draw(h, theta, Weff));
    return pgl_decode_prepare_dev(h, (const double*)h->gtheta.p, (const double*)h->Weff.p);
}

// D: the columns of the caller's arrays, which must be the stimulus dimensions of the handle -- the host forms move Tu * D doubles
static int dec_host_dims(const pgl_context* h, int D)
{
    if (D != h->dec_D)
        return fail(PGL_ERR_ARG, "stimulus decoding: the stimulus has " + std::to_string(D) + " columns, the handle's stimulus " +
                                     std::to_string(h->dec_D) + " dimensions");
    return PGL_OK;
}

int pgl_decode_eval(pgl_handle h, const double* u, int64_t Tu, int D, int q, const pgl_decode_prior* prior, double* F_out,
                    double* grad_u_out)
{
    PASS(dec_eval_check(h, u, Tu, q, prior, F_out));
    PASS(dec_host_dims(h, D));
    HIPCHK(hipSetDevice(h->device));
    const size_t ub = (size_t)Tu * h->dec_D * 8;
    PASS(stage_up(h, 0, u, ub));
    PASS(stage_up(h, 1, nullptr, PGL_DEC_NF * 8));
    PASS(stage_up(h, 2, nullptr, ub));
    PASS(pgl_decode_eval_dev(h, (const double*)h->stage[0].p, Tu, q, prior, (double*)h->stage[1].p,
                             grad_u_out ? (double*)h->stage[2].p : nullptr));
    PASS(stage_down(h, F_out, h->stage[1].p, PGL_DEC_NF * 8));
    PASS(stage_down(h, grad_u_out, h->stage[2].p, ub));
    return stage_end(h);
}

int pgl_decode_hvp(pgl_handle h, const double* v, int64_t Tu, int D, double* hv_out)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!v || !hv_out) return fail(PGL_ERR_ARG, "null argument");
    PASS(dec_served(h));
    if (!h->dec_ok || !h->dec_point) return fail(PGL_ERR_STATE, "pgl_decode_hvp before pgl_decode_eval");
    PASS(dec_host_dims(h, D));
    if (Tu != h->dec_Tu)
        return fail(PGL_ERR_ARG, "stimulus decoding: the direction has " + std::to_string(Tu) + " frames, the last evaluation had " +
                                     std::to_string(h->dec_Tu));
    HIPCHK(hipSetDevice(h->device));
    const size_t ub = (size_t)h->dec_Tu * h->dec_D * 8;
    PASS(stage_up(h, 0, v, ub));
    PASS(stage_up(h, 1, nullptr, ub));
    PASS(pgl_decode_hvp_dev(h, (const double*)h->stage[0].p, (double*)h->stage[1].p));
    PASS(stage_down(h, hv_out, h->stage[1].p, ub));
    return stage_end(h);
}

// the rule on the host (csrc/pglm_decode.h), no GPU: what tests/csrc/decode_host.c compiles with gcc
int pgl_decode_host(int N, int64_t nT, int nlin, double dt, const double* c, const double* S, const double* basis_t, int Rt, int B,
                    int D, const double* theta, int P, const double* u, int64_t Tu, int q, const pgl_decode_prior* prior,
                    const double* v, double* F_out, double* grad_u_out, double* hv_out)
{
    if (!c || !S || !basis_t || !theta || !u || !prior || !F_out) return fail(PGL_ERR_ARG, "null argument");
    if (N < 1 || nT < 1 || Rt < 1 || B < 1 || D < 1 || P < 1 + D * B || Tu < 1 || q < 1 || !(dt > 0) || !(prior->sigma > 0.0) ||
        (nlin != PGL_NLIN_EXP && nlin != PGL_NLIN_EXPLINEAR) || (v && !hv_out))
        return fail(PGL_ERR_ARG, "bad decoding problem");
    const PglDecPrior pr = {prior->mu, prior->sigma, prior->rho};
    std::vector<double> K((size_t)Rt * D * N), r((size_t)nT * N), cc((size_t)nT * N), s((size_t)nT * D), gs((size_t)nT * D);
    for (int tau = 0; tau < Rt; ++tau)
        for (int d = 0; d < D; ++d)
            for (int n = 0; n < N; ++n) K[((size_t)tau * D + d) * N + n] = pgl_dec_filter_at(basis_t, B, theta, P, tau, d, n);
    pgl_dec_eval_host(nT, N, nlin, dt, c, S, K.data(), Rt, D, u, Tu, q, &pr, F_out, grad_u_out, r.data(), cc.data(), s.data(),
                      gs.data());
    if (v) {
        std::vector<double> y((size_t)nT * N);
        pgl_dec_hvp_host(nT, N, cc.data(), K.data(), Rt, D, v, Tu, q, &pr, hv_out, s.data(), y.data(), gs.data());
    }
    return PGL_OK;
}

int pgl_state(pgl_handle h, int n, const double* theta_n, const double* Weff_col, double* lam_out,
              double* I_net_out, double* I_stim_out)
{
    int rc = pgl_gibbs_prepare(h, n, theta_n, Weff_col);
    if (rc) return rc;
    const size_t bytes = (size_t)h->nT * 8;
    if (lam_out) {
        ENSURE(h->lam, bytes);
        hipLaunchKernelGGL(k_lam, dim3(1024), dim3(256), 0, h->stream, (const double*)h->Inet.p,
                           (const double*)h->Istim.p, theta_n[0], h->nlin, (double*)h->lam.p,
                           (long long)h->nT);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(lam_out, h->lam.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (I_net_out) HIPCHK(hipMemcpyAsync(I_net_out, h->Inet.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (I_stim_out) HIPCHK(hipMemcpyAsync(I_stim_out, h->Istim.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGL_OK;
}

}  // extern "C"

#ifdef PGL_PROF
// dev builds only (tools/phase_profile.py): copy out the per-wave phase cycle sums of k_fused5 / 6 / 7
extern "C" int pgl_debug_prof(long long* out, int n_ll)
{
    const size_t bytes = std::min((size_t)n_ll * 8, sizeof(long long) * 2 * 4096 * 8 * 12);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pgl_prof), bytes, 0, hipMemcpyDeviceToHost));
    return PGL_OK;
}
extern "C" int pgl_debug_prof_ts(long long* out, int n_ll)
{
    const size_t bytes = std::min((size_t)n_ll * 8, sizeof(long long) * 4096 * 5);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pgl_prof_ts), bytes, 0, hipMemcpyDeviceToHost));
    return PGL_OK;
}
#endif
