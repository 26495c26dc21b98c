"""
ctypes binding of the C ABI declared in include/pyglm_hip.h (libpyglm_hip.so,
built from theano_pyglm_amd/csrc by __graft_entry__.build()).

There is NO CPU fallback: if the shared library is missing, or no HIP device is
visible, every compute entry point raises PglError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PYGLM_HIP_LIB', os.path.join(_HERE, 'libpyglm_hip.so'))   # env: dev A/B builds

NLIN_EXP = 0
NLIN_EXPLINEAR = 1
OPT_FEATURE_F32 = 1
OPT_NCHUNKS = 2
OPT_KERNEL = 3
OPT_GIBBS_KERNEL = 4
OPT_EPI_F64 = 5
OPT_TIMING = 6
OPT_BFGS_MERGE = 7
OPT_RECORD_KERNELS = 96             # dev / test: DeviceGlm.last_kernels() lists the fused launches of the last evaluation
RESCALE_CHUNK = 256                 # bins per chunk of the rescaling kernels (PGL_RS_CHUNK): chunks start at t_lo + k * 256

# every symbol include/pyglm_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    'pgl_last_error', 'pgl_version', 'pgl_device_count', 'pgl_create', 'pgl_destroy',
    'pgl_set_option', 'pgl_set_time_range', 'pgl_set_spikes_u8', 'pgl_set_spikes_f64', 'pgl_set_basis',
    'pgl_set_stim_features', 'pgl_set_stimulus', 'pgl_get_stim_features', 'pgl_ll_grad', 'pgl_ll_grad_dev', 'pgl_sync', 'pgl_features',
    'pgl_impulse_currents', 'pgl_state', 'pgl_ll_from_current', 'pgl_gibbs_prepare',
    'pgl_gibbs_ll', 'pgl_gibbs_update', 'pgl_last_timing', 'pgl_info', 'pgl_simulate', 'pgl_sta',
    'pgl_timing_summary', 'pgl_set_stream',
    'pgl_set_stimulus_separable', 'pgl_ll_grad_list_dev', 'pgl_gibbs_prepare_all', 'pgl_gibbs_ll_cols', 'pgl_gibbs_update_cols', 'pgl_gibbs_currents',
    'pgl_bfgs_state_doubles', 'pgl_bfgs_init_dev', 'pgl_bfgs_trial_dev', 'pgl_bfgs_objective_dev',
    'pgl_bfgs_linesearch_dev', 'pgl_bfgs_hmul_dev', 'pgl_bfgs_hmul_hist_dev', 'pgl_bfgs_update_dev', 'pgl_bfgs_step_dev', 'pgl_plan_kernels', 'pgl_last_kernels', 'pgl_gibbs_last_geometry', 'pgl_leading_singular_pairs', 'pgl_gemm_dev',
    'pgl_hvp_prepare_dev', 'pgl_hvp_prepare_list_dev', 'pgl_hvp_apply_dev', 'pgl_hvp',
    'pgl_ncg_state_doubles', 'pgl_ncg_init_dev', 'pgl_ncg_cg_step_dev', 'pgl_ncg_trial_dev', 'pgl_ncg_search_step_dev',
    'pgl_hmc_state_doubles', 'pgl_hmc_init_dev', 'pgl_hmc_begin_dev', 'pgl_hmc_leap_dev',
    'pgl_tri_matvec_dev', 'pgl_hmc_dense_begin_dev', 'pgl_hmc_dense_leap_dev',
    'pgl_nuts_state_doubles', 'pgl_nuts_init_dev', 'pgl_nuts_step_dev',
    'pgl_adapt_state_doubles', 'pgl_mass_adapt_dev', 'pgl_nuts_adapt_step_dev',
    'pgl_prox_state_doubles', 'pgl_prox_init_dev', 'pgl_prox_step_dev',
    'pgl_ais_state_doubles', 'pgl_ais_init_dev', 'pgl_ais_start_dev', 'pgl_ais_temper_dev', 'pgl_ais_begin_dev',
    'pgl_ais_leap_dev',
    'pgl_tri_matvec_shared_dev', 'pgl_ais_dense_begin_dev', 'pgl_ais_dense_leap_dev',
    'pgl_smc_state_doubles', 'pgl_smc_init_dev', 'pgl_smc_stage_dev', 'pgl_smc_gather_dev', 'pgl_smc_begin_dev', 'pgl_smc_leap_dev',
    'pgl_smc_dense_begin_dev', 'pgl_smc_dense_leap_dev',
    'pgl_hess_dev', 'pgl_hess',
    'pgl_chol_factor_dev', 'pgl_tri_inverse_dev', 'pgl_chol_solve_dev',
    'pgl_newton_state_doubles', 'pgl_newton_init_dev', 'pgl_newton_assemble_dev', 'pgl_newton_direction_dev',
    'pgl_newton_trial_dev', 'pgl_newton_search_step_dev',
    'pgl_rescale_count', 'pgl_rescale_dev', 'pgl_rescale',
    'pgl_rescale_corr_dev', 'pgl_rescale_corr', 'pgl_ks_uniform_dev', 'pgl_ks_uniform', 'pgl_rescale_acf_dev', 'pgl_rescale_acf',
    'pgl_pointwise_count', 'pgl_pointwise_dev', 'pgl_pointwise',
    'pgl_rate_windows_count', 'pgl_rate_windows_dev', 'pgl_rate_windows',
    'pgl_psis_loo_dev', 'pgl_psis_loo',
    'pgl_wald_groups_dev', 'pgl_wald_groups',
    'pgl_chain_diag_dev', 'pgl_chain_diag',
    'pgl_filter_bands_dev', 'pgl_filter_bands',
    'pgl_simulate_streams', 'pgl_simulate_batch', 'pgl_simulate_batch_dev', 'pgl_simulate_batch_plan',
    'pgl_simulate_cond_streams', 'pgl_cond_currents_dev', 'pgl_cond_currents', 'pgl_simulate_cond_workspace',
    'pgl_simulate_cond_dev', 'pgl_simulate_cond',
    'pgl_decode_prepare_dev', 'pgl_decode_eval_dev', 'pgl_decode_hvp_dev', 'pgl_decode_prepare', 'pgl_decode_eval', 'pgl_decode_hvp', 'pgl_decode_host',
]


ABI_VERSION = 119                   # PGL_ABI_VERSION of include/pyglm_hip.h: load() refuses a library that reports another

GEMM_NT, GEMM_MFMA_1, GEMM_MFMA_4, GEMM_KC_4_1_8, GEMM_KC_1_0_16 = range(5)   # PGL_GEMM_*: the kernel of pgl_gemm_dev

RW_NACC = 5                         # PGL_RW_NACC: planes of the rate-window accumulator -- mean, M2, min, max, pit
RW_MAX_COUNT = 1024                 # PGL_RW_MAX_COUNT: the largest observed window count with a pit (more: NaN)
RW_MAX_LAM = 700.0                  # the largest expected window count with a pit (more: NaN)
KS_NOUT = 4                         # PGL_KS_NOUT: columns of ks_uniform's result -- D, D+, D-, n
ACF_MAX_LAG = 64                    # PGL_ACF_MAX_LAG: the largest lag of rescale_acf
ACF_NHEAD = 6                       # PGL_ACF_NHEAD: n, mean, c_0, Q, dof, 0 in front of r_1 .. r_L (csrc/pglm_acf.h)
ACF_PIECE = 256                     # PGL_ACF_PIECE: the elements of a piece of its sums
KS_TILE = 4096                      # PGL_KS_TILE: the doubles of a tile of the KS sort (csrc/pglm_gof.h)
PSIS_NOUT = 4                       # PGL_PSIS_NOUT: planes of psis_loo's result -- elpd, khat, n_eff, tail length
PSIS_MAX_DRAWS = 4096               # PGL_PSIS_MAX_DRAWS: the draws a workgroup's LDS holds; more: PGL_ERR_UNSUPPORTED
WALD_MAX_B = 16                     # PGL_WALD_MAX_B: the largest coupling group wald_groups serves; more: PGL_ERR_UNSUPPORTED
WALD_NOUT = 4                       # PGL_WALD_NOUT: T, lin, var, info per group (csrc/pglm_wald.h)
DIAG_MAX_DRAWS = 4096               # PGL_DIAG_MAX_DRAWS: the pooled draws (chains x draws) chain_diag's workgroup holds
DIAG_ROWS = ('mean', 'sd', 'median', 'q025', 'q975', 'rhat_plain', 'rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean',
             'lag_bulk', 'lag_q05', 'lag_q95', 'lag_mean')          # the rows of chain_diag's result, in PGL_DIAG_* order
DIAG_NOUT = len(DIAG_ROWS)          # PGL_DIAG_NOUT
FILT_MAX_B = 16                     # PGL_FILT_MAX_B: the largest group of weights filter_bands serves
FILT_MAX_DRAWS = 4096               # PGL_FILT_MAX_DRAWS: the pooled draws filter_bands' workgroup sorts in LDS
FILT_LAG_COLS = ('mean', 'sd', 'q_lo', 'median', 'q_hi')            # the PGL_FILT_NLAG figures per lag (csrc/pglm_filters.h)
CS_NACC = 6                         # PGL_CS_NACC: planes of the clamped simulation's accumulator (csrc/pglm_condsim.h)
CS_PLANES = ('sum', 'sum_sq', 'n_less', 'n_equal', 'min', 'max')
CS_QUEUE = 32                       # PGL_CS_QUEUE: own spike bins a chain of k_simulate_cond keeps before it moves to a ring
CS_MAX_R = 4096                     # PGL_CS_MAX_R: taps of self-history simulate_cond serves; more: PGL_ERR_UNSUPPORTED
DEC_NF = 3                          # PGL_DEC_NF: F, log likelihood, log prior of decode_eval (csrc/pglm_decode.h)
OPT_DECODE_CUT = 89                 # PGL_OPT_DECODE_CUT: chunks / tiles a workgroup of the decoding kernels takes (same bits)
FILT_GRP_COLS = ('c_sim', 'weight_mean', 'weight_sd', 'weight_q_lo', 'weight_median', 'weight_q_hi', 'p_pos', 'info')   # PGL_FILT_NGRP


class PglError(RuntimeError):
    pass


class Prior(C.Structure):
    """pgl_prior of include/pyglm_hip.h."""
    _fields_ = [('kind', C.c_int), ('mu_b', C.c_double), ('sg_b', C.c_double), ('stim_sigma', C.c_double),
                ('mu', C.c_double), ('sigma', C.c_double), ('lam', C.c_double)]


class DecodePrior(C.Structure):
    """pgl_decode_prior of include/pyglm_hip.h: per stimulus dimension Gaussian with mean mu and precision I / sigma^2 +
    Dt^T Dt / rho^2 (Dt: first differences in time); rho = inf: iid."""
    _fields_ = [('mu', C.c_double), ('sigma', C.c_double), ('rho', C.c_double)]


def as_decode_prior(p):
    """A DecodePrior from a DecodePrior or from (mu, sigma, rho)."""
    if isinstance(p, DecodePrior):
        return p
    mu, sigma, rho = p
    return DecodePrior(float(mu), float(sigma), float(rho))


def as_prior(p):
    """A Prior from a Prior or from the tuple (kind, mu_b, sg_b, stim_sigma, mu, sigma, lam) of _Packing.prior_params()."""
    if isinstance(p, Prior):
        return p
    if len(p) != 7:
        raise ValueError("prior: (kind, mu_b, sg_b, stim_sigma, mu, sigma, lam)")
    return Prior(int(p[0]), *[float(z) for z in p[1:]])


def _prox_prior(p):
    """as_prior for the prox calls, which also take the five numbers (mu_b, sg_b, stim_sigma, mu, sigma) of the smooth part
    as the host mirror states them (tests/prox_mirror.py): the kind is 1 and lam is the calls' d_lam."""
    if not isinstance(p, Prior) and len(p) == 5:
        p = (1,) + tuple(p) + (0.0,)
    return as_prior(p)


def plan_kernels(N, B=5, R=200, Dstim=0, nT=300000, stim=0, n_lo=0, count=None, path=0, opt_kernel=0, opt_f32=0):
    """Names of the fused kernel instantiations the dispatcher would launch for this shape (pgl_plan_kernels: a dry run,
    works without a GPU); raises PglError where no plan exists."""
    lib = load()
    buf = C.create_string_buffer(4096)
    rc = lib.pgl_plan_kernels(int(N), int(B), int(R), int(Dstim), int(nT), int(stim), int(n_lo), int(N - n_lo if count is None else count),
                              int(path), int(opt_kernel), int(opt_f32), buf, 4096)
    if rc != 0:
        raise PglError(lib.pgl_last_error().decode())
    return [ln for ln in buf.value.decode().splitlines() if ln]


_lib = None


def _preload_torch_hip():
    """One HIP runtime per process.  PyTorch (used for device tensors / torch.distributed by
    bench.py, parallel.py and the GPU-resident optimizer) bundles its own libamdhip64 /
    libhsa-runtime64 with the same SONAMEs as the system ROCm ones this library links to.  If the
    system copies are mapped first, a later `import torch` resolves its HIP symbols against them
    and cannot initialise ("No HIP GPUs are available"); mapped in the other order everything
    works.  So when torch is installed its runtime is mapped before libpyglm_hip.so -- without
    importing torch."""
    if os.environ.get('PYGLM_NO_TORCH_PRELOAD'):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], 'lib')
        for name in ('libhsa-runtime64.so', 'libamdhip64.so'):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load libpyglm_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PglError("HIP library %s not found: run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback."
                       % LIB_PATH)
    _preload_torch_hip()
    lib = C.CDLL(LIB_PATH)
    lib.pgl_version.restype = C.c_int
    lib.pgl_version.argtypes = []
    if lib.pgl_version() != ABI_VERSION:                      # before any signature below is trusted
        raise PglError("HIP library %s has ABI version %d, this binding needs %d: rebuild it "
                       "(`python -c 'import __graft_entry__ as g; g.build()'`)" % (LIB_PATH, lib.pgl_version(), ABI_VERSION))
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    pr = C.POINTER(Prior)
    lib.pgl_last_error.restype = C.c_char_p
    lib.pgl_last_error.argtypes = []
    lib.pgl_device_count.restype = C.c_int
    lib.pgl_create.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                               C.POINTER(vp)]
    lib.pgl_destroy.argtypes = [vp]
    lib.pgl_set_option.argtypes = [vp, C.c_int, C.c_int]
    lib.pgl_set_time_range.argtypes = [vp, C.c_int64, C.c_int64]
    lib.pgl_set_spikes_u8.argtypes = [vp, vp]
    lib.pgl_set_spikes_f64.argtypes = [vp, vp]
    lib.pgl_set_basis.argtypes = [vp, vp]
    lib.pgl_set_stim_features.argtypes = [vp, vp, C.c_int]
    lib.pgl_set_stimulus.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int,
                                     C.c_int, C.c_int]
    lib.pgl_get_stim_features.argtypes = [vp, vp]
    lib.pgl_set_stimulus_separable.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int,
                                               C.c_int]
    lib.pgl_timing_summary.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.pgl_set_stream.argtypes = [vp, vp]
    lib.pgl_sta.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_double, C.c_int, vp, C.c_int, vp]
    lib.pgl_leading_singular_pairs.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_gemm_dev.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64,
                                 vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pgl_ll_grad.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_ll_grad_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_ll_grad_list_dev.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    lib.pgl_sync.argtypes = [vp]
    lib.pgl_hvp_prepare_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    lib.pgl_hvp_prepare_list_dev.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.pgl_hvp_apply_dev.argtypes = [vp, vp, vp]
    lib.pgl_hvp.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_hess_dev.argtypes = [vp, vp, C.c_int]
    lib.pgl_hess.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_chol_factor_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_tri_inverse_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.pgl_chol_solve_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_rescale_count.argtypes = [vp, vp]
    lib.pgl_rescale_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.pgl_rescale.argtypes = [vp, vp, vp, vp, vp]
    lib.pgl_rescale_corr_dev.argtypes = [vp, vp, vp, C.c_uint64, C.c_int64, vp, vp, vp]
    lib.pgl_rescale_corr.argtypes = [vp, vp, vp, C.c_uint64, C.c_int64, vp, vp]
    lib.pgl_ks_uniform_dev.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.pgl_ks_uniform.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.pgl_rescale_acf_dev.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int, vp, vp]
    lib.pgl_rescale_acf.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int, vp, vp]
    lib.pgl_pointwise_count.argtypes = [vp, C.c_int, vp]
    lib.pgl_pointwise_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int64]
    lib.pgl_pointwise.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.pgl_rate_windows_count.argtypes = [vp, C.c_int64, vp]
    lib.pgl_rate_windows_dev.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64]
    lib.pgl_rate_windows.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.pgl_psis_loo_dev.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp]
    lib.pgl_psis_loo.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp]
    lib.pgl_wald_groups_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_wald_groups.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.pgl_chain_diag_dev.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.pgl_chain_diag.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.pgl_filter_bands_dev.argtypes = lib.pgl_filter_bands.argtypes = \
        [vp, vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_double, vp, vp]
    # the lock-step methods; pr: const pgl_prior*
    lib.pgl_bfgs_state_doubles.argtypes = [C.c_int, C.c_int]
    lib.pgl_bfgs_init_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double]
    lib.pgl_bfgs_trial_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.pgl_bfgs_objective_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, pr]
    lib.pgl_bfgs_linesearch_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int]
    lib.pgl_bfgs_hmul_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int]
    lib.pgl_bfgs_update_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, C.c_int]
    lib.pgl_bfgs_hmul_hist_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]
    lib.pgl_bfgs_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, pr, C.c_int, C.c_double, C.c_int,
                                      C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.pgl_ncg_state_doubles.argtypes = [C.c_int, C.c_int]
    lib.pgl_ncg_init_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, pr, C.c_int, vp, vp]
    lib.pgl_ncg_cg_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, pr, vp, vp]
    lib.pgl_ncg_trial_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.pgl_ncg_search_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, pr, C.c_int, vp, vp, vp, vp]
    lib.pgl_newton_state_doubles.argtypes = [C.c_int, C.c_int]
    lib.pgl_newton_init_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, pr, C.c_double, C.c_int, vp]
    lib.pgl_newton_assemble_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, pr, vp]
    lib.pgl_newton_direction_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.pgl_newton_trial_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.pgl_newton_search_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, pr, C.c_double, C.c_int, vp,
                                               vp, vp]
    lib.pgl_hmc_state_doubles.argtypes = [C.c_int, C.c_int]
    lib.pgl_hmc_init_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, pr, C.c_double, C.c_uint64]
    lib.pgl_hmc_begin_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.pgl_hmc_leap_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, pr, C.c_int, C.c_int, vp, vp]
    lib.pgl_tri_matvec_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.pgl_hmc_dense_begin_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.pgl_hmc_dense_leap_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, pr, C.c_int, C.c_int, vp, vp]
    lib.pgl_nuts_state_doubles.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.pgl_nuts_init_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, pr, vp, vp, vp, C.c_uint64,
                                      C.c_int, C.c_int, C.c_int, vp]
    lib.pgl_nuts_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, pr, vp, vp, C.c_double, C.c_int, C.c_int,
                                      C.c_int, vp, vp, vp]
    lib.pgl_adapt_state_doubles.argtypes = [C.c_int, C.c_int]
    lib.pgl_mass_adapt_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_nuts_adapt_step_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, pr, vp, vp, vp, C.c_double, C.c_int,
                                            C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_ais_state_doubles.argtypes = [C.c_int, C.c_int]
    kmp = [vp, vp, C.c_int, C.c_int, C.c_int]
    lib.pgl_ais_init_dev.argtypes = kmp + [C.c_int, C.c_int, pr, C.c_double, C.c_uint64, vp]
    lib.pgl_ais_start_dev.argtypes = kmp + [vp, vp, pr]
    lib.pgl_ais_temper_dev.argtypes = kmp + [pr, C.c_double, vp]
    lib.pgl_ais_begin_dev.argtypes = kmp + [vp, vp]
    lib.pgl_ais_leap_dev.argtypes = kmp + [vp, vp, vp, pr, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_tri_matvec_shared_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.pgl_ais_dense_begin_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.pgl_ais_dense_leap_dev.argtypes = kmp + [vp, vp, vp, pr, C.c_int, C.c_int, vp, vp, vp]
    lib.pgl_smc_state_doubles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    smc = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pgl_smc_init_dev.argtypes = smc + [C.c_int, pr, C.c_double, C.c_uint64, vp]
    lib.pgl_smc_stage_dev.argtypes = smc + [pr, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint64]
    lib.pgl_smc_gather_dev.argtypes = smc + [pr]
    lib.pgl_smc_begin_dev.argtypes = smc + [vp, vp]
    lib.pgl_smc_leap_dev.argtypes = smc + [vp, vp, vp, pr, C.c_int, vp]
    lib.pgl_smc_dense_begin_dev.argtypes = smc + [vp, vp]
    lib.pgl_smc_dense_leap_dev.argtypes = smc + [vp, vp, vp, pr, C.c_int, vp]
    lib.pgl_prox_state_doubles.argtypes = [C.c_int, C.c_int]
    prox = [vp, vp, C.c_int, C.c_int, vp, vp, pr, vp, C.c_double, C.c_int]
    lib.pgl_prox_init_dev.argtypes = prox + [vp, vp]
    lib.pgl_prox_step_dev.argtypes = prox + [C.c_int, vp, vp]
    lib.pgl_features.argtypes = [vp, vp]
    lib.pgl_impulse_currents.argtypes = [vp, vp, vp]
    lib.pgl_state.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.pgl_ll_from_current.argtypes = [vp, C.c_int, C.c_double, vp, vp, vp, vp, C.c_int, vp]
    lib.pgl_gibbs_prepare.argtypes = [vp, C.c_int, vp, vp]
    lib.pgl_gibbs_ll.argtypes = [vp, C.c_int, C.c_double, vp, C.c_int, vp]
    lib.pgl_gibbs_update.argtypes = [vp, C.c_int, C.c_double]
    lib.pgl_gibbs_prepare_all.argtypes = [vp, vp, vp]
    lib.pgl_gibbs_ll_cols.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.pgl_gibbs_update_cols.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.pgl_gibbs_currents.argtypes = [vp, C.c_int, vp]
    lib.pgl_last_timing.argtypes = [vp, dp, dp]
    lib.pgl_info.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
    lib.pgl_plan_kernels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.pgl_last_kernels.argtypes = [vp, C.c_char_p, C.c_int]
    lib.pgl_gibbs_last_geometry.argtypes = [vp, vp, C.c_int]
    lib.pgl_simulate.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, vp, vp, vp,
                                 C.c_int64, C.c_uint64, vp, vp]
    lib.pgl_simulate_streams.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, vp, vp, C.c_int, C.c_uint64,
                                         vp, vp, vp]
    sim = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_int,
           vp, vp, vp, vp]
    lib.pgl_simulate_batch.argtypes = sim
    lib.pgl_simulate_batch_dev.argtypes = sim + [vp, vp]
    lib.pgl_simulate_batch_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.pgl_simulate_cond_streams.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, vp, vp, C.c_int, C.c_uint64,
                                              vp, vp, vp]
    lib.pgl_cond_currents_dev.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.pgl_cond_currents.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.pgl_simulate_cond_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    cond = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_uint64,
            C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.pgl_simulate_cond.argtypes = cond
    lib.pgl_simulate_cond_dev.argtypes = cond + [vp, vp]
    dpr = C.POINTER(DecodePrior)
    lib.pgl_decode_prepare_dev.argtypes = [vp, vp, vp]
    lib.pgl_decode_eval_dev.argtypes = [vp, vp, C.c_int64, C.c_int, dpr, vp, vp]
    lib.pgl_decode_hvp_dev.argtypes = [vp, vp, vp]
    lib.pgl_decode_prepare.argtypes = [vp, vp, vp]
    lib.pgl_decode_eval.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, dpr, vp, vp]
    lib.pgl_decode_hvp.argtypes = [vp, vp, C.c_int64, C.c_int, vp]
    lib.pgl_decode_host.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_double, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp,
                                    C.c_int64, C.c_int, dpr, vp, vp, vp, vp]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name in ('pgl_bfgs_state_doubles', 'pgl_ncg_state_doubles', 'pgl_newton_state_doubles', 'pgl_hmc_state_doubles',
                    'pgl_ais_state_doubles', 'pgl_prox_state_doubles', 'pgl_nuts_state_doubles', 'pgl_adapt_state_doubles', 'pgl_smc_state_doubles',
                    'pgl_simulate_cond_workspace'):
            fn.restype = C.c_longlong
        elif name not in ('pgl_last_error',):
            fn.restype = C.c_int
    _lib = lib
    return lib


def device_count():
    return load().pgl_device_count()


def _chk(rc):
    if rc != 0:
        raise PglError("libpyglm_hip error %d: %s" % (rc, load().pgl_last_error().decode()))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(x):
    """The device address every _dev method hands to the library: an integer (torch.Tensor.data_ptr(), say) or an object
    with data_ptr() -- a torch tensor; None and 0 are NULL."""
    if hasattr(x, 'data_ptr'):
        x = x.data_ptr()
    return C.c_void_p(x) if x else None


def _dev_tensor(t, dtype, msg, ndim=None, min_ndim=0, numel=0, shape=None, strides=None, contiguous=True):
    """t where it is a torch device tensor of this dtype ('float64', 'int64') with exactly `ndim` / at least `min_ndim` axes,
    at least `numel` elements and exactly `shape` and `strides`, as far as each is given; ValueError(msg) where not."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and
            (ndim is None or t.dim() == ndim) and t.dim() >= min_ndim and t.numel() >= numel and
            (shape is None or tuple(t.shape) == tuple(shape)) and (strides is None or t.stride() == tuple(strides)) and
            (not contiguous or t.is_contiguous())):
        raise ValueError(msg)
    return t


def _out_tensor(out, shape, like, msg):
    """The result tensor of a tensor form: a new float64 tensor of this shape on `like`'s device, or the caller's `out`
    where it is a contiguous one of that shape."""
    if out is None:
        import torch
        return torch.empty(shape, dtype=torch.float64, device=like.device)
    return _dev_tensor(out, 'float64', msg, shape=shape)


def _second_out(want, fresh, check, none_is_fresh=False):
    """The optional second output of a tensor form: True -> fresh(), which the form returns beside the first; a tensor ->
    check(tensor), written into; False -> none.  None is none as well (ks_uniform: the handle sorts in a buffer of its own),
    or with none_is_fresh a fresh tensor that is not returned (rescale_acf, whose kernel always writes the scores)."""
    if want is True or (want is None and none_is_fresh):
        return fresh()
    if want is None or (want is False and not none_is_fresh):
        return None
    return check(want)


def simulate(X0, AW, nlin, dt, uniforms=None, seed=0):
    """Native Population.simulate (population.py:233-389); host code, needs no GPU.
    X0 (nT,N) background current, AW (N,R,N) [n_pre][tau][n_post].  Returns (S, X, n_exceptions)."""
    lib = load()
    X = np.array(X0, dtype=np.float64, order='C')
    nT, N = X.shape
    AW = _f64(AW)
    assert AW.ndim == 3 and AW.shape[0] == N and AW.shape[2] == N
    R = AW.shape[1]
    S = np.empty((nT, N))
    u = None if uniforms is None else _f64(uniforms)
    nexc = C.c_int64(0)
    kind = {'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin)
    _chk(lib.pgl_simulate(N, nT, R, int(kind), float(dt), _ptr(X), _ptr(AW), _ptr(u),
                          0 if u is None else u.size, int(seed), _ptr(S), C.byref(nexc)))
    return S, X, int(nexc.value)


def _sim_args(X0, AW, nlin):
    X0 = _f64(X0)
    AW = _f64(AW)
    if X0.ndim != 2 or AW.ndim != 3 or AW.shape[0] != X0.shape[1] or AW.shape[2] != X0.shape[1]:
        raise ValueError("X0 must be (nT, N) and AW (N, R, N) [n_pre][tau][n_post]")
    return X0, AW, int({'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin))


def simulate_streams(X0, AW, nlin, dt, rep=0, seed=0):
    """Host reference of one replicate on the per-neuron threshold streams (pgl_simulate_streams; needs no GPU).
    X0 (nT, N), AW (N, R, N) as in simulate.  Returns (S uint8 (nT, N), X (nT, N), n_exceptions, closest_call)."""
    lib = load()
    X0, AW, kind = _sim_args(X0, AW, nlin)
    X = X0.copy()
    nT, N = X.shape
    S = np.empty((nT, N), dtype=np.uint8)
    nexc = C.c_int64(0)
    closest = C.c_double(0.0)
    _chk(lib.pgl_simulate_streams(N, nT, AW.shape[1], kind, float(dt), _ptr(X), _ptr(AW), int(rep), int(seed), _ptr(S),
                                  C.byref(nexc), C.byref(closest)))
    return S, X, int(nexc.value), float(closest.value)


def simulate_batch_plan(N, R, flags=0):
    """(ring_in_lds, workspace_bytes_per_rep) of pgl_simulate_batch for this shape: a dry run, needs no GPU."""
    lds, ws = C.c_int(0), C.c_longlong(0)
    _chk(load().pgl_simulate_batch_plan(int(N), int(R), int(flags), C.byref(lds), C.byref(ws)))
    return bool(lds.value), int(ws.value)


def simulate_batch(X0, AW, nlin, dt, n_rep, seed=0, rep0=0, flags=0, spikes=True, currents=False, device=0):
    """n_rep replicates on the device (pgl_simulate_batch), stream indices rep0 .. rep0 + n_rep - 1.  Returns a dict:
    S (n_rep, nT, N) uint8 or None, X (n_rep, nT, N) total currents or None, counts (n_rep, N), exceptions (n_rep)."""
    lib = load()
    X0, AW, kind = _sim_args(X0, AW, nlin)
    nT, N = X0.shape
    n_rep = int(n_rep)
    S = np.empty((n_rep, nT, N), dtype=np.uint8) if spikes else None
    X = np.empty((n_rep, nT, N)) if currents else None
    counts = np.empty((n_rep, N), dtype=np.int64)
    exc = np.empty(n_rep, dtype=np.int64)
    _chk(lib.pgl_simulate_batch(int(device), N, nT, AW.shape[1], kind, float(dt), _ptr(X0), _ptr(AW), n_rep, int(rep0),
                                int(seed), int(flags), _ptr(S), _ptr(X), _ptr(counts), _ptr(exc)))
    return {'S': S, 'X': X, 'counts': counts, 'exceptions': exc}


def simulate_batch_dev(N, nT, R, nlin, dt, d_X0, d_AW, n_rep, d_counts, d_exceptions, seed=0, rep0=0, flags=0, d_S=0, d_X=0,
                       d_workspace=0, stream=0, device=0):
    """Device-pointer form (integers, e.g. torch.Tensor.data_ptr(); asynchronous on `stream`, 0 = the null stream);
    d_S / d_X = 0: counts and exceptions alone; see pgl_simulate_batch_dev."""
    kind = int({'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin))
    _chk(load().pgl_simulate_batch_dev(int(device), int(N), int(nT), int(R), kind, float(dt), _dp(d_X0), _dp(d_AW),
                                       int(n_rep), int(rep0), int(seed), int(flags), _dp(d_S), _dp(d_X), _dp(d_counts),
                                       _dp(d_exceptions), _dp(d_workspace), _dp(stream)))


def spike_events(S):
    """The event lists of recorded spikes S (nT, N) as the clamped simulation takes them: (ev_pre (E) int32, ev_cnt (E) uint8,
    bin_off (nT + 1) int64), sorted by (bin, pre).  Counts above 255 in a bin are refused."""
    S = np.asarray(S)
    if S.ndim != 2 or np.any(S < 0) or np.any(S > 255) or np.any(S != np.floor(S)):
        raise ValueError("S must be (nT, N) integer counts in 0 .. 255")
    t, pre = np.nonzero(S)                                    # row-major: sorted by (bin, pre)
    bin_off = np.zeros(S.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(t, minlength=S.shape[0]), out=bin_off[1:])
    return pre.astype(np.int32), S[t, pre].astype(np.uint8), bin_off


def window_counts(S, win):
    """(n_win, N) int64 counts of S (nT, N) over windows of `win` bins from bin 0 (the last one may be short)."""
    S = np.asarray(S)
    return np.add.reduceat(S.astype(np.int64), np.arange(0, S.shape[0], int(win)), axis=0)


def simulate_cond_streams(Xc, AW, nlin, dt, rep=0, seed=0):
    """Host reference of one replicate of the clamped simulation (pgl_simulate_cond_streams; needs no GPU).  Xc (nT, N) clamped
    currents, AW (N, R, N) of which only [n, :, n] is read.  Returns (S uint8 (nT, N), exceptions (N) int64, closest_call)."""
    lib = load()
    Xc, AW, kind = _sim_args(Xc, AW, nlin)
    nT, N = Xc.shape
    S = np.empty((nT, N), dtype=np.uint8)
    exc = np.zeros(N, dtype=np.int64)
    closest = C.c_double(0.0)
    _chk(lib.pgl_simulate_cond_streams(N, nT, AW.shape[1], kind, float(dt), _ptr(Xc), _ptr(AW), int(rep), int(seed), _ptr(S),
                                       _ptr(exc), C.byref(closest)))
    return S, exc, float(closest.value)


def cond_currents(X0, AW, ev_pre, ev_cnt, bin_off, device=0):
    """Xc (nT, N) on the device from host arrays (pgl_cond_currents); the events as spike_events gives them."""
    X0, AW, _ = _sim_args(X0, AW, 0)
    nT, N = X0.shape
    ev_pre = np.ascontiguousarray(ev_pre, dtype=np.int32)
    ev_cnt = np.ascontiguousarray(ev_cnt, dtype=np.uint8)
    bin_off = np.ascontiguousarray(bin_off, dtype=np.int64)
    if bin_off.shape != (nT + 1,) or ev_pre.shape != ev_cnt.shape or ev_pre.ndim != 1 or ev_pre.size != bin_off[-1]:
        raise ValueError("bin_off must be (nT + 1) and ev_pre / ev_cnt (bin_off[nT])")
    Xc = np.empty((nT, N))
    _chk(load().pgl_cond_currents(int(device), N, nT, AW.shape[1], _ptr(X0), _ptr(AW), _ptr(ev_pre), _ptr(ev_cnt),
                                  _ptr(bin_off), _ptr(Xc)))
    return Xc


def cond_currents_dev(N, nT, R, d_X0, d_AW, d_ev_pre, d_ev_cnt, d_bin_off, d_Xc, stream=0, device=0):
    _chk(load().pgl_cond_currents_dev(int(device), int(N), int(nT), int(R), _dp(d_X0), _dp(d_AW), _dp(d_ev_pre), _dp(d_ev_cnt),
                                      _dp(d_bin_off), _dp(d_Xc), _dp(stream)))


def simulate_cond_workspace(N, R, n_rep):
    """bytes of d_workspace of simulate_cond_dev: the fallback rings, N R n_rep doubles"""
    return int(load().pgl_simulate_cond_workspace(int(N), int(R), int(n_rep)))


def simulate_cond(Xc, AW, nlin, dt, obs, win, n_rep, seed=0, rep0=0, flags=0, acc=None, exceptions=None, fallbacks=None,
                  counts=False, spikes=False, device=0):
    """n_rep clamped replicates on the device from host arrays (pgl_simulate_cond), stream indices rep0 .. rep0 + n_rep - 1.
    obs (n_win, N) recorded window counts.  acc / exceptions / fallbacks of an earlier call continue it (all three, or none).
    Returns a dict: acc (6, n_win, N) int64, exceptions (N), fallbacks (int), counts (n_rep, N) or None, S (n_rep, nT, N) uint8
    or None."""
    Xc, AW, kind = _sim_args(Xc, AW, nlin)
    nT, N = Xc.shape
    n_rep, win = int(n_rep), int(win)
    n_win = -(-nT // win) if win > 0 else 0
    obs = np.ascontiguousarray(obs, dtype=np.int64)
    if obs.shape != (n_win, N):
        raise ValueError("obs must be (n_win, N) = %s" % ((n_win, N),))
    cont = acc is not None
    acc = np.array(acc, dtype=np.int64, order='C') if cont else np.empty((CS_NACC, n_win, N), dtype=np.int64)
    if acc.shape != (CS_NACC, n_win, N):
        raise ValueError("acc must be (6, n_win, N)")
    exc = np.array(exceptions, dtype=np.int64, order='C') if cont else np.empty(N, dtype=np.int64)
    fb = np.array([fallbacks if cont else 0], dtype=np.int64)
    cnt = np.empty((max(n_rep, 0), N), dtype=np.int64) if counts else None
    S = np.empty((max(n_rep, 0), nT, N), dtype=np.uint8) if spikes else None
    _chk(load().pgl_simulate_cond(int(device), N, nT, AW.shape[1], kind, float(dt), _ptr(Xc), _ptr(AW), _ptr(obs), win, n_rep,
                                  int(rep0), int(seed), int(flags), int(cont), _ptr(acc), _ptr(exc), _ptr(cnt), _ptr(S), _ptr(fb)))
    return {'acc': acc, 'exceptions': exc, 'fallbacks': int(fb[0]), 'counts': cnt, 'S': S}


def simulate_cond_dev(N, nT, R, nlin, dt, d_Xc, d_AW, d_obs, win, n_rep, d_acc, d_exceptions, d_workspace, seed=0, rep0=0,
                      flags=0, accumulate=False, d_counts=0, d_S=0, d_fallbacks=0, stream=0, device=0):
    """Device-pointer form (pgl_simulate_cond_dev; asynchronous on `stream`, 0 = the null stream)."""
    kind = int({'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin))
    _chk(load().pgl_simulate_cond_dev(int(device), int(N), int(nT), int(R), kind, float(dt), _dp(d_Xc), _dp(d_AW), _dp(d_obs),
                                      int(win), int(n_rep), int(rep0), int(seed), int(flags), int(bool(accumulate)), _dp(d_acc),
                                      _dp(d_exceptions), _dp(d_counts), _dp(d_S), _dp(d_fallbacks), _dp(d_workspace),
                                      _dp(stream)))


def decode_host(c, S, basis_t, D, theta, nlin, dt, u, q, prior, v=None, want_grad=True):
    """The decoding rule on the host (pgl_decode_host: plain C, no GPU): c, S (nT, N), basis_t (Rt, B), theta (N, P) with the
    stimulus weights in columns 1 .. D B, u (Tu, D), prior (mu, sigma, rho) -> (F (3,): F, log likelihood, log prior; grad
    (Tu, D) or None; H v (Tu, D) where v is given, else None)."""
    c = _f64(c)
    nT, N = c.shape
    S = _f64(S, (nT, N))
    bt = _f64(basis_t)
    th = _f64(theta)
    u = _f64(u)
    if u.ndim != 2 or u.shape[1] != D:
        raise ValueError("u must be (Tu, D)")
    vv = None if v is None else _f64(v, u.shape)
    F = np.empty(DEC_NF)
    g = np.empty(u.shape) if want_grad else None
    hv = None if v is None else np.empty(u.shape)
    pr = as_decode_prior(prior)
    _chk(load().pgl_decode_host(N, nT, int({'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin)), float(dt), _ptr(c),
                                _ptr(S), _ptr(bt), bt.shape[0], bt.shape[1], int(D), _ptr(th), th.shape[1], _ptr(u), u.shape[0],
                                int(q), C.byref(pr), _ptr(vv), _ptr(F), _ptr(g), _ptr(hv)))
    return F, g, hv


class DeviceGlm(object):
    """One pgl_handle: the device-resident data of one data sequence
    (the Theano shared variables S / ir / stim of glm.py:17-18, impulse.py:41-42,
    bkgd.py:70-71) plus the kernels that evaluate glm.ll and its gradient on it.  Where a *_dev method's docstring
    says "device pointer" or "integer", a torch device tensor serves as well (_dp)."""

    def __init__(self, N, nT, B, R, nlin, dt, device=0):
        self.lib = load()
        self.N, self.nT, self.B, self.R, self.dt = int(N), int(nT), int(B), int(R), float(dt)
        self.nlin = {'exp': NLIN_EXP, 'explinear': NLIN_EXPLINEAR}.get(nlin, nlin)
        self.Dstim = 0
        self.dec_D = None                  # stimulus dimensions of a 'basis' stimulus (set_stimulus): what decode_* serves
        h = C.c_void_p()
        _chk(self.lib.pgl_create(self.N, self.nT, self.B, self.R, int(self.nlin), self.dt,
                                 int(device), C.byref(h)))
        self.h = h

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, 'h', None) is not None and self.h.value:
            self.lib.pgl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def P(self):
        return 1 + self.Dstim + self.N * self.B

    # -- data ---------------------------------------------------------------
    def set_option(self, opt, value):
        _chk(self.lib.pgl_set_option(self.h, int(opt), int(value)))

    def set_time_range(self, t_lo, t_hi):
        """Evaluate only bins [t_lo, t_hi) (partial ll / gradient; t_lo multiple of 16)."""
        _chk(self.lib.pgl_set_time_range(self.h, int(t_lo), int(t_hi)))

    def set_spikes(self, S):
        S = np.asarray(S)
        if S.shape != (self.nT, self.N):
            raise ValueError("S must be (nT,N)=(%d,%d), got %s" % (self.nT, self.N, S.shape))
        if S.dtype == np.uint8:
            S = np.ascontiguousarray(S)
            _chk(self.lib.pgl_set_spikes_u8(self.h, _ptr(S)))
        else:
            S = _f64(S)
            _chk(self.lib.pgl_set_spikes_f64(self.h, _ptr(S)))

    def set_basis(self, ibasis):
        ib = _f64(ibasis, (self.R, self.B))
        _chk(self.lib.pgl_set_basis(self.h, _ptr(ib)))

    def set_stim_features(self, fstim):
        if fstim is None:
            _chk(self.lib.pgl_set_stim_features(self.h, None, 0))
            self.Dstim = 0
            self.dec_D = None
            return
        f = _f64(fstim)
        if f.ndim != 2 or f.shape[0] != self.nT:
            raise ValueError("fstim must be (nT,Dstim)")
        _chk(self.lib.pgl_set_stim_features(self.h, _ptr(f), int(f.shape[1])))
        self.Dstim = int(f.shape[1])
        self.dec_D = None

    def set_stimulus(self, stim, dt_stim, basis_t, basis_x=None, layout=0):
        """Build the dense stimulus feature columns on the device from the raw stimulus
        (interp -> spatial projection -> causal temporal filtering); see pgl_set_stimulus."""
        stim = _f64(stim)
        if stim.ndim != 2:
            raise ValueError("stim must be (Tstim, D)")
        bt = _f64(basis_t)
        bx = None if basis_x is None else _f64(basis_x, (stim.shape[1], np.shape(basis_x)[1]))
        Bx = stim.shape[1] if bx is None else bx.shape[1]
        _chk(self.lib.pgl_set_stimulus(self.h, _ptr(stim), stim.shape[0], stim.shape[1], float(dt_stim),
                                       _ptr(bx), int(Bx), _ptr(bt), bt.shape[0], bt.shape[1],
                                       int(layout)))
        self.Dstim = int(Bx * bt.shape[1])
        self.dec_D = int(stim.shape[1]) if bx is None and int(layout) == 1 else None

    def set_stimulus_separable(self, stim, dt_stim, basis_t, basis_x=None):
        """Rank-1 (w_t (x) w_x) stimulus kept separable on the device; theta rows become
        [bias, w_t, w_x, w_imp] (see pgl_set_stimulus_separable)."""
        stim = _f64(stim)
        if stim.ndim != 2:
            raise ValueError("stim must be (Tstim, D)")
        bt = _f64(basis_t)
        bx = None if basis_x is None else _f64(basis_x, (stim.shape[1], np.shape(basis_x)[1]))
        Bx = stim.shape[1] if bx is None else bx.shape[1]
        _chk(self.lib.pgl_set_stimulus_separable(self.h, _ptr(stim), stim.shape[0], stim.shape[1],
                                                 float(dt_stim), _ptr(bx), int(Bx), _ptr(bt), bt.shape[0],
                                                 bt.shape[1]))
        self.Dstim = int(Bx + bt.shape[1])
        self.dec_D = None

    def get_stim_features(self):
        out = np.empty((self.nT, self.Dstim))
        _chk(self.lib.pgl_get_stim_features(self.h, _ptr(out)))
        return out

    def sta(self, stim, dt_stim, L, Ns=None, keep_on_device=False):
        """Spike-triggered average (n_sel, L, D) of the resident spikes; see pgl_sta.  keep_on_device: the averages stay
        on the device for leading_singular_pairs(None, shape) and the shape (n_sel, L, D) is returned instead."""
        stim = _f64(stim)
        if stim.ndim != 2:
            raise ValueError("stim must be (Tstim, D)")
        sel = None if Ns is None else np.ascontiguousarray(np.atleast_1d(Ns), dtype=np.int32)
        nsel = self.N if sel is None else int(sel.size)
        out = None if keep_on_device else np.empty((nsel, int(L), stim.shape[1]))
        _chk(self.lib.pgl_sta(self.h, _ptr(stim), stim.shape[0], stim.shape[1], float(dt_stim), int(L),
                              _ptr(sel), nsel, _ptr(out)))
        return (nsel, int(L), int(stim.shape[1])) if keep_on_device else out

    def leading_singular_pairs(self, A, shape=None):
        """(U (n, L), sigma (n,), V (n, D)): leading singular pair of every matrix of the batch A (n, L, D); see
        pgl_leading_singular_pairs."""
        if A is None:                                      # the averages sta(keep_on_device=True) left on the device
            n, L, D = shape
        else:
            A = _f64(A)
            if A.ndim != 3:
                raise ValueError("A must be (n, L, D)")
            n, L, D = A.shape
        U, sig, V = np.empty((n, L)), np.empty(n), np.empty((n, D))
        _chk(self.lib.pgl_leading_singular_pairs(self.h, _ptr(A), n, L, D, _ptr(U), _ptr(sig), _ptr(V)))
        return U, sig, V

    def gemm_dev(self, kernel, A, sa, B, sb, Cm, sc, M, N, K, batch=1):
        """One thin GEMM on device operands (pgl_gemm_dev): C[b][m scm + n scn] = sum_k A[b][m sam + k sak] B[b][n sbn + k sbk].
        kernel: GEMM_NT, GEMM_MFMA_1, GEMM_MFMA_4, GEMM_KC_4_1_8 or GEMM_KC_1_0_16.  A, B, Cm: device addresses (int) of the
        first element; sa = (sam, sak, sAb), sb = (sbn, sbk, sBb), sc = (scm, scn, sCb), in doubles.  Asynchronous on the
        handle's stream; PglError where the kernel's preconditions do not hold (nothing is launched then)."""
        _chk(self.lib.pgl_gemm_dev(self.h, int(kernel), _dp(A), int(sa[0]), int(sa[1]), int(sa[2]), _dp(B), int(sb[0]),
                                   int(sb[1]), int(sb[2]), _dp(Cm), int(sc[0]), int(sc[1]), int(sc[2]), int(M), int(N),
                                   int(K), int(batch)))

    def _draw(self, theta, Weff, rows=None):
        """Host theta (rows, P) -- rows: every neuron's unless given -- and Weff (N, N) as contiguous float64 arrays."""
        return _f64(theta, (self.N if rows is None else rows, self.P)), _f64(Weff, (self.N, self.N))

    # -- hot path -------------------------------------------------------------
    def ll_grad(self, theta, Weff, n_lo=0, n_hi=None, want_grad=True):
        n_hi = self.N if n_hi is None else n_hi
        npost = n_hi - n_lo
        th, We = self._draw(theta, Weff, npost)
        ll = np.empty(npost)
        g = np.empty((npost, self.P)) if want_grad else None
        _chk(self.lib.pgl_ll_grad(self.h, int(n_lo), int(n_hi), _ptr(th), _ptr(We), _ptr(ll),
                                  _ptr(g)))
        return ll, g

    def ll_grad_dev(self, d_theta, d_Weff, d_ll, d_grad, n_lo=0, n_hi=None):
        """Device-pointer form (integers, e.g. torch.Tensor.data_ptr()); asynchronous."""
        n_hi = self.N if n_hi is None else n_hi
        _chk(self.lib.pgl_ll_grad_dev(self.h, int(n_lo), int(n_hi), _dp(d_theta), _dp(d_Weff), _dp(d_ll), _dp(d_grad)))

    def ll_grad_list_dev(self, d_idx, count, d_theta, d_Weff, d_ll, d_grad):
        """ll+grad of the `count` neurons listed in d_idx (device int32 pointer); row j of the device
        arrays belongs to neuron d_idx[j].  Asynchronous like ll_grad_dev."""
        _chk(self.lib.pgl_ll_grad_list_dev(self.h, _dp(d_idx), int(count), _dp(d_theta), _dp(d_Weff), _dp(d_ll),
                                           _dp(d_grad)))

    # -- Hessian-vector products of ll (grads.py:68-95 hessian_rop_wrt_list) -------
    def hvp_prepare(self, d_theta, d_Weff, n_lo=0, n_hi=None, d_idx=0, count=None):
        """Curvature pass at theta (device pointers as integers; asynchronous): rows [n_lo, n_hi), or the `count` neurons
        listed in d_idx (device int32 pointer).  The curvature stays on the device for hvp_apply."""
        if d_idx:
            _chk(self.lib.pgl_hvp_prepare_list_dev(self.h, _dp(d_idx), int(count), _dp(d_theta), _dp(d_Weff)))
            return
        n_hi = self.N if n_hi is None else n_hi
        _chk(self.lib.pgl_hvp_prepare_dev(self.h, int(n_lo), int(n_hi), _dp(d_theta), _dp(d_Weff)))

    def hvp_apply(self, d_v, d_hv):
        """d_hv = H . d_v for the prepared rows, (rows, P) each, theta layout (device pointers; asynchronous)."""
        _chk(self.lib.pgl_hvp_apply_dev(self.h, _dp(d_v), _dp(d_hv)))

    def hvp(self, theta, v, Weff, n_lo=0, n_hi=None):
        """H . v of ll for rows [n_lo, n_hi) with host arrays: theta, v (rows, P), Weff (N, N) -> (rows, P).  Repeated
        calls with the same theta / Weff / range (a CG solve) reuse the curvature on the device."""
        n_hi = self.N if n_hi is None else n_hi
        npost = n_hi - n_lo
        th, We = self._draw(theta, Weff, npost)
        vv = _f64(v, (npost, self.P))
        out = np.empty((npost, self.P))
        _chk(self.lib.pgl_hvp(self.h, int(n_lo), int(n_hi), _ptr(th), _ptr(vv), _ptr(We), _ptr(out)))
        return out

    # -- dense Hessians of ll (grads.py:30-66 hessian_wrt_list) ---------------------
    def hess(self, d_H, ld=None):
        """d_H (rows, P, ld) = the Hessian of ll of every row of the last hvp_prepare, theta layout, both triangles (device
        pointer; asynchronous).  ld >= P, default P; the padding columns are not written."""
        _chk(self.lib.pgl_hess_dev(self.h, _dp(d_H), int(self.P if ld is None else ld)))

    def hessian(self, theta, Weff, n_lo=0, n_hi=None):
        """Hessian of ll for rows [n_lo, n_hi) with host arrays: theta (rows, P), Weff (N, N) -> (rows, P, P)."""
        n_hi = self.N if n_hi is None else n_hi
        npost = n_hi - n_lo
        th, We = self._draw(theta, Weff, npost)
        out = np.empty((npost, self.P, self.P))
        _chk(self.lib.pgl_hess(self.h, int(n_lo), int(n_hi), _ptr(th), _ptr(We), _ptr(out)))
        return out

    # -- batched dense factorisation for the Laplace posterior (pgl_chol_factor_dev / pgl_tri_inverse_dev) --------
    @staticmethod
    def _stack(A, name):
        import torch
        if not (isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 and A.dim() == 3 and
                A.is_contiguous() and A.shape[0] > 0 and 0 < A.shape[1] <= A.shape[2]):
            raise ValueError("%s: a contiguous float64 device tensor (M, P, ld), ld >= P" % name)
        return torch

    def chol_factor(self, A):
        """In place on the torch device tensor A (M, P, ld) f64: the lower triangle of every matrix becomes the factor Ls of
        its equilibrated form (pgl_chol_factor_dev).  Returns (scale (M, P), logdet (M,), info (M,) int32) on A's device.
        Asynchronous on the handle's stream: the caller orders it against the stream that produced A."""
        torch = self._stack(A, 'chol_factor')
        M, P, ld = A.shape
        scale = torch.empty((M, P), dtype=torch.float64, device=A.device)
        logdet = torch.empty(M, dtype=torch.float64, device=A.device)
        info = torch.empty(M, dtype=torch.int32, device=A.device)
        _chk(self.lib.pgl_chol_factor_dev(self.h, _dp(A), int(M), int(P), int(ld), _dp(scale), _dp(logdet), _dp(info)))
        return scale, logdet, info

    def tri_inverse(self, L, info):
        """In place on the torch device tensor L (M, P, ld) f64: the lower triangle of every matrix becomes its inverse
        (pgl_tri_inverse_dev); rows with info[m] != 0 (int32 device tensor, chol_factor's) are skipped.  Asynchronous."""
        torch = self._stack(L, 'tri_inverse')
        if not (isinstance(info, torch.Tensor) and info.is_cuda and info.dtype == torch.int32 and info.is_contiguous() and
                tuple(info.shape) == (L.shape[0],)):
            raise ValueError("tri_inverse: info must be a contiguous int32 device tensor (M,)")
        M, P, ld = L.shape
        _chk(self.lib.pgl_tri_inverse_dev(self.h, _dp(L), int(M), int(P), int(ld), _dp(info)))

    def chol_solve(self, Ls, scale, info, b, out=None):
        """x = A^-1 b for every matrix of the factor Ls (M, P, ld) with chol_factor's scale (M, P) and info (M,)
        (pgl_chol_solve_dev); b (M, P) f64 on the device.  out: (M, P), may be b itself; default a new tensor.  Rows with
        info[m] != 0 are NaN.  Asynchronous on the handle's stream; returns out."""
        torch = self._stack(Ls, 'chol_solve')
        M, P, ld = Ls.shape
        out = torch.empty((M, P), dtype=torch.float64, device=Ls.device) if out is None else out
        for t, dt, shp, what in ((scale, torch.float64, (M, P), 'scale'), (info, torch.int32, (M,), 'info'),
                                 (b, torch.float64, (M, P), 'b'), (out, torch.float64, (M, P), 'out')):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous() and
                    tuple(t.shape) == shp):
                raise ValueError("chol_solve: %s must be a contiguous %s device tensor %s" % (what, dt, shp))
        _chk(self.lib.pgl_chol_solve_dev(self.h, _dp(Ls), int(M), int(P), int(ld), _dp(scale), _dp(info), _dp(b), _dp(out)))
        return out

    # -- time-rescaling goodness of fit (pgl_rescale*) ------------------------------
    def rescale_count(self):
        """(N + 1) int64 offsets of every neuron's rescaled intervals in the concatenated output, for the current time
        range: a neuron with K event bins in the range has max(K - 1, 0) intervals."""
        off = np.empty(self.N + 1, dtype=np.int64)
        _chk(self.lib.pgl_rescale_count(self.h, _ptr(off)))
        return off

    def rescale_dev(self, d_theta, d_Weff, d_tau, d_off, d_stats):
        """Device-pointer form (integers; asynchronous): d_theta (N, P), d_Weff (N, N), d_off (N + 1) int64 = rescale_count(),
        d_tau (d_off[N]) out, d_stats (N, 4) out; see pgl_rescale_dev."""
        _chk(self.lib.pgl_rescale_dev(self.h, _dp(d_theta), _dp(d_Weff), _dp(d_tau), _dp(d_off), _dp(d_stats)))

    def _rescale(self, theta, Weff, call):
        """(tau, off, stats) of rescale / rescale_corr; call(theta, Weff, tau, stats): the library call on their pointers."""
        th, We = self._draw(theta, Weff)
        off = self.rescale_count()
        tau = np.empty(max(int(off[-1]), 1))
        stats = np.empty((self.N, 4))
        _chk(call(_ptr(th), _ptr(We), _ptr(tau), _ptr(stats)))
        return tau[:int(off[-1])], off, stats

    def rescale(self, theta, Weff):
        """Rescaled inter-event intervals of every neuron over the current time range with host arrays: theta (N, P), Weff
        (N, N) -> (tau, off, stats): tau[off[n]:off[n + 1]] are neuron n's intervals, stats (N, 4) = expected count, event
        bins, event bins holding more than one spike, 0."""
        return self._rescale(theta, Weff, lambda th, We, tau, stats: self.lib.pgl_rescale(self.h, th, We, tau, stats))

    # -- discrete-time corrected intervals and the KS distance on the device (pgl_rescale_corr*, pgl_ks_uniform*) ----
    def rescale_corr_dev(self, d_theta, d_Weff, d_tau, d_off, d_stats, seed=0, draw=0):
        """rescale_dev with the discrete-time correction of the event bin's term at the uniforms of (seed, draw); see
        pgl_rescale_corr_dev.  The pointers are integers or torch device tensors."""
        _chk(self.lib.pgl_rescale_corr_dev(self.h, _dp(d_theta), _dp(d_Weff), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                           int(draw), _dp(d_tau), _dp(d_off), _dp(d_stats)))

    def rescale_corr(self, theta, Weff, seed=0, draw=0):
        """rescale with the discrete-time correction: (tau', off, stats); tau' is a random function of seed and draw, the same
        bits for the same pair (pgl_rescale_corr)."""
        seed, draw = C.c_uint64(int(seed) & (2 ** 64 - 1)), int(draw)
        return self._rescale(theta, Weff,
                             lambda th, We, tau, stats: self.lib.pgl_rescale_corr(self.h, th, We, seed, draw, tau, stats))

    def ks_uniform(self, tau, off, out=None, zsorted=None):
        """KS distance from Exp(1) of the segments tau[off[m]:off[m + 1]] of the torch device tensors tau (f64) and off
        (M + 1, int64): -> out (M, 4) = D, D+, D-, n on tau's device, written into `out` (a row of a draws matrix, say)
        where given.  zsorted: True returns (out, z) with every segment's z = -expm1(-tau) sorted, a tensor of tau's length
        is written into, None lets the handle sort in a buffer of its own -- the call then waits once for the stream
        (pgl_ks_uniform_dev)."""
        import torch
        _dev_tensor(tau, 'float64', "ks_uniform: tau must be a contiguous float64 device vector", ndim=1)
        _dev_tensor(off, 'int64', "ks_uniform: off must be a contiguous int64 device vector (M + 1)", ndim=1, numel=2)
        M = int(off.numel()) - 1
        n_tau = int(tau.numel())
        src = tau if n_tau else torch.zeros(1, dtype=torch.float64, device=tau.device)     # (an empty tensor has no address)
        out = _out_tensor(out, (M, KS_NOUT), tau,
                          "ks_uniform: out must be a contiguous float64 device tensor (%d, %d)" % (M, KS_NOUT))
        z = _second_out(zsorted, lambda: torch.empty(max(n_tau, 1), dtype=torch.float64, device=tau.device),
                        lambda t: _dev_tensor(t, 'float64', numel=max(n_tau, 1), msg="ks_uniform: zsorted must be a contiguous "
                                              "float64 device vector of tau's length"))
        _chk(self.lib.pgl_ks_uniform_dev(self.h, _dp(src), _dp(off), M, _dp(out), _dp(z)))
        return (out, z[:n_tau]) if zsorted is True else out

    def ks_uniform_dev(self, d_tau, d_off, M, d_ks, d_zsorted=0):
        """Device-pointer form: see pgl_ks_uniform_dev."""
        _chk(self.lib.pgl_ks_uniform_dev(self.h, _dp(d_tau), _dp(d_off), int(M), _dp(d_ks), _dp(d_zsorted)))

    def ks_uniform_host(self, tau, off, zsorted=False):
        """The same with host arrays: -> ks (M, 4), or (ks, z) with zsorted=True (pgl_ks_uniform)."""
        t = np.ascontiguousarray(tau, dtype=np.float64).ravel()
        o = np.ascontiguousarray(off, dtype=np.int64).ravel()
        if o.size < 2 or o[0] != 0 or int(o[-1]) != t.size:
            raise ValueError("ks_uniform_host: off (M + 1) from 0 to len(tau)")
        M = o.size - 1
        ks = np.empty((M, KS_NOUT))
        z = np.empty(max(t.size, 1)) if zsorted else None
        tt = t if t.size else np.zeros(1)
        _chk(self.lib.pgl_ks_uniform(self.h, _ptr(tt), _ptr(o), int(M), _ptr(ks), _ptr(z) if zsorted else None))
        return (ks, z[:t.size]) if zsorted else ks

    # -- serial correlation of the normal scores of the rescaled intervals (pgl_rescale_acf*) ---------------------------
    def rescale_acf(self, tau, run_off, seg_run, max_lag, out=None, scores=None):
        """Lag-1 .. max_lag serial correlation of the normal scores of the segments of the torch device tensor tau (f64):
        run_off (R + 1, int64) cuts tau into runs, seg_run (M + 1, int64) the runs into segments; pairs never cross a run
        boundary.  -> out (M, 6 + max_lag) = n, mean, c_0, Q, dof, 0, r_1 .. r_L on tau's device, written into `out` where
        given.  scores: True returns (out, g) with every normal score, a tensor of tau's length is written into, None uses a
        fresh one.  Asynchronous on the handle's stream (pgl_rescale_acf_dev)."""
        import torch
        _dev_tensor(tau, 'float64', "rescale_acf: tau must be a contiguous float64 device vector", ndim=1)
        for name, o in (('run_off', run_off), ('seg_run', seg_run)):
            _dev_tensor(o, 'int64', "rescale_acf: %s must be a contiguous int64 device vector" % name, ndim=1, numel=1)
        if seg_run.numel() < 2:
            raise ValueError("rescale_acf: seg_run holds M + 1 >= 2 offsets")
        L = int(max_lag)
        if not 1 <= L <= ACF_MAX_LAG:
            raise ValueError("rescale_acf: max_lag must lie in 1 .. %d" % ACF_MAX_LAG)
        M = int(seg_run.numel()) - 1
        n_tau = int(tau.numel())
        src = tau if n_tau else torch.zeros(1, dtype=torch.float64, device=tau.device)     # (an empty tensor has no address)
        out = _out_tensor(out, (M, ACF_NHEAD + L), tau,
                          "rescale_acf: out must be a contiguous float64 device tensor (%d, %d)" % (M, ACF_NHEAD + L))
        g = _second_out(scores, lambda: torch.empty(max(n_tau, 1), dtype=torch.float64, device=tau.device),
                        lambda t: _dev_tensor(t, 'float64', numel=max(n_tau, 1), msg="rescale_acf: scores must be a contiguous "
                                              "float64 device vector of tau's length"), none_is_fresh=True)
        _chk(self.lib.pgl_rescale_acf_dev(self.h, _dp(src), _dp(run_off), _dp(seg_run), M, L, _dp(out), _dp(g)))
        return (out, g[:n_tau]) if scores is True else out

    def rescale_acf_dev(self, d_tau, d_run_off, d_seg_run, M, max_lag, d_out, d_scores):
        """Device-pointer form: see pgl_rescale_acf_dev."""
        _chk(self.lib.pgl_rescale_acf_dev(self.h, _dp(d_tau), _dp(d_run_off), _dp(d_seg_run), int(M), int(max_lag),
                                          _dp(d_out), _dp(d_scores)))

    def rescale_acf_host(self, tau, run_off, seg_run, max_lag, scores=False):
        """The same with host arrays: -> out (M, 6 + max_lag), or (out, g) with scores=True (pgl_rescale_acf)."""
        t = np.ascontiguousarray(tau, dtype=np.float64).ravel()
        ro = np.ascontiguousarray(run_off, dtype=np.int64).ravel()
        sr = np.ascontiguousarray(seg_run, dtype=np.int64).ravel()
        if sr.size < 2 or sr[0] != 0 or int(sr[-1]) != ro.size - 1 or ro[0] != 0 or int(ro[-1]) != t.size:
            raise ValueError("rescale_acf_host: seg_run (M + 1) from 0 to R, run_off (R + 1) from 0 to len(tau)")
        M = sr.size - 1
        out = np.empty((M, ACF_NHEAD + int(max_lag)))
        g = np.empty(max(t.size, 1)) if scores else None
        tt = t if t.size else np.zeros(1)
        _chk(self.lib.pgl_rescale_acf(self.h, _ptr(tt), _ptr(ro), _ptr(sr), int(M), int(max_lag), _ptr(out),
                                      _ptr(g) if scores else None))
        return (out, g[:t.size]) if scores else out

    # -- pointwise log-likelihood of a draw, and its accumulation over draws (pgl_pointwise*) -------------
    def pointwise_count(self, block_chunks=1):
        """Number of time blocks of block_chunks chunks (RESCALE_CHUNK bins each, counted from t_lo) in the current time
        range."""
        n = C.c_int64()
        _chk(self.lib.pgl_pointwise_count(self.h, int(block_chunks), C.byref(n)))
        return int(n.value)

    def pointwise_dev(self, d_theta, d_Weff, block_chunks, d_ll_blk=0, d_acc=0, draw=0):
        """Device-pointer form (integers; asynchronous): d_theta (N, P), d_Weff (N, N), d_ll_blk (n_blocks, N) out or 0,
        d_acc (4, n_blocks, N) in/out or 0 with the index `draw` of this draw; see pgl_pointwise_dev."""
        _chk(self.lib.pgl_pointwise_dev(self.h, _dp(d_theta), _dp(d_Weff), int(block_chunks), _dp(d_ll_blk), _dp(d_acc),
                                        int(draw)))

    def pointwise(self, theta, Weff, block_chunks=1):
        """Block sums of the log-likelihood terms of every neuron over the current time range with host arrays: theta
        (N, P), Weff (N, N) -> (n_blocks, N)."""
        th, We = self._draw(theta, Weff)
        out = np.empty((self.pointwise_count(block_chunks), self.N))
        _chk(self.lib.pgl_pointwise(self.h, _ptr(th), _ptr(We), int(block_chunks), _ptr(out)))
        return out

    # -- expected and observed counts over time windows, and their accumulation over draws (pgl_rate_windows*) ----
    def rate_windows_count(self, win):
        """Number of windows of `win` bins (counted from t_lo, the last one may be short) in the current time range."""
        n = C.c_int64()
        _chk(self.lib.pgl_rate_windows_count(self.h, int(win), C.byref(n)))
        return int(n.value)

    def rate_windows_dev(self, d_theta, d_Weff, win, d_lam=0, d_obs=0, d_acc=0, draw=0):
        """Device-pointer form (integers; asynchronous): d_theta (N, P), d_Weff (N, N), d_lam and d_obs (n_win, N) out or 0,
        d_acc (RW_NACC, n_win, N) in/out or 0 with the index `draw` of this draw; see pgl_rate_windows_dev."""
        _chk(self.lib.pgl_rate_windows_dev(self.h, _dp(d_theta), _dp(d_Weff), int(win), _dp(d_lam), _dp(d_obs), _dp(d_acc),
                                           int(draw)))

    def rate_windows(self, theta, Weff, win):
        """Expected and observed spike counts of every neuron over windows of `win` bins of the current time range with host
        arrays: theta (N, P), Weff (N, N) -> (Lam, obs), each (n_win, N)."""
        th, We = self._draw(theta, Weff)
        n_win = self.rate_windows_count(win)
        lam = np.empty((n_win, self.N))
        obs = np.empty((n_win, self.N))
        _chk(self.lib.pgl_rate_windows(self.h, _ptr(th), _ptr(We), int(win), _ptr(lam), _ptr(obs)))
        return lam, obs

    # -- stimulus decoding: F(u), its gradient and Hessian-vector products w.r.t. the stimulus (pgl_decode_*) ------------
    def _decode_array(self, a, name, Tu=None):
        """a as a contiguous float64 (Tu, D) array, D the stimulus dimensions of the 'basis' stimulus on the handle; ValueError
        where its shape is another (the library moves Tu * D doubles each way)."""
        a = _f64(a)
        if self.dec_D is None:
            raise ValueError("stimulus decoding needs a 'basis' stimulus on the handle (set_stimulus with basis_x=None, layout=1)")
        if a.ndim != 2 or a.shape[1] != self.dec_D or (Tu is not None and a.shape[0] != Tu):
            raise ValueError("%s must be (Tu, D) = (%s, %d), got %s" % (name, 'Tu' if Tu is None else Tu, self.dec_D, a.shape))
        return a

    def decode_prepare(self, theta, Weff):
        """Builds the filters K and the offset c = bias + the currents of the recorded spikes at the host arrays theta (N, P),
        Weff (N, N) and keeps them on the device for decode_eval / decode_hvp; see pgl_decode_prepare.  A 'basis' stimulus
        only.  The handle's copy of theta and its currents GX are overwritten."""
        th, We = self._draw(theta, Weff)
        _chk(self.lib.pgl_decode_prepare(self.h, _ptr(th), _ptr(We)))
        self._dec_Tu = None

    def decode_prepare_dev(self, d_theta, d_Weff):
        """Device-pointer form (integers; asynchronous): d_theta (N, P), d_Weff (N, N)."""
        _chk(self.lib.pgl_decode_prepare_dev(self.h, _dp(d_theta), _dp(d_Weff)))
        self._dec_Tu = None

    def decode_eval_dev(self, d_u, Tu, q, prior, d_F, d_grad_u=0):
        """Device-pointer form (integers; asynchronous): d_u (Tu, D) -> d_F (3,) and d_grad_u (Tu, D) or 0; prior: (mu, sigma,
        rho) or a DecodePrior; see pgl_decode_eval_dev.  The caller answers for the shapes."""
        pr = as_decode_prior(prior)
        _chk(self.lib.pgl_decode_eval_dev(self.h, _dp(d_u), int(Tu), int(q), C.byref(pr), _dp(d_F), _dp(d_grad_u)))
        self._dec_Tu = int(Tu)

    def decode_hvp_dev(self, d_v, d_hv):
        """d_hv = H d_v at the point, Tu, q and prior of the last decode_eval[_dev] (device pointers; asynchronous)."""
        _chk(self.lib.pgl_decode_hvp_dev(self.h, _dp(d_v), _dp(d_hv)))

    def decode_eval(self, u, q, prior, want_grad=True):
        """(F (3,): F, log likelihood, log prior; grad (Tu, D) or None) at the host array u (Tu, D) behind decode_prepare."""
        u = self._decode_array(u, 'u')
        F = np.empty(DEC_NF)
        g = np.empty(u.shape) if want_grad else None
        pr = as_decode_prior(prior)
        _chk(self.lib.pgl_decode_eval(self.h, _ptr(u), u.shape[0], u.shape[1], int(q), C.byref(pr), _ptr(F), _ptr(g)))
        self._dec_Tu = u.shape[0]
        return F, g

    def decode_hvp(self, v):
        """H v (Tu, D) at the point of the last decode_eval, host arrays."""
        v = self._decode_array(v, 'v', getattr(self, '_dec_Tu', None))
        out = np.empty(v.shape)
        _chk(self.lib.pgl_decode_hvp(self.h, _ptr(v), v.shape[0], v.shape[1], _ptr(out)))
        return out

    # -- PSIS-LOO of the columns of a pointwise matrix over draws (pgl_psis_loo*) -----------------------
    def psis_loo(self, ll, out=None, weights=False):
        """PSIS-LOO of every column of the torch device tensor ll (S, ...) f64, the draws on axis 0 (pgl_psis_loo_dev).  The
        trailing axes are flattened to columns; they must be contiguous among themselves, and the stride of axis 0 is the
        leading dimension, so a last-axis slice full[:, a:b] of a matrix is served where it is.  Returns out (4, ...) on ll's
        device -- elpd, khat, n_eff, tail length per column; `out`: a contiguous tensor of that shape to write into.
        weights=True also returns the log weights, a tensor of ll's shape and strides; weights=<tensor of ll's shape and
        strides> writes them there (it must not overlap ll).  Asynchronous on the handle's stream."""
        import torch
        _dev_tensor(ll, 'float64', "psis_loo: a float64 device tensor (S, ...)", min_ndim=2, numel=1, contiguous=False)
        S, shape = int(ll.shape[0]), tuple(ll.shape[1:])
        ncol = int(np.prod(shape))
        ld = int(ll.stride(0))
        if not ll[0].is_contiguous() or ld < ncol:
            raise ValueError("psis_loo: the trailing axes must be contiguous and the draw stride at least their size")
        out = _out_tensor(out, (PSIS_NOUT,) + shape, ll,
                          "psis_loo: out must be a contiguous float64 device tensor %s" % ((PSIS_NOUT,) + shape,))
        lw = _second_out(weights, lambda: torch.empty_strided(tuple(ll.shape), ll.stride(), dtype=torch.float64, device=ll.device),
                         lambda t: _dev_tensor(t, 'float64', "psis_loo: weights must be a float64 device tensor of ll's shape and "
                                               "strides", shape=ll.shape, strides=ll.stride(), contiguous=False))
        _chk(self.lib.pgl_psis_loo_dev(self.h, _dp(ll), S, ncol, ld, _dp(out), _dp(lw)))
        return out if lw is None else (out, lw)

    def psis_loo_host(self, ll, weights=False):
        """The same with a host array ll (S, ...): -> out (4, ...), or (out, lw) with weights=True (pgl_psis_loo)."""
        a = np.ascontiguousarray(ll, dtype=np.float64)
        if a.ndim < 2 or a.size == 0:
            raise ValueError("psis_loo_host: an array (S, ...)")
        S, shape = a.shape[0], a.shape[1:]
        out = np.empty((PSIS_NOUT,) + shape)
        lw = np.empty(a.shape) if weights else None
        _chk(self.lib.pgl_psis_loo(self.h, _ptr(a), int(S), int(np.prod(shape)), _ptr(out), _ptr(lw) if weights else None))
        return (out, lw) if weights else out

    # -- Wald statistics of the coupling groups from the factor of the Laplace covariance (pgl_wald_groups*) -----------
    def wald_groups(self, W, theta, first, G, B, c, info, out=None, u=False):
        """T, lin, var, info of the G groups of B weights from column `first` of every row (pgl_wald_groups_dev; the rule:
        csrc/pglm_wald.h).  Torch device tensors: W (M, P, ld) f64, ld >= P, row m lower triangular in its first P columns
        with W W^T the Laplace covariance, theta (M, P) f64, c (B,) f64, info (M,) int32 (chol_factor's).
        Returns out (M, G, 4) on W's device, written into `out` where given; u=True also returns (G * M, P) = W_g^T S^-1 w_g,
        row g * M + m, u=<tensor of that shape> writes it there.  Asynchronous on the handle's stream."""
        torch = self._stack(W, 'wald_groups')
        M, P, ld = (int(v) for v in W.shape)
        G, B, first = int(G), int(B), int(first)
        _dev_tensor(theta, 'float64', "wald_groups: theta must be a contiguous float64 device tensor (M, P)", shape=(M, P))
        _dev_tensor(c, 'float64', "wald_groups: c must be a contiguous float64 device tensor (B,)", shape=(B,))
        _dev_tensor(info, 'int32', "wald_groups: info must be a contiguous int32 device tensor (M,)", shape=(M,))
        out = _out_tensor(out, (M, G, WALD_NOUT), W, "wald_groups: out must be a contiguous float64 device tensor (M, G, 4)")
        du = _second_out(u, lambda: torch.empty((G * M, P), dtype=torch.float64, device=W.device),
                         lambda t: _dev_tensor(t, 'float64', "wald_groups: u must be a contiguous float64 device tensor (G * M, P)",
                                               shape=(G * M, P)))
        _chk(self.lib.pgl_wald_groups_dev(self.h, _dp(W), M, P, ld, _dp(theta), first, G, B, _dp(c), _dp(info), _dp(out), _dp(du)))
        return out if du is None else (out, du)

    def wald_groups_dev(self, d_W, M, P, ld, d_theta, first, G, B, d_c, d_info, d_out, d_u=0):
        """Device-pointer form (integers or tensors; d_u = 0: no directions): see pgl_wald_groups_dev."""
        _chk(self.lib.pgl_wald_groups_dev(self.h, _dp(d_W), int(M), int(P), int(ld), _dp(d_theta), int(first), int(G), int(B),
                                          _dp(d_c), _dp(d_info), _dp(d_out), _dp(d_u)))

    def wald_groups_host(self, W, theta, first, G, B, c, info=None, u=False):
        """The same with host arrays: W (M, P, ld), theta (M, P), c (B,), info (M,) or None for zeros -> out (M, G, 4), or
        (out, u) with u=True (pgl_wald_groups)."""
        Wc = np.ascontiguousarray(W, dtype=np.float64)
        if Wc.ndim != 3:
            raise ValueError("wald_groups_host: W (M, P, ld)")
        M, P, ld = Wc.shape
        th = _f64(theta, (M, P))
        cc = _f64(c, (int(B),))
        inf = np.zeros(M, dtype=np.int32) if info is None else np.ascontiguousarray(info, dtype=np.int32)
        if inf.shape != (M,):
            raise ValueError("wald_groups_host: info (M,)")
        out = np.empty((M, int(G), WALD_NOUT))
        uu = np.empty((int(G) * M, P)) if u else None
        _chk(self.lib.pgl_wald_groups(self.h, _ptr(Wc), M, P, ld, _ptr(th), int(first), int(G), int(B), _ptr(cc), _ptr(inf),
                                      _ptr(out), _ptr(uu)))
        return (out, uu) if u else out

    # -- convergence diagnostics of the columns of a samplers' tensor (pgl_chain_diag*) ------------------
    def chain_diag(self, x, n_chains=1, out=None):
        """Rank-normalised split-R-hat, bulk / tail / mean ESS, MCSE and the pooled moments and quantiles of every column
        of the torch device tensor x (n, n_chains * M, ...) f64 as the lock-step samplers keep it: draw i of chain c of
        neuron m in row c * M + m (pgl_chain_diag_dev; the rule: csrc/pglm_diag.h).  The trailing axes must be contiguous
        among themselves; the stride of axis 0 may exceed their size.  Returns out (DIAG_NOUT, M, ...) on x's device, rows
        in DIAG_ROWS order; `out`: a contiguous tensor of that shape to write into.  Asynchronous on the handle's stream."""
        import torch
        nc = int(n_chains)
        _dev_tensor(x, 'float64', "chain_diag: a float64 device tensor (n, n_chains * M, ...)", min_ndim=2, numel=1,
                    contiguous=False)
        if nc < 1 or x.shape[1] % nc:
            raise ValueError("chain_diag: axis 1 must hold n_chains blocks of rows")
        n, shape = int(x.shape[0]), (int(x.shape[1]) // nc,) + tuple(x.shape[2:])
        K = int(np.prod(shape))
        if not x[0].is_contiguous() or int(x.stride(0)) < nc * K or int(x.stride(0)) % nc:
            raise ValueError("chain_diag: the trailing axes must be contiguous and the draw stride a multiple of n_chains")
        if nc > 1 and int(x.stride(0)) != nc * K:
            raise ValueError("chain_diag: with n_chains > 1 the draws must be contiguous")
        ld = int(x.stride(0)) // nc
        out = _out_tensor(out, (DIAG_NOUT,) + shape, x,
                          "chain_diag: out must be a contiguous float64 device tensor %s" % ((DIAG_NOUT,) + shape,))
        _chk(self.lib.pgl_chain_diag_dev(self.h, _dp(x), n, nc, K, ld, _dp(out)))
        return out

    def chain_diag_host(self, x, n_chains=1):
        """The same with a host array x (n, n_chains * M, ...): -> out (DIAG_NOUT, M, ...) (pgl_chain_diag)."""
        a = np.ascontiguousarray(x, dtype=np.float64)
        nc = int(n_chains)
        if a.ndim < 2 or a.size == 0 or nc < 1 or a.shape[1] % nc:
            raise ValueError("chain_diag_host: an array (n, n_chains * M, ...)")
        shape = (a.shape[1] // nc,) + a.shape[2:]
        out = np.empty((DIAG_NOUT,) + shape)
        _chk(self.lib.pgl_chain_diag(self.h, _ptr(a), int(a.shape[0]), nc, int(np.prod(shape)), _ptr(out)))
        return out

    # -- posterior bands of the filters from the samplers' draws (pgl_filter_bands*) ----------------------
    def filter_bands(self, samples, n_chains, first, G, basis, c, level, out=None, grp=None):
        """The bands of the G groups of B weights from column `first` of every theta row over the draws of the torch device
        tensor samples (n, n_chains * M, P) f64, contiguous, as the lock-step samplers keep it (pgl_filter_bands_dev; the
        rule: csrc/pglm_filters.h).  basis (R, B) and c (B,) contiguous f64 device tensors.  Returns (out (M, G, R, 5) in
        FILT_LAG_COLS order, grp (M, G, 8) in FILT_GRP_COLS order) on the samples' device, written into `out` / `grp` where
        given.  Asynchronous on the handle's stream."""
        nc = int(n_chains)
        _dev_tensor(samples, 'float64', "filter_bands: samples must be a contiguous float64 device tensor (n, n_chains * M, P)",
                    ndim=3, numel=1)
        if nc < 1 or samples.shape[1] % nc:
            raise ValueError("filter_bands: axis 1 must hold n_chains blocks of rows")
        n, M, P = int(samples.shape[0]), int(samples.shape[1]) // nc, int(samples.shape[2])
        _dev_tensor(basis, 'float64', "filter_bands: basis must be a contiguous float64 device tensor (R, B)", ndim=2, numel=1)
        R, B = (int(v) for v in basis.shape)
        G, first = int(G), int(first)
        _dev_tensor(c, 'float64', "filter_bands: c must be a contiguous float64 device tensor (B,)", shape=(B,))
        out = _out_tensor(out, (M, G, R, len(FILT_LAG_COLS)), samples,
                          "filter_bands: out must be a contiguous float64 device tensor (M, G, R, 5)")
        grp = _out_tensor(grp, (M, G, len(FILT_GRP_COLS)), samples,
                          "filter_bands: grp must be a contiguous float64 device tensor (M, G, 8)")
        _chk(self.lib.pgl_filter_bands_dev(self.h, _dp(samples), n, nc, M, P, first, G, B, _dp(basis), R, _dp(c), float(level),
                                           _dp(out), _dp(grp)))
        return out, grp

    def filter_bands_dev(self, d_samples, n, C_, M, P, first, G, B, d_basis, R, d_c, level, d_out, d_grp):
        """Device-pointer form (integers or tensors): see pgl_filter_bands_dev."""
        _chk(self.lib.pgl_filter_bands_dev(self.h, _dp(d_samples), int(n), int(C_), int(M), int(P), int(first), int(G), int(B),
                                           _dp(d_basis), int(R), _dp(d_c), float(level), _dp(d_out), _dp(d_grp)))

    def filter_bands_host(self, samples, n_chains, first, G, basis, c, level):
        """The same with host arrays: samples (n, n_chains * M, P), basis (R, B), c (B,) -> (out (M, G, R, 5), grp (M, G, 8))
        (pgl_filter_bands)."""
        a = np.ascontiguousarray(samples, dtype=np.float64)
        nc = int(n_chains)
        if a.ndim != 3 or a.size == 0 or nc < 1 or a.shape[1] % nc:
            raise ValueError("filter_bands_host: samples (n, n_chains * M, P)")
        n, M, P = a.shape[0], a.shape[1] // nc, a.shape[2]
        bs = np.ascontiguousarray(basis, dtype=np.float64)
        if bs.ndim != 2 or bs.size == 0:
            raise ValueError("filter_bands_host: basis (R, B)")
        R, B = bs.shape
        cc = _f64(c, (B,))
        out = np.empty((M, int(G), R, len(FILT_LAG_COLS)))
        grp = np.empty((M, int(G), len(FILT_GRP_COLS)))
        _chk(self.lib.pgl_filter_bands(self.h, _ptr(a), int(n), nc, int(M), int(P), int(first), int(G), int(B), _ptr(bs), int(R),
                                       _ptr(cc), float(level), _ptr(out), _ptr(grp)))
        return out, grp

    # -- lock-step optimiser bookkeeping (device pointers as integers; asynchronous on the handle's stream) --
    def bfgs_state_doubles(self, M, P):
        return int(self.lib.pgl_bfgs_state_doubles(int(M), int(P)))

    def bfgs_trial_dev(self, d_state, M, P, d_rows, L, d_Xt):
        _chk(self.lib.pgl_bfgs_trial_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt)))

    # prior, here and below: a Prior or the tuple of _Packing.prior_params() (as_prior)
    def bfgs_objective_dev(self, L, P, d_Xt, d_ll_f, d_grad_g, prior):
        _chk(self.lib.pgl_bfgs_objective_dev(self.h, int(L), int(P), _dp(d_Xt), _dp(d_ll_f), _dp(d_grad_g),
                                             C.byref(as_prior(prior))))

    def bfgs_init_dev(self, d_state, M, P, gtol):
        _chk(self.lib.pgl_bfgs_init_dev(self.h, _dp(d_state), int(M), int(P), float(gtol)))

    def bfgs_linesearch_dev(self, d_state, M, P, d_rows, L, d_Xt, d_f, d_g, max_trials=100):
        _chk(self.lib.pgl_bfgs_linesearch_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt), _dp(d_f),
                                              _dp(d_g), int(max_trials)))

    def bfgs_hmul_dev(self, d_state, M, P, d_rows, L, d_H, ld):
        _chk(self.lib.pgl_bfgs_hmul_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_H), int(ld)))

    def bfgs_hmul_hist_dev(self, d_state, M, P, d_rows, L, d_hist, d_coef, Kmax, d_ab):
        _chk(self.lib.pgl_bfgs_hmul_hist_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_hist),
                                             _dp(d_coef), int(Kmax), _dp(d_ab)))

    def bfgs_update_dev(self, d_state, M, P, gtol, maxiter, init_scaling=False, d_hist=0, d_coef=0, Kmax=0):
        _chk(self.lib.pgl_bfgs_update_dev(self.h, _dp(d_state), int(M), int(P), float(gtol), int(maxiter),
                                          1 if init_scaling else 0, _dp(d_hist), _dp(d_coef), int(Kmax)))

    def bfgs_step_dev(self, d_state, M, P, d_rows, L, d_Xt, d_f, d_g, prior=None, max_trials=100, gtol=1e-5, maxiter=225,
                      init_scaling=False, d_hist=0, d_coef=0, Kmax=0, d_ab=0, hk_bound=0, d_H=0, ld=0, d_pos_next=0,
                      d_Xt_next=0, flags_out=0):
        """One whole optimiser iteration behind an evaluation (pgl_bfgs_step_dev).  prior: as for bfgs_objective_dev, or
        None when d_f / d_g already hold the objective and its gradient."""
        pr = (-1, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0) if prior is None else prior
        _chk(self.lib.pgl_bfgs_step_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt), _dp(d_f),
                                        _dp(d_g), C.byref(as_prior(pr)), int(max_trials), float(gtol), int(maxiter),
                                        1 if init_scaling else 0, _dp(d_hist), _dp(d_coef), int(Kmax), _dp(d_ab),
                                        int(hk_bound), _dp(d_H), int(ld), _dp(d_pos_next), _dp(d_Xt_next), _dp(flags_out)))

    # -- lock-step Newton-CG row kernels (pgl_ncg_*; inference/batched_newton_cg.py)
    def ncg_state_doubles(self, M, P):
        return int(self.lib.pgl_ncg_state_doubles(int(M), int(P)))

    def ncg_init_dev(self, d_state, M, P, d_ll, d_grad, prior, maxiter, d_V, flags_out=0):
        _chk(self.lib.pgl_ncg_init_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_ll), _dp(d_grad),
                                       C.byref(as_prior(prior)), int(maxiter), _dp(d_V), _dp(flags_out)))

    def ncg_cg_step_dev(self, d_state, M, P, d_hv, prior, d_V, flags_out=0):
        _chk(self.lib.pgl_ncg_cg_step_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_hv), C.byref(as_prior(prior)),
                                          _dp(d_V), _dp(flags_out)))

    def ncg_trial_dev(self, d_state, M, P, d_rows, L, d_Xt):
        _chk(self.lib.pgl_ncg_trial_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt)))

    def ncg_search_step_dev(self, d_state, M, P, d_rows, L, d_Xt, d_f, d_g, prior, maxiter, d_pos_next, d_Xt_next, d_V,
                            flags_out=0):
        _chk(self.lib.pgl_ncg_search_step_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt), _dp(d_f),
                                              _dp(d_g), C.byref(as_prior(prior)), int(maxiter), _dp(d_pos_next),
                                              _dp(d_Xt_next), _dp(d_V), _dp(flags_out)))

    # -- lock-step dense Newton row kernels (pgl_newton_*; inference/batched_newton.py); device pointers
    def newton_state_doubles(self, M, P):
        return int(self.lib.pgl_newton_state_doubles(int(M), int(P)))

    def newton_init_dev(self, d_state, M, P, d_ll, d_grad, prior, gtol, maxiter, flags_out=0):
        _chk(self.lib.pgl_newton_init_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_ll), _dp(d_grad),
                                          C.byref(as_prior(prior)), float(gtol), int(maxiter), _dp(flags_out)))

    def newton_assemble_dev(self, d_state, M, P, d_rows, L, d_H, ld, prior, d_rhs=0):
        _chk(self.lib.pgl_newton_assemble_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_H), int(ld),
                                              C.byref(as_prior(prior)), _dp(d_rhs)))

    def newton_direction_dev(self, d_state, M, P, d_rows, L, d_info, d_p, flags_out=0):
        _chk(self.lib.pgl_newton_direction_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_info),
                                               _dp(d_p), _dp(flags_out)))

    def newton_trial_dev(self, d_state, M, P, d_rows, L, d_Xt):
        _chk(self.lib.pgl_newton_trial_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt)))

    def newton_search_step_dev(self, d_state, M, P, d_rows, L, d_Xt, d_f, d_g, prior, gtol, maxiter, d_pos_next, d_Xt_next,
                               flags_out=0):
        _chk(self.lib.pgl_newton_search_step_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_rows), int(L), _dp(d_Xt),
                                                 _dp(d_f), _dp(d_g), C.byref(as_prior(prior)), float(gtol), int(maxiter),
                                                 _dp(d_pos_next), _dp(d_Xt_next), _dp(flags_out)))

    # -- lock-step HMC row kernels (pgl_hmc_*; inference/batched_hmc.py); device pointers.  n_chains = C: the run has R = C M
    # rows, chain c of neuron n_lo + m is row c M + m, and every call after init takes R as its M
    def hmc_state_doubles(self, M, P):
        return int(self.lib.pgl_hmc_state_doubles(int(M), int(P)))

    def hmc_init_dev(self, d_state, M, P, n_lo, d_ll, d_grad, prior, step0, seed, n_chains=1):
        _chk(self.lib.pgl_hmc_init_dev(self.h, _dp(d_state), int(M), int(n_chains), int(P), int(n_lo), _dp(d_ll),
                                       _dp(d_grad), C.byref(as_prior(prior)), float(step0), int(seed) & 0xffffffffffffffff))

    def hmc_begin_dev(self, d_state, M, P, d_minv, d_Xt):
        _chk(self.lib.pgl_hmc_begin_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_minv), _dp(d_Xt)))

    def hmc_leap_dev(self, d_state, M, P, d_minv, d_ll, d_grad, prior, last, n_warmup, d_Xt, d_sample_out=0):
        _chk(self.lib.pgl_hmc_leap_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_minv), _dp(d_ll), _dp(d_grad),
                                       C.byref(as_prior(prior)), 1 if last else 0, int(n_warmup), _dp(d_Xt),
                                       _dp(d_sample_out)))

    # -- NUTS row kernels (pgl_nuts_*; inference/batched_nuts.py).  d_minv (M, P) or d_W (M, P, P) or neither; device pointers;
    # n_chains as for hmc_init_dev (d_minv, d_W: one per row)
    def nuts_state_doubles(self, M, P, max_depth):
        return int(self.lib.pgl_nuts_state_doubles(int(M), int(P), int(max_depth)))

    def nuts_init_dev(self, d_state, M, P, max_depth, n_lo, d_ll, d_grad, prior, d_minv, d_W, d_step0, seed, n_warmup, thin,
                      n_keep, d_Xt, n_chains=1):
        _chk(self.lib.pgl_nuts_init_dev(self.h, _dp(d_state), int(M), int(n_chains), int(P), int(max_depth), int(n_lo),
                                        _dp(d_ll), _dp(d_grad), C.byref(as_prior(prior)), _dp(d_minv), _dp(d_W),
                                        _dp(d_step0), int(seed) & 0xffffffffffffffff, int(n_warmup), int(thin), int(n_keep),
                                        _dp(d_Xt)))

    def nuts_step_dev(self, d_state, M, P, max_depth, d_ll, d_grad, prior, d_minv, d_W, target_accept, n_warmup, thin, n_keep,
                      d_Xt, d_samples=0, d_stats=0):
        _chk(self.lib.pgl_nuts_step_dev(self.h, _dp(d_state), int(M), int(P), int(max_depth), _dp(d_ll), _dp(d_grad),
                                        C.byref(as_prior(prior)), _dp(d_minv), _dp(d_W), float(target_accept), int(n_warmup),
                                        int(thin), int(n_keep), _dp(d_Xt), _dp(d_samples), _dp(d_stats)))

    # -- the warm-up mass adaptation (csrc/pglm_adapt.h) over the R rows of a run; d_adapt: adapt_state_doubles(R, P) zeroed
    # doubles; d_sched: mass_adapt.schedule_ints on the device
    def adapt_state_doubles(self, R, P):
        return int(self.lib.pgl_adapt_state_doubles(int(R), int(P)))

    def mass_adapt_dev(self, d_state, R, P, d_adapt, d_sched, d_minv):
        _chk(self.lib.pgl_mass_adapt_dev(self.h, _dp(d_state), int(R), int(P), _dp(d_adapt), _dp(d_sched), _dp(d_minv)))

    def nuts_adapt_step_dev(self, d_state, R, P, max_depth, d_ll, d_grad, prior, d_minv, d_adapt, d_sched, target_accept,
                            n_warmup, thin, n_keep, d_Xt, d_samples=0, d_stats=0):
        _chk(self.lib.pgl_nuts_adapt_step_dev(self.h, _dp(d_state), int(R), int(P), int(max_depth), _dp(d_ll), _dp(d_grad),
                                              C.byref(as_prior(prior)), _dp(d_minv), _dp(d_adapt), _dp(d_sched),
                                              float(target_accept), int(n_warmup), int(thin), int(n_keep), _dp(d_Xt),
                                              _dp(d_samples), _dp(d_stats)))

    # -- the same chain with a dense mass matrix (pgl_hmc_dense_*): d_W (M, P, P) lower-triangular factors of the inverse
    # mass matrices
    def tri_matvec_dev(self, d_W, M, P, trans, d_x, d_y):
        _chk(self.lib.pgl_tri_matvec_dev(self.h, _dp(d_W), int(M), int(P), 1 if trans else 0, _dp(d_x), _dp(d_y)))

    def hmc_dense_begin_dev(self, d_state, M, P, d_W, d_Xt):
        _chk(self.lib.pgl_hmc_dense_begin_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_W), _dp(d_Xt)))

    def hmc_dense_leap_dev(self, d_state, M, P, d_W, d_ll, d_grad, prior, last, n_warmup, d_Xt, d_sample_out=0):
        _chk(self.lib.pgl_hmc_dense_leap_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_W), _dp(d_ll), _dp(d_grad),
                                             C.byref(as_prior(prior)), 1 if last else 0, int(n_warmup), _dp(d_Xt),
                                             _dp(d_sample_out)))

    # -- lock-step proximal gradient row kernels for the group-lasso MAP (pgl_prox_*; inference/batched_prox.py).  prior:
    # kind 1, its lam unused (_prox_prior); d_lam: (M) device, one lam per row; flags_out: pinned host memory or 0
    def prox_state_doubles(self, M, P):
        return int(self.lib.pgl_prox_state_doubles(int(M), int(P)))

    def prox_init_dev(self, d_state, M, P, d_ll, d_grad, prior, d_lam, gtol, maxiter, d_Xt, flags_out=0):
        _chk(self.lib.pgl_prox_init_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_ll), _dp(d_grad),
                                        C.byref(_prox_prior(prior)), _dp(d_lam), float(gtol), int(maxiter), _dp(d_Xt),
                                        _dp(flags_out)))

    def prox_step_dev(self, d_state, M, P, d_ll, d_grad, prior, d_lam, gtol, maxiter, max_backtrack, d_Xt, flags_out=0):
        _chk(self.lib.pgl_prox_step_dev(self.h, _dp(d_state), int(M), int(P), _dp(d_ll), _dp(d_grad),
                                        C.byref(_prox_prior(prior)), _dp(d_lam), float(gtol), int(maxiter),
                                        int(max_backtrack), _dp(d_Xt), _dp(flags_out)))

    # -- annealed importance sampling row kernels (pgl_ais_*; inference/batched_ais.py).  K particles x M neurons, rows
    # particle-major; prior: Gaussian only; device pointers
    def ais_state_doubles(self, R, P):
        return int(self.lib.pgl_ais_state_doubles(int(R), int(P)))

    def ais_init_dev(self, d_state, K, M, P, n_lo, particle0, prior, step0, seed, d_Xt):
        _chk(self.lib.pgl_ais_init_dev(self.h, _dp(d_state), int(K), int(M), int(P), int(n_lo), int(particle0),
                                       C.byref(as_prior(prior)), float(step0), int(seed) & 0xffffffffffffffff, _dp(d_Xt)))

    def ais_start_dev(self, d_state, K, M, P, d_ll, d_grad, prior):
        _chk(self.lib.pgl_ais_start_dev(self.h, _dp(d_state), int(K), int(M), int(P), _dp(d_ll), _dp(d_grad),
                                        C.byref(as_prior(prior))))

    def ais_temper_dev(self, d_state, K, M, P, prior, beta, d_step_row=0):
        _chk(self.lib.pgl_ais_temper_dev(self.h, _dp(d_state), int(K), int(M), int(P), C.byref(as_prior(prior)), float(beta),
                                         _dp(d_step_row)))

    def ais_begin_dev(self, d_state, K, M, P, d_minv, d_Xt):
        _chk(self.lib.pgl_ais_begin_dev(self.h, _dp(d_state), int(K), int(M), int(P), _dp(d_minv), _dp(d_Xt)))

    def ais_leap_dev(self, d_state, K, M, P, d_minv, d_ll, d_grad, prior, last, adapt, d_Xt, d_acc_out=0, d_step_out=0):
        _chk(self.lib.pgl_ais_leap_dev(self.h, _dp(d_state), int(K), int(M), int(P), _dp(d_minv), _dp(d_ll), _dp(d_grad),
                                       C.byref(as_prior(prior)), 1 if last else 0, 1 if adapt else 0, _dp(d_Xt),
                                       _dp(d_acc_out), _dp(d_step_out)))

    # -- the same run with a dense mass matrix (pgl_ais_dense_*): d_W (M, P, P) lower-triangular factors of the inverse mass
    # matrices, one per NEURON, shared by its K particles; d_x, d_y (K M, P) particle-major
    def tri_matvec_shared_dev(self, d_W, M, K, P, trans, d_x, d_y):
        _chk(self.lib.pgl_tri_matvec_shared_dev(self.h, _dp(d_W), int(M), int(K), int(P), 1 if trans else 0, _dp(d_x),
                                                _dp(d_y)))

    def ais_dense_begin_dev(self, d_state, K, M, P, d_W, d_Xt):
        _chk(self.lib.pgl_ais_dense_begin_dev(self.h, _dp(d_state), int(K), int(M), int(P), _dp(d_W), _dp(d_Xt)))

    def ais_dense_leap_dev(self, d_state, K, M, P, d_W, d_ll, d_grad, prior, last, adapt, d_Xt, d_acc_out=0, d_step_out=0):
        _chk(self.lib.pgl_ais_dense_leap_dev(self.h, _dp(d_state), int(K), int(M), int(P), _dp(d_W), _dp(d_ll), _dp(d_grad),
                                             C.byref(as_prior(prior)), 1 if last else 0, 1 if adapt else 0, _dp(d_Xt),
                                             _dp(d_acc_out), _dp(d_step_out)))

    # -- adaptive sequential Monte Carlo on the AIS rows (pgl_smc_*; inference/batched_smc.py): d_state the AIS block of
    # K M rows, d_smc the per-neuron block of smc_state_doubles(K, M, P, S) doubles, S the number of stage records
    def smc_state_doubles(self, K, M, P, S):
        return int(self.lib.pgl_smc_state_doubles(int(K), int(M), int(P), int(S)))

    def _smc(self, d_state, d_smc, K, M, P, S):
        return (self.h, _dp(d_state), _dp(d_smc), int(K), int(M), int(P), int(S))

    def smc_init_dev(self, d_state, d_smc, K, M, P, S, n_lo, prior, step0, seed, d_Xt):
        _chk(self.lib.pgl_smc_init_dev(*self._smc(d_state, d_smc, K, M, P, S), int(n_lo), C.byref(as_prior(prior)),
                                       float(step0), int(seed) & 0xffffffffffffffff, _dp(d_Xt)))

    def smc_stage_dev(self, d_state, d_smc, K, M, P, S, prior, n_steps, cess, ess_min, delta_min, seed):
        _chk(self.lib.pgl_smc_stage_dev(*self._smc(d_state, d_smc, K, M, P, S), C.byref(as_prior(prior)), int(n_steps),
                                        float(cess), float(ess_min), float(delta_min), int(seed) & 0xffffffffffffffff))

    def smc_gather_dev(self, d_state, d_smc, K, M, P, S, prior):
        _chk(self.lib.pgl_smc_gather_dev(*self._smc(d_state, d_smc, K, M, P, S), C.byref(as_prior(prior))))

    def smc_begin_dev(self, d_state, d_smc, K, M, P, S, d_minv, d_Xt):
        _chk(self.lib.pgl_smc_begin_dev(*self._smc(d_state, d_smc, K, M, P, S), _dp(d_minv), _dp(d_Xt)))

    def smc_leap_dev(self, d_state, d_smc, K, M, P, S, d_minv, d_ll, d_grad, prior, last, d_Xt):
        _chk(self.lib.pgl_smc_leap_dev(*self._smc(d_state, d_smc, K, M, P, S), _dp(d_minv), _dp(d_ll), _dp(d_grad),
                                       C.byref(as_prior(prior)), 1 if last else 0, _dp(d_Xt)))

    def smc_dense_begin_dev(self, d_state, d_smc, K, M, P, S, d_W, d_Xt):
        _chk(self.lib.pgl_smc_dense_begin_dev(*self._smc(d_state, d_smc, K, M, P, S), _dp(d_W), _dp(d_Xt)))

    def smc_dense_leap_dev(self, d_state, d_smc, K, M, P, S, d_W, d_ll, d_grad, prior, last, d_Xt):
        _chk(self.lib.pgl_smc_dense_leap_dev(*self._smc(d_state, d_smc, K, M, P, S), _dp(d_W), _dp(d_ll), _dp(d_grad),
                                             C.byref(as_prior(prior)), 1 if last else 0, _dp(d_Xt)))

    def sync(self):
        _chk(self.lib.pgl_sync(self.h))

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        _chk(self.lib.pgl_last_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_kernels(self):
        """The fused kernel instantiations the last ll_grad / gibbs_prepare_all / hvp_* / hess call launched, in launch order, as
        plan_kernels names them (pgl_last_kernels); needs set_option(OPT_RECORD_KERNELS, 1).  gibbs_ll_cols / gibbs_update_cols
        append the k_gibbs_* kernels they launch; set_option(OPT_RECORD_KERNELS, 1) clears the record."""
        buf = C.create_string_buffer(16384)
        _chk(self.lib.pgl_last_kernels(self.h, buf, 16384))
        return [ln for ln in buf.value.decode().splitlines() if ln]

    def gibbs_last_geometry(self):
        """Launch geometry of the last recorded gibbs_ll_cols call (pgl_gibbs_last_geometry), as a dict."""
        v = np.zeros(10, dtype=np.int32)
        _chk(self.lib.pgl_gibbs_last_geometry(self.h, _ptr(v), 10))
        keys = ['path', 'CP', 'nsplit', 'ygroups', 'nloop', 'nblk', 'sblk', 'same_pre', 'gtb', 'rows']
        return dict(zip(keys, (int(x) for x in v)))

    def timing_summary(self, reset=True):
        """(n_launches, mean fused-kernel ms, mean whole-call ms) since the last reset."""
        n, a, b = C.c_int(), C.c_double(), C.c_double()
        _chk(self.lib.pgl_timing_summary(self.h, 1 if reset else 0, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def set_stream(self, stream_ptr):
        """Order the handle's work on a caller-owned HIP stream (integer hipStream_t of a
        torch.cuda.Stream(): `.cuda_stream`); None returns to the handle's own stream.
        The NULL stream cannot be named through this call (pgl_set_stream(NULL) means "own stream"):
        torch's DEFAULT stream has handle 0, so `torch.cuda.current_stream().cuda_stream` is only
        valid inside `with torch.cuda.stream(torch.cuda.Stream())` -- a 0 raises instead of silently
        un-ordering the kernels from the caller's collectives."""
        if stream_ptr is None:
            _chk(self.lib.pgl_set_stream(self.h, None))
            return
        if int(stream_ptr) == 0:
            raise ValueError("stream handle 0 is the NULL stream: create a torch.cuda.Stream(), make it "
                             "current and pass its .cuda_stream")
        _chk(self.lib.pgl_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    def info(self, n_lo=0, n_hi=None):
        n_hi = self.N if n_hi is None else n_hi
        v = np.zeros(13)
        _chk(self.lib.pgl_info(self.h, int(n_lo), int(n_hi), _ptr(v), 13))
        keys = ['blocks', 'threads', 'chunks', 'ktiles', 'lds_bytes', 'tile_rows', 'flops',
                'bytes', 'events', 'kernel_version', 'resident_feature_bytes', 'streamed_bytes', 'stim_path']
        return dict(zip(keys, v.tolist()))

    # -- direct-form helpers --------------------------------------------------
    def features(self):
        out = np.empty((self.nT, self.N, self.B))
        _chk(self.lib.pgl_features(self.h, _ptr(out)))
        return out

    def impulse_currents(self, w):
        w = _f64(w, (self.N, self.B))
        out = np.empty((self.nT, self.N))
        _chk(self.lib.pgl_impulse_currents(self.h, _ptr(w), _ptr(out)))
        return out

    def state(self, n, theta_n, Weff_col):
        th = _f64(theta_n, (self.P,))
        wc = _f64(Weff_col, (self.N,))
        lam = np.empty(self.nT)
        inet = np.empty(self.nT)
        istim = np.empty(self.nT)
        _chk(self.lib.pgl_state(self.h, int(n), _ptr(th), _ptr(wc), _ptr(lam), _ptr(inet),
                                _ptr(istim)))
        return lam, inet, istim

    def ll_from_current(self, n_post, I_bias, I_stim, I_other, I_col, ws):
        ws = _f64(np.atleast_1d(ws))
        I_other = _f64(I_other, (self.nT,))
        I_col = _f64(I_col, (self.nT,))
        I_stim = None if I_stim is None else _f64(I_stim, (self.nT,))
        out = np.empty(len(ws))
        _chk(self.lib.pgl_ll_from_current(self.h, int(n_post), float(I_bias), _ptr(I_stim),
                                          _ptr(I_other), _ptr(I_col), _ptr(ws), len(ws),
                                          _ptr(out)))
        return out

    def gibbs_prepare(self, n_post, theta_n, Weff_col):
        th = _f64(theta_n, (self.P,))
        wc = _f64(Weff_col, (self.N,))
        _chk(self.lib.pgl_gibbs_prepare(self.h, int(n_post), _ptr(th), _ptr(wc)))

    def gibbs_ll(self, n_pre, aw_cur, ws):
        ws = _f64(np.atleast_1d(ws))
        out = np.empty(len(ws))
        _chk(self.lib.pgl_gibbs_ll(self.h, int(n_pre), float(aw_cur), _ptr(ws), len(ws),
                                   _ptr(out)))
        return out

    def gibbs_update(self, n_pre, delta):
        _chk(self.lib.pgl_gibbs_update(self.h, int(n_pre), float(delta)))

    # -- batched column Gibbs (all post-synaptic columns resident) ---------------
    def gibbs_prepare_all(self, theta, Weff):
        th, We = self._draw(theta, Weff)
        _chk(self.lib.pgl_gibbs_prepare_all(self.h, _ptr(th), _ptr(We)))

    def gibbs_ll_cols(self, n_post, n_pre, aw_cur, ws):
        """ll (ncols, K) at the candidate weights ws (ncols, K) of the pairs (n_pre[c], n_post[c])."""
        n_post = np.ascontiguousarray(n_post, dtype=np.int32)
        n_pre = np.ascontiguousarray(n_pre, dtype=np.int32)
        ws = _f64(ws)
        if ws.ndim == 1:
            ws = ws[None, :]
        aw = _f64(aw_cur, (len(n_post),))
        if n_pre.shape != n_post.shape or ws.shape[0] != len(n_post):
            raise ValueError("n_post, n_pre, aw_cur, ws must describe the same columns")
        out = np.empty(ws.shape)
        K = ws.shape[1]
        for k0 in range(0, K, 16):                     # at most 16 candidate weights per launch
            wk = np.ascontiguousarray(ws[:, k0:k0 + 16])
            ok = np.empty(wk.shape)
            _chk(self.lib.pgl_gibbs_ll_cols(self.h, len(n_post), _ptr(n_post), _ptr(n_pre), _ptr(aw),
                                            _ptr(wk), wk.shape[1], _ptr(ok)))
            out[:, k0:k0 + 16] = ok
        return out

    def gibbs_update_cols(self, n_post, n_pre, delta):
        n_post = np.ascontiguousarray(n_post, dtype=np.int32)
        n_pre = np.ascontiguousarray(n_pre, dtype=np.int32)
        d = _f64(delta, (len(n_post),))
        if len(n_post) == 0:
            return
        _chk(self.lib.pgl_gibbs_update_cols(self.h, len(n_post), _ptr(n_post), _ptr(n_pre), _ptr(d)))

    def gibbs_currents(self, n_post, nrows=None):
        out = np.empty(self.nT if nrows is None else int(nrows))
        _chk(self.lib.pgl_gibbs_currents(self.h, int(n_post), _ptr(out)))
        return out
