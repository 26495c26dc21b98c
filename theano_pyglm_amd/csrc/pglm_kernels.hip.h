// Device kernels of the population-GLM likelihood library (gfx950 / CDNA4 only).
//
// Reference arithmetic (slinderman/theano_pyglm):
//   features   fS[t,n',b] = sum_{tau=1..R} S[t-tau,n'] ibasis[tau-1,b]   pyglm/utils/basis.py:201-236
//   currents   x[t,n] = bias_n + fstim[t,:].wstim_n + sum_{n',b} fS[t,n',b] w_n[n',b] Weff[n',n]
//                                                                         pyglm/glm.py:31-45, impulse.py:58
//   likelihood ll_n = sum_t ( -dt*lam + log(lam)*S[t,n] ),  lam = nlin(x)   pyglm/glm.py:52, nlin.py:25,43
//   gradient   T.grad(glm.ll, [bias, w_stim, w_ir])                        pyglm/inference/coord_descent.py:27-30
//
// Design.  The likelihood and its gradient are two dense contractions around an
// elementwise rate epilogue:  X = F.Wmat  (forward), r = dll/dx, G += F^T.r  (backward), all on
// v_mfma_f64_16x16x4_f64; the forward accumulator layout IS the B-operand layout of the backward
// MFMA, so r never leaves its registers in between.  Work is cut into 16-row time tiles; a
// workgroup walks a chunk of tiles with G in registers.  Three kernel families share that scheme:
//   k_build_fimg + k_fused5  F resident in HBM as LDS-shaped tiles (built once per data set, like the
//                            reference's data['fS']) and streamed with LDS-DMA; two passes over the
//                            chunk because G of 128 post neurons (655 KB) exceeds one CU's registers
//   k_fused3                 the same two passes, F tile regenerated in LDS from the spike events
//   k_fused2                 one pass, post tiles x K slices across the 8 waves (small post blocks,
//                            the sliced path for N > 128, optional f32 feature tile)
// Hessian-vector products H.v = F^T.(c o (F.v)) reuse the scheme with the epilogue swapped for one multiply (k_hvp5).
// The dense Hessian H = F^T.diag(c).F is a contraction over time of its own (k_hess, pglm_hess.hip.h).
// Posterior sampling runs HMC chains of all neurons in lock step around the ll+grad launch (k_hmc_*, pglm_hmc.hip.h).
// A dense mass matrix adds two batched triangular matrix-vector products per leapfrog step (k_tri_matvec, pglm_hmc_dense.hip.h).
// The No-U-Turn sampler runs on the same launch and products with rows that do not wait for each other (k_nuts_*, pglm_nuts.hip.h).
// The Laplace posterior factors and inverts the dense Hessians in place, one workgroup per matrix (k_chol_factor, k_tri_inverse,
// pglm_chol.hip.h).
// The dense Newton fit solves against that factor (k_chol_solve) between its row kernels (k_newton_*, pglm_newton.hip.h).
// The per-neuron evidence comes from annealed importance sampling on the same moves (k_ais_*, pglm_ais.hip.h).
// Its dense mass shares one read of a neuron's factor among the neuron's particles (k_tri_matvec_shared, pglm_ais_dense.hip.h).
// Adaptive sequential Monte Carlo walks the same tempered path with per-neuron ladders and resampling on the device (k_smc_*,
// pglm_smc.hip.h).
// The group-lasso MAP runs accelerated proximal gradient fits of all neurons in lock step around the same launch (k_prox_*,
// pglm_prox.hip.h).
// Simulation produces spikes instead of reading them: one workgroup per replicate runs the time loop (k_simulate,
// pglm_simulate.hip.h).
// Rescaled intervals, the pointwise ll and the rate windows below sweep the forward-only pass's currents once, a thread per
// (time unit, neuron) next to the neuron's event list: one source struct and one walk (pgl_bin_walk, pglm_binwalk.hip.h).
// Model comparison needs the log-likelihood of a draw resolved in time: block sums behind the forward-only pass, folded over
// the draws on the device (k_pw_chunk, k_pw_block, pglm_pointwise.hip.h).
// Firing-rate bands and windowed predictive residuals need the expected and observed counts over user-chosen time windows,
// folded over the draws the same way (k_rw_piece, k_rw_window, pglm_ratewin.hip.h).
// The goodness of fit is finished on the device: the discrete-time correction of the event bin's term in the rescaled
// intervals, and the KS distance of every neuron's intervals by a sorting network, one workgroup per segment (k_rcorr_*,
// k_ks_segment, pglm_gof.hip.h); the independence of those intervals -- the serial correlation of their normal scores, lag by
// lag, with run boundaries between the data sequences -- is one workgroup per segment as well (k_acf_segment, pglm_acf.hip.h).
// PSIS-LOO takes the matrix of those terms over the draws one column per workgroup: ranks, generalized-Pareto fit, smoothed
// weights (k_psis_column, pglm_psis.hip.h).
// The couplings are tested from the factor of the Laplace covariance: one wave per group of B weights forms the group's
// block of the covariance and its Wald statistic (k_wald_groups, pglm_wald.hip.h).
// The samplers' draws are judged the same way, one column of (chains x draws) per workgroup: ranks by counting, normal scores,
// split-R-hat, autocovariances in batches of lags and Geyer's sequence (k_diag_column, pglm_diag.hip.h).
// The same draws become the filters with their uncertainty, one (group of B weights, row) per workgroup: the curve of every
// draw lag by lag, moments in a fixed order, quantiles from a sorting network in LDS, a simultaneous band (k_filter_bands,
// pglm_filters.hip.h).
// The clamped simulation holds the other neurons at their recorded spikes: the chains (replicate, neuron) decouple, one wave
// per (neuron, 64 replicates) with the self-history in a per-lane queue (k_cond_currents, k_simulate_cond, pglm_condsim.hip.h).
// Decoding turns the question round: the MAP stimulus given the spikes.  The objective, its gradient and its Hessian-vector
// products with respect to the stimulus are the adjoint pair of the feature build, two convolutions over (nT, N) around the
// rate and curvature functions (k_dec_forward, k_dec_backward, pglm_decode.hip.h).
#pragma once
//
// The kernels live in one header per family; this file is the translation unit's table of contents.
#include "pglm_common.hip.h"
#include "pglm_fused_stream.hip.h"
#include "pglm_fused_resident.hip.h"
#include "pglm_hvp.hip.h"
#include "pglm_hess.hip.h"
#include "pglm_reduce.hip.h"
#include "pglm_direct.hip.h"
#include "pglm_gibbs.hip.h"
#include "pglm_stim.hip.h"
#include "pglm_bfgs.hip.h"
#include "pglm_rowsearch.hip.h"
#include "pglm_ncg.hip.h"
#include "pglm_newton.hip.h"
#include "pglm_hmc.hip.h"
#include "pglm_hmc_dense.hip.h"
#include "pglm_adapt.hip.h"
#include "pglm_nuts.hip.h"
#include "pglm_chol.hip.h"
#include "pglm_ais.hip.h"
#include "pglm_ais_dense.hip.h"
#include "pglm_smc.hip.h"
#include "pglm_prox.hip.h"
#include "pglm_binwalk.hip.h"
#include "pglm_rescale.hip.h"
#include "pglm_gof.hip.h"
#include "pglm_acf.hip.h"
#include "pglm_pointwise.hip.h"
#include "pglm_ratewin.hip.h"
#include "pglm_psis.hip.h"
#include "pglm_wald.hip.h"
#include "pglm_diag.hip.h"
#include "pglm_filters.hip.h"
#include "pglm_simulate.hip.h"
#include "pglm_condsim.hip.h"
#include "pglm_decode.hip.h"
