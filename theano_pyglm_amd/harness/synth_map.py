"""
MAP fit on synthetic data -- counterpart of test/synth_map.py + test/synth_harness.py.

    python -m theano_pyglm_amd.harness.synth_map -d data.pkl -r out_dir [-m standard_glm] [--sequential]

The sweep over the neurons runs as the GPU lock-step optimizer by default (inference/batched_bfgs.py);
--sequential (batched=False) is the reference's loop of per-neuron scipy fits; --newton-cg runs the sweep as the GPU
lock-step Newton-CG optimizer on device Hessian-vector products (inference/batched_newton_cg.py; the reference's use_rop).
--newton runs the sweep as the GPU lock-step dense-Hessian Newton fit (inference/batched_newton.py; the reference's use_hessian).
--prox runs the sweep as the GPU lock-step proximal-gradient fit of the group-lasso MAP (inference/batched_prox.py) and prints
status, iterations and the number of non-zero presynaptic groups per neuron.
--gof prints the time-rescaling KS table of the fitted model (inference/gof.py) after the fit; --gof-correct applies the
discrete-time correction to it (a random function of its seed, 0).  With --hmc N or --nuts N, --gof-draws prints the KS
distance over the posterior draws per neuron (corrected; sorted and tested on the device).  --gof-lags L adds the independence
table (serial correlation of the normal scores at the lags 1 .. L, inference/gof.py) behind either.
--ppc N prints the predictive spike-count table of N replicates simulated from the fitted model (inference/predictive.py).
--cond-ppc N [WIN] prints the clamped predictive check of N replicates per neuron over windows of WIN bins (default 50): every
neuron simulated with its own spikes fed back and the other neurons held at their recorded spikes (inference/predictive.py:
conditional_counts) -- the largest |pearson| and its window, the KS distance of the pit values, the share of windows whose
observed count lies outside the replicates' [min, max].
--decode decodes the data set's own stimulus from its spikes under the fitted model (inference/decode.py: the MAP stimulus under
a Gaussian prior, --decode-sigma and --decode-rho) and prints F at the decoded and at the recorded stimulus and the correlation
of the two per stimulus dimension.
--hmc N draws N posterior samples of every neuron's parameters from the fit by lock-step HMC on the device
(inference/batched_hmc.py) and prints the bias posterior mean +- sd per neuron, beside the Laplace standard error when
the model's packing has one.
--nuts N does the same with the No-U-Turn sampler (inference/batched_nuts.py; --hmc-mass applies) and prints the same table
plus the median tree depth and the divergent transitions per neuron.
--ais K estimates every neuron's log evidence given the network from the fit by annealed importance sampling with K
particles on the device (inference/batched_ais.py; Gaussian impulse priors only) and prints log_Z + log_prior_norm +- se, the
ESS and the Laplace log evidence beside it.
--smc K does the same by adaptive sequential Monte Carlo (inference/batched_smc.py; --ais-mass applies): the table of --ais
without a standard error (one run gives none), plus the stages and the resamplings of every neuron.
--waic (with --hmc N or --nuts N) prints the WAIC table of those draws after them (inference/model_compare.py: the pointwise
log-likelihood of every draw in blocks of 10240 bins, accumulated on the device).
--loo (with --hmc N or --nuts N) prints the PSIS-LOO table of those draws: elpd_loo, p_loo, looic, se and the khat diagnostic
(model_compare.loo_glms: Pareto smoothing of the (draws, blocks, neurons) matrix on the device).
--rates WIN (with --hmc N or --nuts N) prints the windowed predictive residuals of those draws per neuron: the largest |pearson|
and its window, the KS distance of the pit values from the uniform law, and the share of windows whose observed count lies
outside the draws' [min, max] (inference/predictive.py: rate_bands over windows of WIN bins, folded over the draws on the device).
--diag (with --hmc N or --nuts N, N >= 8) prints the convergence diagnostics of those draws per neuron: the worst rank-normalised
R-hat, the smallest bulk and tail ESS, and the number of parameters with rhat > 1.01 or ess_bulk < 100 per chain
(inference/diagnostics.py: k_diag_column on the draws where the sampler keeps them).
--filters [LEVEL] (with --hmc N or --nuts N) prints the posterior bands of the impulse responses of those draws per neuron: the
presynaptic neurons whose simultaneous credible band excludes zero, the largest |effective weight| / sd and, against a true
model, the true / false positives (inference/filters.py: k_filter_bands on the draws where the sampler keeps them).
--coupling-test [ALPHA] prints, after the fit, the number of couplings that the per-pair Wald tests find at the false discovery
rate ALPHA (default 0.05; inference/connectivity.py) and, where the data carry the true model, the true- and false-positive
rates against the true adjacency and the area under the ROC of the statistic; --coupling-lr adds the median and maximum of
|lr1 - T| / max(T, 1), the check of the quadratic approximation.
"""
import argparse
import os
import pickle
import time

import numpy as np

from theano_pyglm_amd.inference.coord_descent import coord_descent
from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
from theano_pyglm_amd.population import Population


def initialize_test_harness(model_name, data, data_dir=None):
    """test/synth_harness.py:9-59."""
    model = make_model(model_name, N=data['N'], dt=0.001)
    stabilize_sparsity(model)
    popn = Population(model)
    popn.add_data(data)
    popn_true, x_true = None, None
    if 'vars' in data and data_dir is not None and os.path.exists(os.path.join(data_dir, 'model.pkl')):
        x_true = data['vars']
        with open(os.path.join(data_dir, 'model.pkl'), 'rb') as f:
            model_true = pickle.load(f)
        popn_true = Population(model_true)
        popn_true.add_data(data)
        print("true LL: %f" % popn_true.compute_log_p(x_true))
    return popn, popn_true, x_true


def run_synth_test(model_name, data, results_dir, data_dir=None, batched=None, rng=None, use_rop=False, gof=False, ppc=0, hmc=0, ais=0,
                   hmc_mass='laplace', prox=False, laplace_device=False, ais_mass='laplace', nuts=0, smc=0, newton=False, waic=False, loo=False, diag=False, rates=0,
                   gof_correct=False, gof_draws=False, gof_lags=0, coupling_test=None, coupling_lr=False, filters=None, cond_ppc=None, decode=None):
    """test/synth_map.py:10-32."""
    popn, popn_true, x_true = initialize_test_harness(model_name, data, data_dir)
    x0 = popn.sample(rng)
    print("LL0: %f" % popn.compute_log_p(x0))
    t0 = time.time()
    x_inf = coord_descent(popn, x0=x0, maxiter=1, batched=batched, use_rop=use_rop, prox=prox, newton=newton)
    wall = time.time() - t0
    if prox:
        print(prox_table(popn, x_inf))
    ll_inf = popn.compute_log_p(x_inf)
    print("LL_inf: %f   (MAP wall-clock %.2f s)" % (ll_inf, wall))
    if results_dir is not None:
        with open(os.path.join(results_dir, 'results.pkl'), 'wb') as f:
            pickle.dump(x_inf, f, protocol=-1)
    if gof:
        from theano_pyglm_amd.inference.gof import ks_time_rescaling, format_table
        print(format_table(ks_time_rescaling(popn, x_inf, correct=True) if gof_correct else ks_time_rescaling(popn, x_inf)))
        if gof_lags:
            from theano_pyglm_amd.inference.gof import independence_time_rescaling, format_independence_table
            print(format_independence_table(independence_time_rescaling(popn, x_inf, max_lag=gof_lags, correct=gof_correct)))
    if coupling_test is not None:
        print(coupling_table(popn, x_inf, coupling_test, coupling_lr, popn_true, x_true))
    if ppc:
        from theano_pyglm_amd.inference import predictive
        print(predictive.format_table(predictive.predictive_counts(popn, x_inf, ppc)))
    if cond_ppc:
        print(cond_ppc_table(popn, x_inf, cond_ppc))
    if decode:
        print(decode_table(popn, x_inf, *decode))
    if hmc:
        print(hmc_bias_table(popn, x_inf, hmc, hmc_mass, laplace_device, waic=waic, loo=loo, diag=diag, rates=rates, gof_draws=gof_draws, gof_lags=gof_lags,
                             filters=filters, truth=true_adjacency(popn_true, x_true)))
    if nuts:
        print(nuts_bias_table(popn, x_inf, nuts, hmc_mass, laplace_device, waic=waic, loo=loo, diag=diag, rates=rates, gof_draws=gof_draws, gof_lags=gof_lags,
                              filters=filters, truth=true_adjacency(popn_true, x_true)))
    if ais:
        print(ais_evidence_table(popn, x_inf, ais, laplace_device, ais_mass))
    if smc:
        print(smc_evidence_table(popn, x_inf, smc, laplace_device, ais_mass))
    return x_inf, ll_inf, wall


def true_adjacency(popn_true, x_true):
    """truth[post, pre] of the true model, or None without one: a coupling is there where W_eff[pre, post] is not zero"""
    import numpy as np
    if popn_true is None or x_true is None:
        return None
    return (np.asarray(popn_true.W_eff(x_true)) != 0.0).T


def coupling_table(popn, x, alpha=0.05, one_step_lr=False, popn_true=None, x_true=None):
    """connectivity.format_table of the per-pair Wald tests at x; with the true model, against its adjacency (a coupling is
    there where the true effective weight W_eff[pre, post] is not zero)."""
    import numpy as np
    from theano_pyglm_amd.inference import connectivity
    t0 = time.time()
    res = connectivity.coupling_tests(popn, x, alpha=alpha, one_step_lr=one_step_lr)
    truth = None
    if popn_true is not None and x_true is not None:
        truth = (np.asarray(popn_true.W_eff(x_true)) != 0.0).T                 # [post, pre]
    return connectivity.format_table(res, alpha, truth) + "\n(coupling tests in %.2f s)" % (time.time() - t0)


def prox_table(popn, x):
    """One line per neuron from the last proximal-gradient sweep: status, iterations, evaluations and the number of
    presynaptic groups of x that are not exactly at the prior's mu."""
    import numpy as np
    per = popn.last_fit_stats['per_neuron']
    mu = float(popn.glm.imp_model.prior.mu)
    lines = ["neuron  status  iters   nfev  non-zero groups (of %d)" % popn.N]
    for n in range(popn.N):
        w = np.asarray(x['glms'][n]['imp']['w_ir'], dtype=float).reshape(popn.N, -1)
        lines.append("%6d  %6d  %5d  %5d  %6d" % (n, per['status'][n], per['iters'][n], per['nfev'][n],
                                                int(np.sum(np.any(w != mu, axis=1)))))
    return "\n".join(lines)


def hmc_bias_table(popn, x, n_draws, mass='laplace', laplace_device=False, waic=False, loo=False, diag=False, rates=0,
                   gof_draws=False, gof_lags=0, filters=None, truth=None):
    """n_draws kept HMC draws from x with the mass matrix `mass` ('laplace' or 'laplace_dense'): one line per neuron, bias
    posterior mean +- sd (and the Laplace standard error).  laplace_device: the Laplace factorisations (the dense mass
    matrix and the standard errors) run on the device.  waic / loo: the WAIC / PSIS-LOO table of the draws follows (waic_table, loo_table); diag: the convergence table
    (diagnostics.worst_table of the sampler's 'summary'); filters: a level -- the table of the posterior bands of the impulse
    responses follows (filters.band_table of the sampler's 'filters', against truth[post, pre] where given)."""
    from theano_pyglm_amd.inference import batched_hmc
    from theano_pyglm_amd.inference.laplace import laplace_glms
    t0 = time.time()
    res = batched_hmc.sample_glms_hmc(popn, x, n_draws, mass=mass,
                                      factor_on_device=laplace_device and mass == 'laplace_dense', diagnostics=diag,
                                      filters=filters if filters is not None else False)
    wall = time.time() - t0
    s = batched_hmc.summarize(res['samples'][:, :, 0])
    try:
        se = [r['stderr_vec'][0] if r['pd'] else float('nan') for r in laplace_glms(popn, x, device=laplace_device)]
    except ValueError:
        se = None
    lines = ["HMC%s: %d draws per neuron in %.2f s (%d ll+grad launches)"
             % ("" if mass == 'laplace' else " (mass=%s)" % mass, n_draws, wall, res['n_evals']),
             "neuron   bias mean +- sd        ESS  accept   step" + ("   Laplace se" if se is not None else "")]
    for n in range(popn.N):
        ln = "%6d  %9.4f +- %-8.4f %6.0f  %6.2f  %6.4f" % (n, s['mean'][n], s['sd'][n], s['ess'][n], res['accept_rate'][n],
                                                          res['step_sz'][n])
        lines.append(ln + ("   %10.4f" % se[n] if se is not None else ""))
    if gof_draws:
        lines.append(gof_draws_table(popn, x, res['samples'], gof_lags))
    if waic:
        lines.append(waic_table(popn, x, res['samples']))
    if loo:
        lines.append(loo_table(popn, x, res['samples']))
    if rates:
        lines.append(rates_table(popn, x, res['samples'], rates))
    if diag:
        from theano_pyglm_amd.inference.diagnostics import worst_table
        lines.append(worst_table(res['summary'], res['samples'].shape[0] if res['samples'].ndim == 4 else 1))
    if filters is not None:
        from theano_pyglm_amd.inference.filters import band_table
        lines.append(band_table(res['filters'], truth=truth))
    return "\n".join(lines)


def nuts_bias_table(popn, x, n_draws, mass='laplace', laplace_device=False, waic=False, loo=False, diag=False, rates=0,
                    gof_draws=False, gof_lags=0, filters=None, truth=None, **kw):
    """hmc_bias_table with the No-U-Turn sampler: the same columns ('accept' is the mean acceptance statistic after
    warm-up) plus the median tree depth of the kept transitions and the divergent transitions after warm-up.  kw: further
    arguments of sample_glms_nuts (n_warmup, max_depth, ...).  waic / loo: the WAIC / PSIS-LOO table of the draws follows (waic_table, loo_table); diag: the convergence table
    (diagnostics.worst_table of the sampler's 'summary'); filters, truth: as hmc_bias_table."""
    import numpy as np
    from theano_pyglm_amd.inference import batched_nuts
    from theano_pyglm_amd.inference.laplace import laplace_glms
    t0 = time.time()
    res = batched_nuts.sample_glms_nuts(popn, x, n_draws, mass=mass,
                                        factor_on_device=laplace_device and mass == 'laplace_dense', diagnostics=diag,
                                        filters=filters if filters is not None else False, **kw)
    wall = time.time() - t0
    s = batched_nuts.summarize(res['samples'][:, :, 0])
    try:
        se = [r['stderr_vec'][0] if r['pd'] else float('nan') for r in laplace_glms(popn, x, device=laplace_device)]
    except ValueError:
        se = None
    depth = np.median(res['depth'], axis=0)
    lines = ["NUTS%s: %d draws per neuron in %.2f s (%d ll+grad launches, %d idle row evaluations; median depth %g, "
             "%d divergent transitions)" % ("" if mass == 'laplace' else " (mass=%s)" % mass, n_draws, wall, res['n_evals'],
                                           res['idle_row_evaluations'], np.median(res['depth']), res['divergent'].sum()),
             "neuron   bias mean +- sd        ESS  accept   step  depth  divergent" + ("   Laplace se" if se is not None else "")]
    for n in range(popn.N):
        ln = "%6d  %9.4f +- %-8.4f %6.0f  %6.2f  %6.4f  %5g  %9d" % (n, s['mean'][n], s['sd'][n], s['ess'][n],
                                                                    res['accept_rate'][n], res['step_sz'][n], depth[n],
                                                                    res['divergent'][n])
        lines.append(ln + ("   %10.4f" % se[n] if se is not None else ""))
    if gof_draws:
        lines.append(gof_draws_table(popn, x, res['samples'], gof_lags))
    if waic:
        lines.append(waic_table(popn, x, res['samples']))
    if loo:
        lines.append(loo_table(popn, x, res['samples']))
    if rates:
        lines.append(rates_table(popn, x, res['samples'], rates))
    if diag:
        from theano_pyglm_amd.inference.diagnostics import worst_table
        lines.append(worst_table(res['summary'], res['samples'].shape[0] if res['samples'].ndim == 4 else 1))
    if filters is not None:
        from theano_pyglm_amd.inference.filters import band_table
        lines.append(band_table(res['filters'], truth=truth))
    return "\n".join(lines)


def cond_ppc_table(popn, x, cond_ppc):
    """The clamped predictive check of --cond-ppc N [WIN]: N replicates of every neuron given the recorded spikes of the others,
    over windows of WIN bins (default 50), formatted like --rates."""
    from theano_pyglm_amd.inference import predictive
    n_rep, win = (list(cond_ppc) + [50])[:2]
    return predictive.format_cond_table(predictive.conditional_counts(popn, x, n_rep=n_rep, win=win))


def rates_table(popn, x, samples, win):
    """The windowed predictive residuals of posterior draws (samples (S, N, P) of all neurons) over windows of `win` bins:
    predictive.format_rate_table of predictive.rate_bands."""
    from theano_pyglm_amd.inference import predictive
    t0 = time.time()
    res = predictive.rate_bands(popn, x, samples, win=win)
    return predictive.format_rate_table(res) + "\n(rate bands of %d draws in %.2f s)" % (res['n_draws'], time.time() - t0)


def gof_draws_table(popn, x, samples, gof_lags=0):
    """The time-rescaling KS distance over posterior draws (samples (S, N, P) of all neurons), discrete-time corrected; with
    gof_lags the independence statistic of the same draws behind it."""
    from theano_pyglm_amd.inference import gof
    t0 = time.time()
    res = gof.ks_time_rescaling_draws(popn, x, samples)
    out = gof.format_draws_table(res) + "\n(KS distance of %d draws in %.2f s)" % (res['n_draws'], time.time() - t0)
    if gof_lags:
        t0 = time.time()
        ind = gof.independence_time_rescaling_draws(popn, x, samples, max_lag=gof_lags)
        out += "\n" + gof.format_independence_draws_table(ind) + "\n(serial correlation of %d draws in %.2f s)" % (ind['n_draws'], time.time() - t0)
    return out


def waic_table(popn, x, samples, block_chunks=40):
    """The WAIC table of posterior draws (samples (S, N, P) of all neurons, as the samplers return them) on the population's
    data, in blocks of 256 block_chunks bins."""
    from theano_pyglm_amd.inference import model_compare
    t0 = time.time()
    res = model_compare.waic_glms(popn, x, samples, block_chunks=block_chunks)
    return model_compare.format_table(res) + "\n(pointwise log-likelihood of %d draws in %.2f s)" % (res['n_draws'], time.time() - t0)


def loo_table(popn, x, samples, block_chunks=40):
    """The PSIS-LOO table of posterior draws (samples (S, N, P) of all neurons) on the population's data, in blocks of 256
    block_chunks bins: the matrix of pointwise terms stays on the device (model_compare.loo_glms)."""
    from theano_pyglm_amd.inference import model_compare
    t0 = time.time()
    res = model_compare.loo_glms(popn, x, samples, block_chunks=block_chunks)
    return model_compare.format_table(res) + "\n(pointwise log-likelihood and PSIS of %d draws in %.2f s)" % (res['n_draws'], time.time() - t0)


def ais_evidence_table(popn, x, n_particles, laplace_device=False, mass='laplace'):
    """AIS with n_particles particles per neuron from x: one line per neuron, log_Z + log_prior_norm +- se, the ESS and the
    Laplace log evidence (both under the host priors, which drop their normalising constants).  mass: 'none' (identity),
    'laplace' or 'laplace_dense' (the tempered dense mass)."""
    from theano_pyglm_amd.inference import batched_ais
    from theano_pyglm_amd.inference.laplace import laplace_glms
    t0 = time.time()
    res = batched_ais.ais_glms(popn, x, n_particles=n_particles, mass=None if mass == 'none' else mass)
    wall = time.time() - t0
    lap = [r['log_evidence'] for r in laplace_glms(popn, x, device=laplace_device)]
    lines = ["AIS%s: %d particles per neuron, %d temperatures in %.2f s (%d ll+grad launches)"
             % ("" if mass == 'laplace' else " (mass=%s)" % mass, n_particles, len(res['betas']), wall, res['n_evals']),
             "neuron   log evidence +- se           ESS      Laplace"]
    for n in range(popn.N):
        lines.append("%6d  %13.4f +- %-9.4f %6.1f  %11.4f" % (n, res['log_Z'][n] + res['log_prior_norm'][n], res['log_Z_se'][n],
                                                             res['ess'][n], lap[n]))
    return "\n".join(lines)


def smc_evidence_table(popn, x, n_particles, laplace_device=False, mass='laplace'):
    """Adaptive SMC with n_particles particles per neuron from x: one line per neuron, log_Z + log_prior_norm, the ESS of the
    final weights, the Laplace log evidence, the stages and the resamplings.  No standard error: one run gives none."""
    from theano_pyglm_amd.inference import batched_smc
    from theano_pyglm_amd.inference.laplace import laplace_glms
    t0 = time.time()
    res = batched_smc.smc_glms(popn, x, n_particles=n_particles, mass=None if mass == 'none' else mass)
    wall = time.time() - t0
    lap = [r['log_evidence'] for r in laplace_glms(popn, x, device=laplace_device)]
    lines = ["SMC%s: %d particles per neuron, up to %d stages in %.2f s (%d ll+grad launches, %.0f %% of row evaluations idle)"
             % ("" if mass == 'laplace' else " (mass=%s)" % mass, n_particles, res['betas'].shape[0], wall, res['n_evals'],
                100.0 * res['idle_row_evaluations']),
             "neuron   log evidence      ESS      Laplace  stages  resampled"]
    for n in range(popn.N):
        lines.append("%6d  %13.4f  %6.1f  %11.4f  %6d  %9d%s"
                     % (n, res['log_Z'][n] + res['log_prior_norm'][n], res['ess'][res['n_stages'][n] - 1, n], lap[n],
                        res['n_stages'][n], res['n_resampled'][n], "" if res['finished'][n] else "  (unfinished)"))
    return "\n".join(lines)


def decode_table(popn, x, sigma=1.0, rho=np.inf):
    """The lines of --decode: the MAP stimulus of the current data given its spikes and the fitted parameters."""
    from theano_pyglm_amd.inference.decode import decode_stimulus
    stim = np.asarray(popn._current['stim'], dtype=float)
    stim = stim[:, None] if stim.ndim == 1 else stim
    res = decode_stimulus(popn, x, sigma=sigma, rho=rho)
    F_rec = popn.compute_stimulus_ll_grad(x, stim, sigma=sigma, rho=rho)[0]
    lines = ["stimulus decoding (%s; sigma = %g, rho = %g): status %d, max |grad| = %.2e, %d evaluations, %d products"
             % (res['route'], sigma, rho, res['status'], res['grad_max'], res['n_eval'], res['n_hvp']),
             "  F at the decoded stimulus   %.6f  (log lik %.6f, log prior %.6f)" % (res['F'], res['log_lik'], res['log_prior']),
             "  F at the recorded stimulus  %.6f  (log lik %.6f, log prior %.6f)" % (F_rec[0], F_rec[1], F_rec[2])]
    for d in range(stim.shape[1]):
        a, b = res['stim'][:, d], stim[:, d]
        r = float(np.corrcoef(a, b)[0, 1]) if np.std(a) > 0 and np.std(b) > 0 else float('nan')
        lines.append("  stimulus dimension %d: correlation of decoded and recorded %.4f" % (d, r))
    return "\n".join(lines)


class _CondPpc(argparse.Action):
    """--cond-ppc N [WIN]: one or two positive integers"""
    def __call__(self, ap, namespace, values, option_string=None):
        if len(values) > 2 or min(values) < 1:
            ap.error("--cond-ppc takes N [WIN]: one or two integers, each at least 1")
        setattr(namespace, self.dest, values)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('-m', '--model', default='standard_glm')
    ap.add_argument('-d', '--dataFile', required=True)
    ap.add_argument('-r', '--resultsDir', default='.')
    ap.add_argument('--sequential', action='store_true', help='per-neuron scipy fits (the reference loop)')
    ap.add_argument('--batched', action='store_true', help='(deprecated, no-op: the GPU lock-step sweep is the default)')
    ap.add_argument('--newton-cg', action='store_true',
                    help='lock-step Newton-CG on device Hessian-vector products instead of lock-step BFGS '
                         '(with --sequential: per-neuron scipy Newton-CG fits)')
    ap.add_argument('--newton', action='store_true',
                    help='lock-step dense-Hessian Newton on the device (Hessian contraction, batched Cholesky factor and '
                         'solve per outer iteration) instead of lock-step BFGS')
    ap.add_argument('--prox', action='store_true',
                    help='group-lasso MAP by lock-step proximal gradient on the device (exact zeros); prints status, '
                         'iterations and the non-zero groups per neuron')
    ap.add_argument('--gof', action='store_true',
                    help='after the fit: time-rescaling KS test of every neuron (rescaled inter-spike intervals against Exp(1))')
    ap.add_argument('--gof-correct', action='store_true',
                    help='with --gof: apply the discrete-time correction of Haslinger et al. (2010); the table is then a random '
                         'function of the seed (0)')
    ap.add_argument('--gof-lags', type=int, default=0, metavar='L',
                    help='with --gof: the independence table as well -- serial correlation of the normal scores of the rescaled '
                         'intervals at the lags 1 .. L (at most 64) and the portmanteau p-value; honours --gof-correct; with '
                         '--gof-draws the same over the posterior draws')
    ap.add_argument('--gof-draws', action='store_true',
                    help='with --hmc N / --nuts N: the time-rescaling KS distance of every posterior draw (corrected), sorted and '
                         'tested on the device; prints mean, 5 %% and 95 %% quantiles and the share of draws inside the band')
    ap.add_argument('--ppc', type=int, default=0, metavar='N',
                    help='after the fit: predictive spike counts of N replicates simulated from the fitted model on the device')
    ap.add_argument('--cond-ppc', type=int, nargs='+', default=None, metavar='N', action=_CondPpc,
                    help='N [WIN]: after the fit, the clamped predictive check of N replicates per neuron over windows of WIN bins '
                         '(default 50): each neuron simulated on the device given the recorded spikes of the others')
    ap.add_argument('--decode', action='store_true',
                    help="after the fit: decode the data set's own stimulus from its spikes on the device (a 'basis' stimulus)")
    ap.add_argument('--decode-sigma', type=float, default=1.0, help='standard deviation of the decoding prior (default 1)')
    ap.add_argument('--decode-rho', type=float, default=float('inf'),
                    help='scale of the first differences in the decoding prior (default inf: iid)')
    ap.add_argument('--hmc', type=int, default=0, metavar='N',
                    help='after the fit: N posterior draws per neuron by lock-step HMC on the device; prints the bias mean +- sd')
    ap.add_argument('--nuts', type=int, default=0, metavar='N',
                    help='after the fit: N posterior draws per neuron by the No-U-Turn sampler on the device; prints the table '
                         'of --hmc plus the median tree depth and the divergent transitions')
    ap.add_argument('--hmc-mass', choices=['laplace', 'laplace_dense', 'adapt'], default='laplace',
                    help="mass matrix of --hmc and --nuts: 1 / diag A ('laplace'), the full Laplace covariance ('laplace_dense') "
                         "or a diagonal one learned during the warm-up ('adapt')")
    ap.add_argument('--ais', type=int, default=0, metavar='K',
                    help='after the fit: log evidence of every neuron given the network by annealed importance sampling with '
                         'K particles on the device, beside the Laplace log evidence (Gaussian impulse priors only)')
    ap.add_argument('--smc', type=int, default=0, metavar='K',
                    help='after the fit: log evidence of every neuron by adaptive sequential Monte Carlo with K particles on the '
                         'device (per-neuron ladders, resampling; --ais-mass applies), with stages and resamplings per neuron')
    ap.add_argument('--ais-mass', choices=['none', 'laplace', 'laplace_dense'], default='laplace',
                    help="mass matrix of --ais: identity ('none'), 1 / diag A ('laplace') or the tempered dense mass, the factor "
                         "of (beta G + Lambda)^-1 at every temperature ('laplace_dense')")
    ap.add_argument('--laplace-device', action='store_true',
                    help='the Laplace factorisations behind --hmc (standard errors, and the factor of --hmc-mass laplace_dense) '
                         'and --ais run on the device (batched Cholesky and triangular inverse) instead of on the host')
    ap.add_argument('--waic', action='store_true',
                    help='with --hmc N or --nuts N: the WAIC of every neuron from those draws (pointwise log-likelihood in blocks '
                         'of 10240 bins, accumulated over the draws on the device)')
    ap.add_argument('--rates', type=int, default=0, metavar='WIN',
                    help='with --hmc N or --nuts N: windowed predictive residuals of those draws per neuron over windows of WIN '
                         'bins (largest |pearson|, KS distance of the pit values, share of windows outside the band)')
    ap.add_argument('--diag', action='store_true',
                    help='with --hmc N or --nuts N: rank-normalised R-hat and bulk / tail ESS of those draws per neuron, computed '
                         'on the device (inference/diagnostics.py)')
    ap.add_argument('--loo', action='store_true',
                    help='with --hmc N or --nuts N: PSIS-LOO of every neuron from those draws, with the khat diagnostic per '
                         'block (the matrix of pointwise terms stays on the device; beside or instead of --waic)')
    ap.add_argument('--coupling-test', type=float, nargs='?', const=0.05, default=None, metavar='ALPHA',
                    help='after the fit: per-pair Wald tests of the couplings with Benjamini-Hochberg control at ALPHA (default '
                         '0.05); with the true model in the data, true- and false-positive rates and the area under the ROC')
    ap.add_argument('--filters', type=float, nargs='?', const=0.95, default=None, metavar='LEVEL',
                    help='with --hmc N or --nuts N: the posterior bands of the impulse responses from those draws on the device '
                         '(inference/filters.py): per neuron the presynaptic neurons whose simultaneous band at LEVEL (default '
                         '0.95) excludes zero, the largest |effective weight| / sd, and against a true model the true / false '
                         'positives')
    ap.add_argument('--coupling-lr', action='store_true',
                    help='with --coupling-test: the one-step likelihood ratio beside the Wald statistic, median and maximum of '
                         '|lr1 - T| / max(T, 1)')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    with open(args.dataFile, 'rb') as f:
        data = pickle.load(f)
    run_synth_test(args.model, data, args.resultsDir, os.path.dirname(args.dataFile),
                   False if args.sequential else ('torch' if args.newton_cg else None), use_rop=args.newton_cg, gof=args.gof, ppc=args.ppc, hmc=args.hmc, ais=args.ais,
                   hmc_mass=args.hmc_mass, prox=args.prox, laplace_device=args.laplace_device, ais_mass=args.ais_mass, nuts=args.nuts, smc=args.smc,
                   newton=args.newton, waic=args.waic, loo=args.loo, diag=args.diag, rates=args.rates,
                   gof_correct=args.gof_correct, gof_draws=args.gof_draws, gof_lags=args.gof_lags,
                   coupling_test=args.coupling_test, coupling_lr=args.coupling_lr, filters=args.filters,
                   cond_ppc=args.cond_ppc, decode=(args.decode_sigma, args.decode_rho) if args.decode else None)


if __name__ == '__main__':
    main()
