"""Posterior bands of the coupling and stimulus filters from the samplers' draws: the curves h(tau) = sum_b basis[tau, b] w_b of
every (postsynaptic, presynaptic) pair and of every stimulus dimension, lag by lag -- mean, sd, quantiles -- with a simultaneous
credible band over the whole curve and the posterior of the effective weight.  The counterpart of the reference's plot_results
pipeline (eval_state per sample, average_list_of_dicts / std_list_of_dicts of utils/avg_dicts.py, plot_imp_responses(s_mean,
s_std)) for the two entries it plots as mean +- 2 sd, without a state per draw.

filter_bands_numpy is the readable numpy statement of the rule csrc/pglm_filters.h states for one (row, group); filter_bands runs
the same rule on the device (DeviceGlm.filter_bands, k_filter_bands) on the tensor of draws where the lock-step samplers keep
it, and falls back to the numpy statement only above FILT_MAX_DRAWS pooled draws ('route' says which).  The two agree bit for
bit.  The sampling-based counterpart of connectivity.coupling_tests: 'excl_zero' marks the pairs whose simultaneous band
excludes zero at some lag."""
import numpy as np

from theano_pyglm_amd._lib import FILT_GRP_COLS, FILT_LAG_COLS, FILT_MAX_DRAWS

PIECE = 256                      # PGL_FILT_PIECE: the draws of one piece of a sum


def piece_sum(a):
    """The rule's sum over axis 0 of a (S, K): pieces of 256 consecutive rows, a piece summed ascending from 0.0, the pieces
    added in order from 0.0 (pgl_filt_sum).  Rows of +0.0 pad the last piece: they change no bit."""
    S, K = a.shape
    n_p = -(-S // PIECE)
    pad = np.zeros((n_p * PIECE, K))
    pad[:S] = a
    pad = pad.reshape(n_p, PIECE, K)
    acc = np.zeros((n_p, K))
    for i in range(PIECE):
        acc = acc + pad[:, i]
    tot = np.zeros(K)
    for j in range(n_p):
        tot = tot + acc[j]
    return tot


def band_quantile(sv, p):
    """The quantile p of the sorted columns sv (S, K) by diagnostics.quantile's linear rule with the position in doubles
    (pgl_filt_quantile)."""
    S = sv.shape[0]
    pos = p * float(S - 1)
    k = min(int(pos), S - 1)
    g = pos - float(k)
    lo, hi = sv[k] + 0.0, sv[min(k + 1, S - 1)] + 0.0        # (a zero order statistic is +0.0)
    if g == 0.0:
        return lo
    return lo + (hi - lo) * g if g < 0.5 else hi - (hi - lo) * (1.0 - g)


def band_probs(level):
    return ((1.0 - level) / 2.0, 0.5, (1.0 + level) / 2.0)


def band_rank(level, S):
    """k = ceil(level S), 1 .. S (pgl_filt_rank)"""
    t = level * float(S)
    k = int(t)
    if float(k) < t:
        k += 1
    return min(max(k, 1), S)


def curves(w, rows):
    """h (S, K) = the K rows (K, B) applied to the draws' weights w (S, B): b ascending from 0.0, every product and sum rounded
    on its own (pgl_filt_dot)"""
    h = np.zeros((w.shape[0], rows.shape[0]))
    for b in range(w.shape[1]):
        h = h + rows[None, :, b] * w[:, b, None]
    return h


def group_bands(w, basis, c, level):
    """The rule of one group (pgl_filt_group): w (S, B) the pooled draws of its weights -> (out (R, 5), grp (8,))."""
    S, B = w.shape
    R = basis.shape[0]
    out, grp = np.full((R, len(FILT_LAG_COLS)), np.nan), np.full(len(FILT_GRP_COLS), np.nan)
    if not np.all(np.isfinite(w)):
        grp[7] = 1.0
        return out, grp
    grp[7] = 0.0
    with np.errstate(all='ignore'):
        h = curves(w, np.concatenate([basis, c[None, :]], axis=0))            # (column R: the effective weight)
        fin = np.all(np.isfinite(h), axis=0)
        idx = np.nonzero(fin)[0]
        hv = h[:, idx]
        mean = piece_sum(hv) / float(S)
        dev = hv - mean
        sd = np.sqrt(piece_sum(dev * dev) / float(S - 1))
        sv = np.sort(hv, axis=0)
        five = np.stack([mean, sd] + [band_quantile(sv, p) for p in band_probs(level)], axis=1)      # (len(idx), 5)
        lag = idx < R
        out[idx[lag]] = five[lag]
        if fin[R]:
            grp[1:6] = five[-1]
            grp[6] = int(np.sum(h[:, R] > 0.0)) / float(S)
        use = lag & (sd > 0.0)
        r = np.abs(dev[:, use]) / sd[use]
        d = np.fmax.reduce(np.concatenate([np.zeros((S, 1)), r], axis=1), axis=1)       # (a NaN ratio is skipped)
        grp[0] = np.sort(d)[band_rank(level, S) - 1] + 0.0
    return out, grp


def _check_args(x, n_chains, first, G, basis, c, level):
    basis, c = np.asarray(basis, dtype=float), np.asarray(c, dtype=float)
    if x.ndim != 3 or x.size == 0 or n_chains < 1 or x.shape[1] % n_chains or basis.ndim != 2 or basis.size == 0 or \
            c.shape != (basis.shape[1],) or first < 0 or G < 1 or first + G * basis.shape[1] > x.shape[2] or \
            x.shape[0] * n_chains < 2 or not 0.0 < level < 1.0:
        raise ValueError("filter_bands: samples (n, n_chains * M, P) with n_chains * n >= 2, basis (R, B), c (B,), "
                         "first + G B <= P, level in (0, 1)")
    return basis, c


def filter_bands_numpy(samples, n_chains, first, G, basis, c, level):
    """The numpy statement of pgl_filter_bands: samples (n, n_chains * M, P) in the samplers' layout (draw i of chain c of row
    m at [i, c * M + m]) -> (out (M, G, R, 5) in FILT_LAG_COLS order, grp (M, G, 8) in FILT_GRP_COLS order)."""
    x = np.asarray(samples, dtype=float)
    C, first, G, level = int(n_chains), int(first), int(G), float(level)
    basis, c = _check_args(x, C, first, G, basis, c, level)
    n, M, (R, B) = x.shape[0], x.shape[1] // C, basis.shape
    pooled = x.reshape(n, C, M, -1).transpose(1, 0, 2, 3).reshape(C * n, M, -1)       # s = c n + i
    out, grp = np.empty((M, G, R, len(FILT_LAG_COLS))), np.empty((M, G, len(FILT_GRP_COLS)))
    for m in range(M):
        for g in range(G):
            o = first + g * B
            out[m, g], grp[m, g] = group_bands(pooled[:, m, o:o + B], basis, c, level)
    return out, grp


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def excludes_zero(mean, sd, c_sim):
    """(..., G) bool: some lag with |mean| > c_sim sd -- the simultaneous band mean +- c_sim sd does not contain the zero curve."""
    with np.errstate(invalid='ignore'):
        return np.any(np.abs(mean) > c_sim[..., None] * sd, axis=-1)


def bands_dict(out, grp, lags):
    """The arrays of one call as the dict filter_bands returns: the per-lag figures (M, G, R), the per-group ones (M, G)."""
    d = dict((k, np.array(out[..., i])) for i, k in enumerate(FILT_LAG_COLS))
    for i, k in enumerate(FILT_GRP_COLS):
        d[k] = np.array(grp[..., i])
    d['info'] = d['info'].astype(np.int32)
    d['excl_zero'] = excludes_zero(d['mean'], d['sd'], d['c_sim'])
    d['lags'] = lags
    return d


def filter_specs(population, stim=True):
    """[(key, first, G, basis (R, B), c (B,), lags)] of the filters of a served population under the layout theta_row gives:
    [bias, w_stim (D groups of B_stim, dimension-major), w_ir (N groups of B_imp, presynaptic-neuron-major)].
    c_b = dt sum_t basis[t, b] as connectivity.effective_weight_contrast."""
    from theano_pyglm_amd.components.bkgd import BasisStimulus
    glm = population.glm
    dt = float(glm.dt)
    ib = np.ascontiguousarray(glm.imp_model.ibasis, dtype=float)
    specs = [('impulse', 1 + glm.Dstim, population.N, ib, dt * ib.sum(axis=0), dt * np.arange(ib.shape[0]))]
    if stim and isinstance(glm.bkgd_model, BasisStimulus):
        sb = np.ascontiguousarray(glm.bkgd_model.ibasis, dtype=float)
        specs.append(('stim', 1, glm.Dstim // sb.shape[1], sb, dt * sb.sum(axis=0), dt * np.arange(sb.shape[0])))
    return specs


def _device_layout(samples, torch=None):
    """(x (n, C * M, P) in the samplers' layout, C) of draws (n, M, P) or (C, n, M, P), a host array or a torch tensor"""
    shape = tuple(samples.shape)
    if len(shape) not in (3, 4):
        raise ValueError("filter_bands: draws (n, M, P) or (n_chains, n, M, P)")
    is_t = hasattr(samples, 'is_cuda')
    if len(shape) == 3:
        return (samples if is_t else np.asarray(samples, dtype=float)), 1
    C, n, M, P = shape
    if is_t:
        return samples.permute(1, 0, 2, 3).reshape(n, C * M, P), C
    return np.ascontiguousarray(np.asarray(samples, dtype=float).transpose(1, 0, 2, 3)).reshape(n, C * M, P), C


def queue_bands(population, handle, torch, samples_dev, n_chains, level=0.95, stim=True):
    """The samplers' hook, first half: the kernel queued on their tensor (n, n_chains * M, P) where it lies, before the copy.
    -> {key: (out, grp)} device tensors, or None where n_chains * n exceeds FILT_MAX_DRAWS (finish_bands then runs the numpy
    statement)."""
    n = int(samples_dev.shape[0])
    if n * n_chains < 2 or not 0.0 < float(level) < 1.0:
        raise ValueError("filters: at least 2 pooled draws and a level in (0, 1)")
    if n * n_chains > FILT_MAX_DRAWS:
        return None
    up = lambda a: torch.tensor(a, dtype=torch.float64, device=samples_dev.device)
    return dict((key, handle.filter_bands(samples_dev, n_chains, first, G, up(basis), up(c), level))
                for key, first, G, basis, c, _ in filter_specs(population, stim))


def filters_level(filters):
    """The level of the samplers' filters= argument: True is 0.95, a number is itself"""
    return 0.95 if filters is True else float(filters)


def finish_bands(population, pending, samples, n_chains, level=0.95, stim=True):
    """Second half, behind the synchronisation: the dict filter_bands returns.  samples: the draws in the samplers' layout
    (n, n_chains * M, P), a host array or the device tensor, read only where pending is None."""
    res = {}
    if pending is None and hasattr(samples, 'is_cuda'):
        samples = samples.cpu().numpy()
    samples_host = samples
    for key, first, G, basis, c, lags in filter_specs(population, stim):
        if pending is None:
            out, grp = filter_bands_numpy(samples_host, n_chains, first, G, basis, c, level)
        else:
            out, grp = (t.cpu().numpy() for t in pending[key])
        res[key] = bands_dict(out, grp, lags)
    top = dict(res['impulse'])
    top['impulse'] = dict((k, top.pop(k)) for k in FILT_LAG_COLS)
    if 'stim' in res:
        top['stim'] = res['stim']
    top['route'] = 'host' if pending is None else 'device'
    top['level'] = float(level)
    return top


def filter_bands(population, samples, level=0.95, n_lo=0, stim=True, device=True):
    """The bands of the filters of neurons n_lo .. n_lo + M from posterior draws.  samples: the result of sample_glms_hmc /
    sample_glms_nuts, or the draws themselves, (n, M, P) or with a chain axis (n_chains, n, M, P), a numpy array or a torch
    device tensor.  Returns a dict:
      'impulse'      {'mean', 'sd', 'q_lo', 'median', 'q_hi'}: arrays (M, N, R), [m, j] the response of neuron n_lo + m to a
                     spike of neuron j; the quantiles at (1 - level) / 2, 1 / 2, (1 + level) / 2;
      'c_sim'        (M, N): mean +- c_sim sd holds at least a share `level` of the draws at every lag at once;
      'weight_mean', 'weight_sd', 'weight_q_lo', 'weight_median', 'weight_q_hi', 'p_pos'   (M, N): the posterior of the
                     effective weight dt sum_t h(t) and the share of draws in which it is positive;
      'info'         (M, N) int: 1 where a weight of the pair is not finite in some draw (its figures are NaN);
      'excl_zero'    (M, N) bool: the simultaneous band excludes zero at some lag;
      'lags'         (R,) seconds;  'route': 'device' or 'host';  'level'.
    With stim=True and a basis stimulus, 'stim': the same keys for the stimulus filters, arrays (M, D, R_stim) and (M, D), one
    group per stimulus dimension.  A population the lock-step samplers do not serve raises their ValueError.  n_lo names the
    first row's neuron in messages only: the rows are whatever the draws hold.  device=False runs the numpy statement; so
    do more than FILT_MAX_DRAWS pooled draws ('route' = 'host')."""
    from theano_pyglm_amd.inference.batched_hmc import _check
    _check(population)
    if isinstance(samples, dict):
        samples = samples['samples']
    x, C = _device_layout(samples)
    if x.shape[2] != population.glm.P:
        raise ValueError("filter_bands: the draws have %d columns, the theta rows of neuron %d on have %d"
                         % (x.shape[2], n_lo, population.glm.P))
    S = int(x.shape[0]) * C
    if S < 2 or not 0.0 < float(level) < 1.0:
        raise ValueError("filter_bands: at least 2 pooled draws and a level in (0, 1)")
    is_t = hasattr(x, 'is_cuda')
    if not device or S > FILT_MAX_DRAWS:
        return finish_bands(population, None, x.cpu().numpy() if is_t else x, C, level, stim)
    from theano_pyglm_amd.inference.lockstep import session
    with session(population) as (torch, dev, stream, handles):
        t = x if is_t else torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
        t = t.to(dtype=torch.float64).contiguous()
        pending = queue_bands(population, handles[0], torch, t, C, level, stim)
        stream.synchronize()
        return finish_bands(population, pending, None, C, level, stim)


def average_states(population, x, samples, level=0.95, ddof=0, device=True):
    """(s_mean, s_std): state dicts in eval_state's shape -- {'glms': [glm.get_state(...) per neuron]} -- whose entries
    ['glms'][n]['imp']['impulse'] (N, R) and, with a basis stimulus, ['glms'][n]['bkgd']['stim_response'] (R_stim,: the
    filter of stimulus dimension 0, as get_state gives it) hold the mean and the sd of the draws: what the reference's
    average_list_of_dicts / std_list_of_dicts give for these two entries over eval_state of every sample, from the bands and
    without a state per draw.  samples must hold all N neurons.  ddof=0 (default): the reference's sd, denominator S
    (variance_list_of_dicts averages the squared deviations), the bands' sd times sqrt((S - 1) / S); ddof=1: the bands' own.
    The other entries of s_mean are those of x; s_std holds the two entries only (and each component's basis)."""
    b = filter_bands(population, samples, level=level, stim=True, device=device)
    mean, sd = b['impulse']['mean'], b['impulse']['sd']
    if mean.shape[0] != population.N:
        raise ValueError("average_states: the draws must hold all %d neurons" % population.N)
    if isinstance(samples, dict):
        samples = samples['samples']
    shape = tuple(samples.shape)
    S = shape[0] * shape[1] if len(shape) == 4 else shape[0]
    if ddof not in (0, 1):
        raise ValueError("average_states: ddof 0 or 1")
    scale = 1.0 if ddof == 1 else np.sqrt((S - 1.0) / S)
    s_mean, s_std = {'glms': []}, {'glms': []}
    for n in range(population.N):
        st = population.glm.get_state(x['glms'][n])
        sd_st = population.glm.get_state(None)
        st['imp']['impulse'] = mean[n].copy()
        sd_st['imp']['impulse'] = sd[n] * scale
        if 'stim' in b:
            st['bkgd']['stim_response'] = b['stim']['mean'][n, 0].copy()
            sd_st['bkgd']['stim_response'] = b['stim']['sd'][n, 0] * scale
        s_mean['glms'].append(st)
        s_std['glms'].append(sd_st)
    return s_mean, s_std


def band_table(res, n_lo=0, truth=None):
    """The per-neuron lines synth_map --filters prints: the number of presynaptic neurons whose simultaneous band excludes
    zero, the largest |weight_mean| / weight_sd, and with truth (N, N) bool [post, pre] the true / false positives of
    'excl_zero' by connectivity.detection_counts (the family: every pair with a finite |weight_mean| / weight_sd, the
    diagonal included; row m of the result is the postsynaptic neuron n_lo + m)."""
    from theano_pyglm_amd.inference.connectivity import detection_counts
    ex = res['excl_zero']
    with np.errstate(invalid='ignore', divide='ignore'):
        z = np.abs(res['weight_mean']) / res['weight_sd']
    lines = ["filter bands (level %.3g, %s): neuron  pre excl. zero of %d  max |weight| / sd%s"
             % (res.get('level', np.nan), res['route'], ex.shape[1], "  true pos  false pos" if truth is not None else "")]
    for m in range(ex.shape[0]):
        ln = "%6d  %8d  %12.2f" % (n_lo + m, int(ex[m].sum()), np.nanmax(z[m]) if np.any(~np.isnan(z[m])) else np.nan)
        if truth is not None:
            d = detection_counts({'wald': z[m:m + 1], 'q_value': z[m:m + 1], 'significant': ex[m:m + 1]},
                                 np.asarray(truth, dtype=bool)[n_lo + m:n_lo + m + 1], include_self=True)
            ln += "  %8d  %9d" % (d['tp'], d['fp'])
        lines.append(ln)
    lines.append("%d of %d pairs have a simultaneous band that excludes zero" % (int(ex.sum()), ex.size))
    return "\n".join(lines)
