"""
Posterior-predictive check of the spike counts: draw many spike trains from the model at the parameters x on the current
data's length and stimulus (pgl_simulate_batch_dev: one workgroup per replicate, only the counts come back) and compare
every neuron's observed count with the replicates.

A count far in a tail of its predictive distribution says the model does not reproduce that neuron's rate; it says nothing
about timing (inference/gof.py tests that).  The reference has no counterpart.
"""
import numpy as np

from theano_pyglm_amd import _lib


def replicate_counts(population, x, n_rep, seed=0, rep0=0):
    """(counts (n_rep, N) int64, exceptions (n_rep) int64) of n_rep replicates of the current data set simulated at x.  Always
    on the device: X0, AW and the results stay there, the spike trains are never materialised."""
    import torch
    if population._time_shard is not None:
        raise ValueError("predictive counts of a time-sharded population are not implemented")
    data = population._current
    if data is None:
        raise ValueError("no current data set: add_data / set_data first")
    nT, N = np.asarray(data['S']).shape
    dt = population.glm.dt
    X0, AW = population._simulation_inputs(x, (0.0, nT * dt), dt, data.get('stim', None), data.get('dt_stim', None), nT=nT)
    AW = np.ascontiguousarray(np.transpose(AW, (0, 2, 1)))
    R = AW.shape[1]
    n_rep = int(n_rep)
    in_lds, ws_bytes = _lib.simulate_batch_plan(N, R)
    dev = torch.device('cuda:%d' % population.device)
    d_X0 = torch.from_numpy(X0).to(dev)
    d_AW = torch.from_numpy(AW).to(dev)
    d_counts = torch.empty((n_rep, N), dtype=torch.int64, device=dev)
    d_exc = torch.empty(n_rep, dtype=torch.int64, device=dev)
    d_ws = None if in_lds else torch.empty(n_rep * ws_bytes // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                               # (the uploads, before the library's launch on the null stream)
    _lib.simulate_batch_dev(N, nT, R, population.glm.nlin_model.kind, dt, d_X0.data_ptr(), d_AW.data_ptr(), n_rep,
                            d_counts.data_ptr(), d_exc.data_ptr(), seed=seed, rep0=rep0,
                            d_workspace=0 if d_ws is None else d_ws.data_ptr(), device=population.device)
    torch.cuda.synchronize(dev)
    return d_counts.cpu().numpy(), d_exc.cpu().numpy()


def summarize_counts(observed, counts):
    """Per-neuron summary of replicate counts (n_rep, N) against the observed counts (N): mean, std (ddof = 0), the central
    95 % interval (2.5 and 97.5 percentiles), and the two-sided predictive p-value from the rank of the observed count,
    p = min(1, 2 min(P(rep <= obs), P(rep >= obs))) with P the replicate frequencies."""
    observed = np.asarray(observed, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    lo, hi = np.percentile(counts, [2.5, 97.5], axis=0)
    le = np.mean(counts <= observed[None, :], axis=0)
    ge = np.mean(counts >= observed[None, :], axis=0)
    return {'observed': observed, 'mean': counts.mean(axis=0), 'std': counts.std(axis=0), 'lo': lo, 'hi': hi,
            'min': counts.min(axis=0), 'max': counts.max(axis=0), 'p_value': np.minimum(1.0, 2.0 * np.minimum(le, ge))}


def predictive_counts(population, x, n_rep, seed=0):
    """Predictive check of the spike counts of the population's current data under x.  Returns a dict of per-neuron arrays:
    observed, mean, std, lo / hi (central 95 % interval), min / max, p_value (two-sided, from the rank of the observed
    count among the replicates), plus counts (n_rep, N), exceptions (n_rep) and n_rep."""
    counts, exc = replicate_counts(population, x, n_rep, seed=seed)
    observed = np.asarray(population._current['S']).sum(axis=0).astype(np.int64)
    res = summarize_counts(observed, counts)
    res.update({'counts': counts, 'exceptions': exc, 'n_rep': int(n_rep)})
    return res


def format_table(res):
    lines = ["predictive spike counts (%d replicates)" % res['n_rep'],
             "%6s %10s %12s %10s %10s %10s %8s" % ('neuron', 'observed', 'mean', 'std', '2.5%', '97.5%', 'p')]
    for n in range(len(res['observed'])):
        lines.append("%6d %10d %12.1f %10.1f %10.1f %10.1f %8.3f"
                     % (n, res['observed'][n], res['mean'][n], res['std'][n], res['lo'][n], res['hi'][n], res['p_value'][n]))
    inside = np.sum((res['observed'] >= res['lo']) & (res['observed'] <= res['hi']))
    lines.append("%d of %d neurons inside the central 95 %% interval" % (int(inside), len(res['observed'])))
    return "\n".join(lines)
