"""The goodness of fit on the device against the route the library had before it, in one process, at C2 (N = 32,
nT = 300 000) and C3 (N = 128, nT = 600 000).  Parameters: a seeded draw of the model (Population.sample) on Poisson spikes,
NOT the lock-step BFGS fit -- the kernels' time does not depend on the values, and the JSON says so ('parameters').

Per call, wall time of queued calls in windows of at least 0.5 s around a stream synchronisation (a shorter window measures
the clock), after a warm-up window; pgl_rescale_dev and pgl_rescale_corr_dev ALTERNATE, `rounds` windows each, and every
figure is reported as median, min and max over its windows: a difference inside the spread is no finding.  The same for
pgl_ks_uniform_dev on the intervals (interval counts per neuron beside it) and on an all-clumped input of the same counts
(every z in [1 - 1e-12, 1]).  These are wall times of queued calls, not kernel times: kernel times come from a
`rocprofv3 --kernel-trace --stats` run of this script of its own (no counters in it), which this script does not make.
Per draw at S = 100: ks_time_rescaling_draws on the population, against the parent commit's route -- per draw
compute_rescaled_intervals (every interval over PCIe) and ks_from_intervals in numpy; both after one untimed warm-up call.

    python tools/ks_bench.py [--rounds 5] [--window 0.5] [--draws 100] [--host-draws 5] [--out profiles/ks_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd.inference import gof


def spread(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v)), 'windows': len(v)}


def run(name, N, nT, rounds, window, draws, host_draws):
    import torch
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
    from theano_pyglm_amd.population import Population
    rng = np.random.default_rng(1234)
    dt = 0.001
    popn = Population(stabilize_sparsity(make_model('standard_glm', N=N, dt=dt)))
    x = popn.sample(np.random.RandomState(5))
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(float)
    data = {'S': S, 'N': N, 'dt': dt, 'T': nT * dt, 'stim': None, 'dt_stim': 0.1}
    popn.add_data(data)
    d = popn._handle(data)
    theta, Weff = np.ascontiguousarray(popn.theta_matrix(x)), np.ascontiguousarray(popn.W_eff(x))
    off = d.rescale_count()
    t = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(Weff)
    d_off = torch.tensor(off, dtype=torch.int64, device='cuda')
    total = int(off[-1])
    d_tau = torch.empty((max(total, 1),), dtype=torch.float64, device='cuda')
    d_z = torch.empty_like(d_tau)
    d_st = torch.empty((N, 4), dtype=torch.float64, device='cuda')
    d_ks = torch.empty((N, 4), dtype=torch.float64, device='cuda')
    d_clump = t(rng.uniform(27.7, 40.0, size=max(total, 1)))
    torch.cuda.synchronize()
    cnt = np.diff(off)
    out = {'config': name, 'N': N, 'nT': nT, 'parameters': 'seeded Population.sample, not a fit', 'window_s': window,
           'intervals': total, 'intervals_per_neuron_min': int(cnt.min()), 'intervals_per_neuron_max': int(cnt.max())}

    def one_window(fn):
        """ms per call over one window of >= `window` seconds of queued calls"""
        fn()
        d.sync()
        t0 = time.perf_counter()
        fn()
        d.sync()
        n = max(int(window / max(time.perf_counter() - t0, 1e-6)) + 1, 4)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        d.sync()
        return (time.perf_counter() - t0) / n * 1e3

    fns = {'rescale_dev_ms': lambda: d.rescale_dev(d_th.data_ptr(), d_W.data_ptr(), d_tau.data_ptr(), d_off.data_ptr(), d_st.data_ptr()),
           'rescale_corr_dev_ms': lambda: d.rescale_corr_dev(d_th, d_W, d_tau, d_off, d_st, seed=1, draw=0),
           'ks_uniform_dev_ms': lambda: d.ks_uniform(d_tau[:total], d_off, out=d_ks, zsorted=d_z),
           'ks_uniform_dev_clumped_ms': lambda: d.ks_uniform(d_clump[:total], d_off, out=d_ks, zsorted=d_z)}
    for fn in fns.values():                           # warm-up: buffers, clocks
        one_window(fn)
    got = dict((k, []) for k in fns)
    for _ in range(rounds):                           # interleaved rounds
        for k, fn in fns.items():
            got[k].append(one_window(fn))
    for k, v in got.items():
        out[k] = spread(v)
    out['correction_ms_per_round'] = spread(np.array(got['rescale_corr_dev_ms']) - np.array(got['rescale_dev_ms']))
    out['clumped_over_plain_per_round'] = spread(np.array(got['ks_uniform_dev_clumped_ms']) / np.array(got['ks_uniform_dev_ms']))

    # per draw: the draws function against the parent's route
    P = theta.shape[1]
    samples = np.repeat(theta[None], draws, axis=0) + 1e-3 * rng.standard_normal((draws, N, P))
    gof.ks_time_rescaling_draws(popn, x, samples[:2], seed=1)                 # warm-up
    t0 = time.perf_counter()
    res = gof.ks_time_rescaling_draws(popn, x, samples, seed=1)
    out['draws_device_s'] = time.perf_counter() - t0
    out['draws'] = draws

    def parent():
        taus, stats = popn.compute_rescaled_intervals(x)
        return gof.ks_from_intervals(taus)
    parent()                                                                  # warm-up: the handle's first allocations
    t0 = time.perf_counter()
    for _ in range(host_draws):
        parent()
    per = (time.perf_counter() - t0) / host_draws
    out['parent_route_draws_timed'] = host_draws
    out['draws_parent_route_s'] = per * draws
    out['parent_over_device'] = out['draws_parent_route_s'] / out['draws_device_s']
    out['D_mean_over_neurons'] = float(np.nanmean(res['D_mean']))
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--draws', type=int, default=100)
    ap.add_argument('--host-draws', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'ks', 'C2': run('C2', 32, 300000, a.rounds, a.window, a.draws, a.host_draws),
           'C3': run('C3', 128, 600000, a.rounds, a.window, a.draws, a.host_draws)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
