"""The NUTS chain (inference/batched_nuts.py) beside the fixed-length lock-step HMC chain (inference/batched_hmc.py,
n_leapfrog = 10) per configuration, in one process: the same lock-step BFGS fit, seed, warm-up length, number of kept draws
and mass matrix, for mass='laplace' and mass='laplace_dense'.  Seeded inputs as tools/ncg_bench.py makes them.

    python tools/nuts_bench.py [--configs C2,C3] [--samples 200] [--warmup 100] [--max-depth 8] [--out profiles/nuts_bench.json]

C2: N = 32, nT = 300 000; C3: N = 128, nT = 600 000.  Per configuration floor_ms_per_evaluation (bare pgl_ll_grad_dev calls of
all rows on one stream) and, per mass and sampler (chain time = the call minus the mass set-up):
  ms_per_launch          chain time per evaluation-plus-row-launches; over_floor = that / floor_ms_per_evaluation
  evals_per_kept_draw    evaluations of all rows per kept draw (NUTS: launches / kept draws, warm-up included)
  ess_median, ess_min    Geyer's ESS over all parameters of all rows, of the kept draws; ess_*_per_s per second of chain time
  step                   the frozen steps (min, median, max)
NUTS only: idle_share (row evaluations spent on rows that had finished), depth_histogram (kept transitions by doublings
begun), divergent (transitions after warm-up), leapfrogs_per_row (total, min / median / max over rows), launches.
nuts_over_hmc: the ratio of the two samplers' ess_median_per_s and ess_min_per_s.
Records, sets no threshold.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS, population


def say(msg):
    sys.stderr.write(msg + "\n")
    sys.stderr.flush()


def spread(v):
    v = np.asarray(v, dtype=float)
    return {'min': float(v.min()), 'median': float(np.median(v)), 'max': float(v.max())}


def worth(res, chain_s, launches, floor_ms, n_samples):
    from theano_pyglm_amd.inference.batched_hmc import summarize
    ess = summarize(res['samples'])['ess']
    out = {'chain_s': chain_s, 'launches': int(launches), 'ms_per_launch': chain_s * 1e3 / launches,
           'evals_per_kept_draw': launches / float(n_samples), 'ess_median': float(np.median(ess)), 'ess_min': float(np.min(ess)),
           'step': spread(res['step_sz']), 'accept': spread(res['accept_rate'])}
    out['over_floor'] = out['ms_per_launch'] / floor_ms
    out['ess_median_per_s'] = out['ess_median'] / chain_s
    out['ess_min_per_s'] = out['ess_min'] / chain_s
    if 'dense_rows' in res:
        out['dense_rows'] = int(np.sum(res['dense_rows']))
    return out


def run(name, n_samples, n_warmup, max_depth, n_leapfrog):
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc
    from theano_pyglm_amd.inference.batched_nuts import sample_glms_nuts
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    fit_glms_batched_torch(popn, x)
    say("%s: fitted" % name)
    out = {'config': name, 'N': N, 'nT': nT, 'n_samples': n_samples, 'n_warmup': n_warmup, 'max_depth': max_depth,
           'hmc_n_leapfrog': n_leapfrog}
    # the floor: bare evaluations of all rows
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    P = popn.glm.P
    th = torch.tensor(popn.theta_matrix(x), dtype=torch.float64, device=dev)
    We = torch.tensor(popn.W_eff(x), dtype=torch.float64, device=dev)
    buf = torch.empty(N * (1 + P), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    try:
        reps = 100
        for k in range(2):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                h.ll_grad_dev(th.data_ptr(), We.data_ptr(), buf.data_ptr(), buf[N:].data_ptr(), 0, N)
            stream.synchronize()
            out['floor_ms_per_evaluation'] = (time.perf_counter() - t0) * 1e3 / reps
    finally:
        h.set_stream(None)
    floor = out['floor_ms_per_evaluation']
    out['mass'] = {}
    for mass in ('laplace', 'laplace_dense'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sample_glms_hmc(popn, x, n_samples, n_warmup=n_warmup, n_leapfrog=n_leapfrog, step_sz=0.1, mass=mass, seed=1)
        wall = time.perf_counter() - t0
        st = popn.last_fit_stats
        hmc = worth(res, wall - st['mass_setup_s'], st['ll_grad_launches'] - 1, floor, n_samples)
        hmc['setup_s'] = st['mass_setup_s']
        say("%s %s: HMC %.1f s" % (name, mass, wall))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sample_glms_nuts(popn, x, n_samples, n_warmup=n_warmup, max_depth=max_depth, step_sz=0.1, mass=mass, seed=1)
        wall = time.perf_counter() - t0
        st = popn.last_fit_stats
        nuts = worth(res, wall - st['mass_setup_s'], res['launches'], floor, n_samples)
        nuts.update({'setup_s': st['mass_setup_s'], 'idle_share': st['idle_share'],
                     'depth_histogram': [int(c) for c in np.bincount(res['depth'].ravel(), minlength=max_depth + 1)],
                     'depth_median': float(np.median(res['depth'])), 'divergent': int(res['divergent'].sum()),
                     'leapfrogs_per_row': spread(st['leapfrog_steps']),
                     'leapfrogs_per_kept_transition': spread(res['n_leapfrog'].mean(axis=0))})
        say("%s %s: NUTS %.1f s, %d launches" % (name, mass, wall, res['launches']))
        out['mass'][mass] = {'hmc': hmc, 'nuts': nuts,
                             'nuts_over_hmc': {'ess_median_per_s': nuts['ess_median_per_s'] / hmc['ess_median_per_s'],
                                               'ess_min_per_s': (nuts['ess_min_per_s'] / hmc['ess_min_per_s']
                                                                 if hmc['ess_min_per_s'] > 0 else None)}}
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--samples', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--max-depth', type=int, default=8)
    ap.add_argument('--leapfrog', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'nuts'}
    if a.out and os.path.exists(a.out):                        # (configurations may be run one call at a time)
        with open(a.out) as f:
            res.update(json.loads(f.read()))
    for name in a.configs.split(','):
        res[name] = run(name, a.samples, a.warmup, a.max_depth, a.leapfrog)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
