"""The lock-step proximal-gradient fit of the group-lasso MAP (inference/batched_prox.py) per configuration, next to its
floor and to the lock-step BFGS fit of the same objective, in one process.  Seeded inputs as tools/ncg_bench.py makes
them (Poisson spikes at 20 Hz), standard_glm (group-lasso prior, lam = 1), started at the lock-step BFGS fit.

    python tools/prox_bench.py [--configs C2,C3] [--out profiles/prox_bench.json]

C2: N = 32, nT = 300 000; C3: N = 128, nT = 600 000.  Per configuration:
  bfgs_s                     one lock-step BFGS sweep from the sample (the fit the path is compared with)
  kkt_at_bfgs_max            the KKT residual at the BFGS fit (below gtol: the proximal fit from there ends in init)
  fit / fit_cold             fit_glms_prox at the prior's lam from the BFGS fit / from the sample the BFGS fit started at (the
                             timings and the floor are fit_cold's), --repeats calls after one warm-up (min, median,
                             max): iterations and evaluations per neuron to gtol, statuses, launches, wall_s of the whole call,
                             loop_s (from behind the init launch to the end of the last launch: no packing, upload or copy
                             back) and ms_per_eval = loop_s over the evaluation-plus-row-launch pairs inside it
  floor_ms_per_eval          the same number of bare pgl_ll_grad_dev calls of all rows on the same stream, per call, as often
  over_floor                 the ratio of the medians (the HMC chain's: profiles/hmc_bench.json, device_over_floor)
  row_launch_ms              pgl_prox_step_dev alone, 200 launches in a row on rows that never end
                             F_minus_F_bfgs: the objective minus the objective at the BFGS fit, same lam, per neuron;
                             zero_groups: presynaptic groups exactly at mu (zero_groups_bfgs: at the BFGS fit)
  path                       lasso_path with 10 points from the BFGS fit: wall time, against 10 cold BFGS sweeps (10 bfgs_s),
                             non-zero groups per point
Records, sets no threshold.  Prints one JSON line."""
import argparse, copy, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS, population


def _mmm(a):
    a = np.asarray(a, dtype=float)
    return {'min': float(a.min()), 'median': float(np.median(a)), 'max': float(a.max())}


def run(name, n_lams, reps):
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference import batched_prox as BP
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    x_sample = copy.deepcopy(x)
    fit_glms_batched_torch(popn, copy.deepcopy(x))             # warm: resident tiles, streams
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit_glms_batched_torch(popn, x)
    torch.cuda.synchronize()
    out = {'config': name, 'N': N, 'nT': nT, 'bfgs_s': time.perf_counter() - t0, 'lam': float(popn.glm.imp_model.prior.lam)}
    at_bfgs = BP.fit_glms_prox(popn, copy.deepcopy(x), maxiter=0)        # F and the support at the BFGS fit: no step
    # from the BFGS fit (where the KKT test may already hold: the fit then ends in init) and from the sample itself
    for label, start in (('fit', x), ('fit_cold', x_sample)):
        walls, loops = [], []
        for rep in range(1 + reps):                            # the first call warms up and is dropped
            xf = copy.deepcopy(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = BP.fit_glms_prox(popn, xf)
            walls.append(time.perf_counter() - t0)
            loops.append(popn.last_fit_stats['loop_s'])
        st = popn.last_fit_stats
        n = st['ll_grad_launches'] - 1                         # the launches inside loop_s (the one before init is outside)
        out[label] = {'iters': _mmm(res['iters']), 'nfev': _mmm(res['nfev']), 'kkt_max': float(res['kkt'].max()),
                      'status_counts': [int(np.sum(res['status'] == k)) for k in range(3)],
                      'restarts': _mmm(st['restarts']), 'll_grad_launches': st['ll_grad_launches'],
                      'row_launches': st['row_launches'], 'flag_polls': st['flag_polls'], 'repeats': reps,
                      'wall_s': _mmm(walls[1:]), 'loop_s': _mmm(loops[1:]),
                      'ms_per_eval': _mmm(np.array(loops[1:]) * 1e3 / n) if n > 0 else None,
                      'F_minus_F_bfgs': _mmm(res['objective'] - at_bfgs['objective']),
                      'zero_groups': int(np.sum(~res['support']))}
    n = max(n, 1)
    out['zero_groups_bfgs'] = int(np.sum(~at_bfgs['support']))
    out['groups'] = N * N
    out['kkt_at_bfgs_max'] = float(at_bfgs['kkt'].max())
    # the floor: as many bare evaluations, and the row launch alone
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    P = popn.glm.P
    f64 = torch.float64
    th = torch.tensor(popn.theta_matrix(xf), dtype=f64, device=dev)
    We = torch.tensor(popn.W_eff(xf), dtype=f64, device=dev)
    buf = torch.empty(N * (1 + P), dtype=f64, device=dev)
    stt = torch.zeros(h.prox_state_doubles(N, P), dtype=f64, device=dev)
    stt[:N * P].view(N, P).copy_(th)
    lam = torch.full((N,), out['lam'], dtype=f64, device=dev)
    Xt = torch.empty((N, P), dtype=f64, device=dev)
    pk = BP._Packing(popn, torch, [h], (0, N))
    prm = pk.prior_params()
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    try:
        floors = []
        for k in range(1 + reps):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                h.ll_grad_dev(th.data_ptr(), We.data_ptr(), buf.data_ptr(), buf[N:].data_ptr(), 0, N)
            stream.synchronize()
            floors.append((time.perf_counter() - t0) * 1e3 / n)
        out['floor_ms_per_eval'] = _mmm(floors[1:])
        # k_prox_step alone: rows that never end (no iteration or backtrack limit in reach), the same (ll, grad) fed again and
        # again -- the decisions mean nothing, every row does a step's reductions and emits a trial
        h.ll_grad_dev(th.data_ptr(), We.data_ptr(), buf.data_ptr(), buf[N:].data_ptr(), 0, N)
        g0 = buf.clone()
        h.prox_init_dev(stt.data_ptr(), N, P, g0.data_ptr(), g0[N:].data_ptr(), prm, lam.data_ptr(), 1e-300, 1 << 30,
                        Xt.data_ptr(), 0)
        nrow = 200
        rows = []
        for k in range(1 + reps):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(nrow):
                h.prox_step_dev(stt.data_ptr(), N, P, g0.data_ptr(), g0[N:].data_ptr(), prm, lam.data_ptr(), 1e-300, 1 << 30,
                                1 << 30, Xt.data_ptr(), 0)
            stream.synchronize()
            rows.append((time.perf_counter() - t0) * 1e3 / nrow)
        out['row_launch_ms'] = _mmm(rows[1:])
        out['rows_still_running'] = int((stt[5 * N * P:].view(-1, N)[9] != 2.0).sum().item())
    finally:
        h.set_stream(None)
    out['over_floor'] = out['fit_cold']['ms_per_eval']['median'] / out['floor_ms_per_eval']['median']
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    path = BP.lasso_path(popn, x, n_lams=n_lams)
    wall = time.perf_counter() - t0
    out['path'] = {'n_lams': n_lams, 'wall_s': wall, 'cold_bfgs_sweeps_s': n_lams * out['bfgs_s'],
                   'lams': [float(v) for v in path['lams']], 'nonzero_groups': [int(s.sum()) for s in path['support']],
                   'iters_median': [float(np.median(v)) for v in path['iters']],
                   'status_counts': [[int(np.sum(s == k)) for k in range(3)] for s in path['status']]}
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--lams', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'prox'}
    for name in a.configs.split(','):
        res[name] = run(name, a.lams, a.repeats)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
