"""The adaptive sequential Monte Carlo run (inference/batched_smc.py) per configuration and mass, next to annealed importance
sampling given the same number of ll+grad launches, in one process.  Seeded inputs and the N(0, 1) impulse prior of
tools/ais_bench.py, started at the lock-step BFGS MAP fit.

    python tools/smc_bench.py [--configs C2,C3] [--mass laplace,laplace_dense] [--out profiles/smc_bench.json]

Per configuration and mass:
  smc              smc_glms, seed 1: wall time, launches, host reads, stages per neuron (min / median / max), resamplings,
                   unfinished neurons, idle share, final ESS, log_Z + log_prior_norm minus the Laplace evidence
  floor_s          the same number of bare pgl_ll_grad_dev calls on the same stream; run_over_floor their ratio
  stage_s          as many pgl_smc_stage_dev calls as the run made, alone, on a state whose ll0 are spread wide (every call
                   runs the whole bisection and no neuron finishes)
  ais              ais_glms with a reference ladder whose length gives the K particles the SMC run's launches (its pilot
                   particle comes on top): wall time, launches, ESS, AIS minus Laplace
  seeds            log_Z of both estimators over --seeds seeds: per neuron the standard deviation over the seeds, summarised
A wall budget (--budget-s) bounds the whole: what no longer fits is recorded as skipped, not guessed.
Records, sets no threshold.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS
from ais_bench import population


def q3(v):
    v = np.asarray(v, dtype=float)
    v = v[np.isfinite(v)]
    if not v.size:
        return None
    return {'min': float(v.min()), 'median': float(np.median(v)), 'max': float(v.max())}


def ladder_for(n_moves):
    """The reference ladder with n_moves temperatures that are followed by moves (its length varies with n_temps: duplicates
    are removed), or the nearest below."""
    from theano_pyglm_amd.inference.batched_ais import reference_ladder
    best = reference_ladder(5)
    for n in range(5, 5 * n_moves + 50):
        b = reference_ladder(n)
        if b.size - 2 <= n_moves:
            best = b
        if b.size - 2 >= n_moves:
            break
    return best


def stage_launches_alone(popn, K, M, P, S, prm, n_calls):
    import torch
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    f64 = torch.float64
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            R = K * M
            st = torch.zeros(h.ais_state_doubles(R, P), dtype=f64, device=dev)
            smc = torch.zeros(h.smc_state_doubles(K, M, P, S), dtype=f64, device=dev)
            Xt = torch.empty((R, P), dtype=f64, device=dev)
            buf = torch.zeros(R * (1 + P), dtype=f64, device=dev)
            buf[:R] = -1e6 * torch.rand(R, dtype=f64, device=dev)
            h.smc_init_dev(st.data_ptr(), smc.data_ptr(), K, M, P, S, 0, prm, 0.1, 1, Xt.data_ptr())
            h.ais_start_dev(st.data_ptr(), K, M, P, buf.data_ptr(), buf[R:].data_ptr(), prm)
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_calls):
                h.smc_stage_dev(st.data_ptr(), smc.data_ptr(), K, M, P, S, prm, 1, 0.9, 0.5, 1e-6, 1)
            stream.synchronize()
            dt = time.perf_counter() - t0
            left = int(smc[10 * M + 6 * S * M + 3 * R].item())
            return dt, left
    finally:
        h.set_stream(None)


def run(name, masses, K, L, n_steps, cess, max_stages, seeds, deadline):
    import torch
    from theano_pyglm_amd.inference.batched_ais import ais_glms
    from theano_pyglm_amd.inference.batched_smc import smc_glms
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch, _Packing
    from theano_pyglm_amd.inference.laplace import laplace_glms
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    fit_glms_batched_torch(popn, x)
    P = popn.glm.P
    lap = np.array([r['log_evidence'] for r in laplace_glms(popn, x)])
    out = {'config': name, 'N': N, 'nT': nT, 'P': P, 'n_particles': K, 'n_leapfrog': L, 'n_steps': n_steps, 'cess': cess,
           'max_stages': max_stages, 'impulse_prior': 'gaussian(0, 1)'}
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    prm = _Packing(popn, None).prior_params()
    for mass in masses:
        rec = {}
        out[mass] = rec
        if time.time() > deadline:
            rec['skipped'] = 'wall budget'
            continue
        kw = dict(n_particles=K, cess=cess, n_steps=n_steps, n_leapfrog=L, step_sz=0.1, mass=mass, max_stages=max_stages)
        smc_glms(popn, x, seed=99, **dict(kw, max_stages=2))     # warm-up: allocator, streams, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = smc_glms(popn, x, seed=1, **kw)
        run_s = time.perf_counter() - t0                         # (the mass -- Hessians at x -- is inside this clock)
        st = popn.last_fit_stats
        d = res['log_Z'] + res['log_prior_norm'] - lap
        ess_final = [res['ess'][res['n_stages'][n] - 1, n] for n in range(N)]
        rec['smc'] = {'run_s': run_s, 'll_grad_launches': st['ll_grad_launches'], 'stage_launches': st['stage_launches'],
                      'row_launches': st['row_launches'], 'host_reads': st['host_reads'], 'factorisations': st['factorisations'],
                      'stages_per_neuron': q3(res['n_stages']), 'resamplings_per_neuron': q3(res['n_resampled']),
                      'unfinished': int((~res['finished']).sum()), 'idle_row_evaluations': res['idle_row_evaluations'],
                      'ess_final': q3(ess_final), 'accept_rate': q3(res['accept_rate']), 'step_sz': q3(res['step_sz']),
                      'beta_reached': q3([res['betas'][res['n_stages'][n] - 1, n] for n in range(N)]),
                      'smc_minus_laplace': q3(d)}
        print(name, mass, 'smc', json.dumps(rec['smc']), file=sys.stderr, flush=True)
        # the floor
        th = torch.tensor(popn.theta_matrix(x), dtype=torch.float64, device=dev)
        We = torch.tensor(popn.W_eff(x), dtype=torch.float64, device=dev)
        buf = torch.empty(N * (1 + P), dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(dev)
        h.set_stream(stream.cuda_stream)
        try:
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(st['ll_grad_launches']):
                h.ll_grad_dev(th.data_ptr(), We.data_ptr(), buf.data_ptr(), buf[N:].data_ptr(), 0, N)
            stream.synchronize()
            rec['floor_s'] = time.perf_counter() - t0
        finally:
            h.set_stream(None)
        rec['run_over_floor'] = run_s / rec['floor_s']
        rec['stage_s'], left = stage_launches_alone(popn, K, N, P, max_stages, prm, st['stages'])
        rec['stage_share_of_run'] = rec['stage_s'] / run_s
        rec['stage_bench_neurons_left'] = left
        # annealed importance sampling on the same budget
        n_moves = max((st['ll_grad_launches'] // K - 1) // (L * n_steps), 1)
        betas = ladder_for(n_moves)
        akw = dict(n_particles=K, betas=betas, n_steps=n_steps, n_leapfrog=L, step_sz=0.1, mass=mass)
        if time.time() > deadline:
            rec['ais'] = {'skipped': 'wall budget'}
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ra = ais_glms(popn, x, seed=1, **akw)
        a_s = time.perf_counter() - t0
        sa = popn.last_fit_stats
        rec['ais'] = {'run_s': a_s, 'temperatures': int(betas.size), 'll_grad_launches': sa['ll_grad_launches'],
                      'ess': q3(ra['ess']), 'se': q3(ra['log_Z_se']),
                      'ais_minus_laplace': q3(ra['log_Z'] + ra['log_prior_norm'] - lap)}
        print(name, mass, 'ais', json.dumps(rec['ais']), file=sys.stderr, flush=True)
        # the spread over seeds
        zs, za = [res['log_Z']], [ra['log_Z']]
        for sd in range(2, seeds + 1):
            if time.time() > deadline:
                break
            zs.append(smc_glms(popn, x, seed=sd, **kw)['log_Z'])
            za.append(ais_glms(popn, x, seed=sd, **akw)['log_Z'])
        n = min(len(zs), len(za))
        rec['seeds'] = {'n': n, 'asked': seeds}
        if n > 1:
            with np.errstate(invalid='ignore'):
                rec['seeds']['smc_sd_over_seeds'] = q3(np.std(np.array(zs[:n]), axis=0, ddof=1))
                rec['seeds']['ais_sd_over_seeds'] = q3(np.std(np.array(za[:n]), axis=0, ddof=1))
                rec['seeds']['smc_mean_minus_laplace'] = q3(np.mean(np.array(zs[:n]), axis=0) + res['log_prior_norm'] - lap)
                rec['seeds']['ais_mean_minus_laplace'] = q3(np.mean(np.array(za[:n]), axis=0) + res['log_prior_norm'] - lap)
        print(name, mass, 'seeds', json.dumps(rec['seeds']), file=sys.stderr, flush=True)
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--mass', default='laplace,laplace_dense')
    ap.add_argument('--particles', type=int, default=8)
    ap.add_argument('--leapfrog', type=int, default=10)
    ap.add_argument('--steps', type=int, default=1)
    ap.add_argument('--cess', type=float, default=0.9)
    ap.add_argument('--max-stages', type=int, default=2000)
    ap.add_argument('--seeds', type=int, default=4)
    ap.add_argument('--budget-s', type=float, default=1e9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    deadline = time.time() + a.budget_s
    res = {'bench': 'smc'}
    for name in a.configs.split(','):
        res[name] = run(name, tuple(a.mass.split(',')), a.particles, a.leapfrog, a.steps, a.cess, a.max_stages, a.seeds, deadline)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(res, sort_keys=True) + '\n')
    print(json.dumps(res, sort_keys=True))
