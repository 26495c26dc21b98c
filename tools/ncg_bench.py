"""One lock-step Newton-CG sweep (inference/batched_newton_cg.py) per configuration, next to the lock-step BFGS sweep and
the sequential use_rop sweep of the same build, in one process: wall time of the second (steady) call, per-row nit / nhev
distribution, launch counts.  Seeded inputs as tools/hvp_bench.py makes them (Poisson spikes at 20 Hz), standard_glm.

    python tools/ncg_bench.py --config C3 [--sequential 8] [--out profiles/ncg_bench_C3.json]

C1: N = 4, nT = 60 000; C2: N = 32, nT = 300 000; C3: N = 128, nT = 600 000.  --sequential K also times
coord_descent's sequential use_rop fits of the first K neurons (fit_glm(use_rop=True) each) and scales the time by N / K
(labelled as scaled).  Prints one JSON line."""
import argparse, copy, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'C1': (4, 60000), 'C2': (32, 300000), 'C3': (128, 600000)}


def population(N, nT, seed=1234):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model('standard_glm', N=N, dt=0.001))
    rng = np.random.default_rng(seed)
    S = np.minimum(rng.poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': nT * 0.001, 'stim': None, 'dt_stim': 0.1})
    return popn


def dist(v):
    v = np.asarray(v)
    return {'min': int(v.min()), 'median': float(np.median(v)), 'max': int(v.max()), 'sum': int(v.sum())}


def run(name, n_seq):
    import torch
    from theano_pyglm_amd.inference import coord_descent as cd
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference.batched_newton_cg import fit_glms_newton_cg_torch
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x0 = popn.sample(np.random.RandomState(4321))
    out = {'config': name, 'N': N, 'nT': nT}
    for rep in range(2):                                       # the second call is the steady one
        x = copy.deepcopy(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fun, nit, nfev, nhev, status = fit_glms_newton_cg_torch(popn, x)
        out['newton_cg_s'] = time.perf_counter() - t0
    st = popn.last_fit_stats
    out.update({'newton_cg_nlp_sum': float(fun.sum()), 'nit': dist(nit), 'nhev': dist(nhev),
                'status_counts': dict((str(k), int(c)) for k, c in zip(*np.unique(status, return_counts=True))),
                'apply_launches': st['apply_launches'], 'prepare_launches': st['prepare_launches'],
                'll_grad_launches': st['ll_grad_launches'], 'outer_iterations': st['outer_iterations']})
    for rep in range(2):
        x = copy.deepcopy(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fb, itb, evb = fit_glms_batched_torch(popn, x)
        out['bfgs_s'] = time.perf_counter() - t0
    out.update({'bfgs_nlp_sum': float(fb.sum()), 'bfgs_iterations': int(itb), 'bfgs_evaluations': int(evb)})
    if n_seq:
        prms = cd.prep_first_order_glm_inference(popn)
        hessp = cd.prep_second_order_glm_inference(popn)
        t0 = time.perf_counter()
        fs, nhs = [], []
        for n in range(n_seq):
            nv = popn.extract_vars(copy.deepcopy(x0), n)
            res = cd.fit_glm(nv, n, prms, use_rop=True, hessp=hessp)
            fs.append(float(res.fun))
            nhs.append(int(res.nhev))
        t = time.perf_counter() - t0
        out.update({'sequential_neurons': n_seq, 'sequential_s': t, 'sequential_scaled_to_N_s': t * N / n_seq,
                    'sequential_scaled': n_seq != N, 'sequential_nhev': dist(nhs),
                    'sequential_nlp_sum': float(np.sum(fs)), 'newton_cg_nlp_sum_same_neurons': float(fun[:n_seq].sum()),
                    'speedup_over_sequential': t * N / n_seq / out['newton_cg_s']})
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3', choices=sorted(CONFIGS))
    ap.add_argument('--sequential', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    line = json.dumps({'bench': 'ncg', a.config: run(a.config, a.sequential)}, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
