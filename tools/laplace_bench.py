"""The Laplace set-up (inference/laplace.py) on the host route and on the device route, in one process, and the two kernels
of the device route alone.  Seeded inputs as tools/ncg_bench.py makes them, standard_glm, at the lock-step BFGS MAP fit.

    python tools/laplace_bench.py [--configs C2,C3] [--out profiles/laplace_bench.json]

C2: N = 32, nT = 300 000 (P = 161); C3: N = 128, nT = 600 000 (P = 641).  Per configuration, each the second (steady) call:
  host     laplace_glms(): hessian_s (compute_hessian_packed: device contraction, copy to the host, priors), algebra_s (the
           per-neuron loop of laplace_from_hessian), total_s; dense_factor_s: _laplace_dense_factor (Hessian, the same
           algebra and the second factorisation of the permuted covariance)
  device   laplace_glms(device=True): hessian_s (contraction, priors uploaded and permuted), factor_s, inverse_s (the two
           kernels with the torch gathers around them), rest_s (log posterior, copies of the small results), total_s;
           dense_factor_s: _laplace_dense_factor_device
  kernels  pgl_chol_factor_dev and pgl_tri_inverse_dev alone on the same stack: ms and GFLOP/s (P^3 / 3 flops per matrix each)
  agreement  max relative difference of the standard errors and max absolute difference of the log evidences
  device_stage_faster   factor_s + inverse_s < host algebra_s
Records, sets no threshold.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS, population


def run(name):
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference import batched_hmc as BH
    from theano_pyglm_amd.inference import laplace as LP
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    fit_glms_batched_torch(popn, x)
    P = popn.glm.P
    out = {'config': name, 'N': N, 'nT': nT, 'P': P}
    clock = time.perf_counter
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = clock()
        H = popn.compute_hessian_packed(x)
        t1 = clock()
        lps, _ = popn.compute_lp_grad_packed(x)
        t2 = clock()
        host = [LP.laplace_from_hessian(-0.5 * (H[i] + H[i].T), lps[i]) for i in range(N)]
        t3 = clock()
        out['host'] = {'hessian_s': t1 - t0, 'log_post_s': t2 - t1, 'algebra_s': t3 - t2, 'total_s': t3 - t0}
        t0 = clock()
        BH._laplace_dense_factor(popn, x, 0, N, 1e-8)
        out['host']['dense_factor_s'] = clock() - t0
    for rep in range(2):
        torch.cuda.synchronize()
        tm = {}
        t0 = clock()
        LP.laplace_on_device(popn, x, timings=tm)
        t1 = clock()
        dev = LP.laplace_glms(popn, x, device=True)
        t2 = clock()
        Wd, dense = BH._laplace_dense_factor_device(popn, x, 0, N, 1e-8)
        torch.cuda.synchronize()
        t3 = clock()
        out['device'] = {'hessian_s': tm['hessian'], 'factor_s': tm['factor'], 'inverse_s': tm['inverse'],
                         'stages_total_s': t1 - t0, 'total_s': t2 - t1, 'rest_s': (t2 - t1) - (t1 - t0),
                         'dense_factor_s': t3 - t2, 'dense_rows': int(dense.sum())}
    del Wd
    pd = np.array([h['pd'] and d['pd'] for h, d in zip(host, dev)])
    out['pd_rows'] = {'host': int(sum(h['pd'] for h in host)), 'device': int(sum(d['pd'] for d in dev))}
    if pd.any():
        out['agreement'] = {
            'stderr_rel': float(max(np.max(np.abs(d['stderr_vec'] - h['stderr_vec']) / h['stderr_vec'])
                                    for h, d, ok in zip(host, dev, pd) if ok)),
            'log_evidence_abs': float(max(abs(d['log_evidence'] - h['log_evidence']) for h, d, ok in zip(host, dev, pd) if ok))}
    out['device_stage_faster'] = bool(out['device']['factor_s'] + out['device']['inverse_s'] < out['host']['algebra_s'])
    out['algebra_speedup'] = out['host']['algebra_s'] / (out['device']['factor_s'] + out['device']['inverse_s'])
    # the kernels alone, on the (reversed is immaterial) stack of minus the Hessians in the packed order
    h0 = popn._handle(popn.data_sequences[0])
    dev_t = torch.device('cuda', popn.device)
    A0 = torch.tensor(-0.5 * (H + np.swapaxes(H, 1, 2)), dtype=torch.float64, device=dev_t)
    flops = N * P ** 3 / 3.0
    kern = {}
    for rep in range(3):
        A = A0.clone()
        torch.cuda.synchronize()
        t0 = clock()
        _, _, info = h0.chol_factor(A)
        h0.sync()
        t1 = clock()
        h0.tri_inverse(A, info)
        h0.sync()
        t2 = clock()
        kern = {'factor_ms': (t1 - t0) * 1e3, 'inverse_ms': (t2 - t1) * 1e3, 'factor_gflops': flops / (t1 - t0) / 1e9,
                'inverse_gflops': flops / (t2 - t1) / 1e9, 'failed_rows': int((info != 0).sum().item())}
    out['kernels'] = kern
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'laplace'}
    for name in a.configs.split(','):
        res[name] = run(name)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
