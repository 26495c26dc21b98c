"""Dense Hessian (pgl_hess_dev) against the only route the library had before it -- P Hessian-vector products on identity
columns (pgl_hvp_apply_dev) after the same prepare -- in one process with queued calls, as tools/hvp_bench.py: C3
(N = 128, nT = 600 000), C2 (N = 32, nT = 300 000) and a single neuron of C3.  Flops: the Gram contraction over one
triangle nT P^2 per row (the products: 4 nT N B flops per row and apply), fractions of the 78.6 TFLOP/s f64 MFMA peak.  Prints one JSON line.

    python tools/hess_bench.py [--calls 3] [--warmup 1] [--out profiles/hess_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from tests import helpers as H

PEAK = 78.6e12


def run(name, N, nT, rows, calls, warmup):
    import torch
    rng = np.random.default_rng(1234)
    B, R, dt = 5, 200, 0.001
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    d = _lib.DeviceGlm(N, nT, B, R, 'explinear', dt, 0)
    d.set_spikes(S)
    d.set_basis(H.std_ibasis(R))
    d.set_option(_lib.OPT_TIMING, 0)
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    P = d.P
    theta = np.zeros((rows, P))
    theta[:, 0] = 20.0 + 0.3 * rng.standard_normal(rows)
    theta[:, 1:] = 0.05 * rng.standard_normal((rows, P - 1))
    t = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(np.ones((N, N)))
    d_H = torch.empty((rows, P, P), dtype=torch.float64, device='cuda')
    d_E = t(np.eye(P))                                     # row k: the identity column every row of apply k is given
    d_v = torch.empty((rows, P), dtype=torch.float64, device='cuda')
    d_hv = torch.empty((P, rows, P), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    out = {'config': name, 'N': N, 'nT': nT, 'B': B, 'P': P, 'rows': rows, 'calls': calls}
    d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), 0, rows)
    d.sync()
    out['hvp_prepare_kernels'] = d.last_kernels()
    for _ in range(warmup):
        d.hess(d_H.data_ptr(), P)
    d.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        d.hess(d_H.data_ptr(), P)
    d.sync()
    out['hess_ms'] = (time.perf_counter() - t0) / calls * 1e3
    out['hess_kernels'] = d.last_kernels()
    # the identity-column route, once: P applies queued back to back (the copies of the columns ride on torch's stream,
    # made before the clock starts)
    vs = d_E[:, None, :].expand(P, rows, P).contiguous()
    torch.cuda.synchronize()
    for k in range(min(warmup, P)):
        d.hvp_apply(vs[k].data_ptr(), d_hv[k].data_ptr())
    d.sync()
    t0 = time.perf_counter()
    for k in range(P):
        d.hvp_apply(vs[k].data_ptr(), d_hv[k].data_ptr())
    d.sync()
    out['identity_columns_ms'] = (time.perf_counter() - t0) * 1e3
    out['hvp_apply_kernels'] = d.last_kernels()
    Hh = d_H.cpu().numpy()
    Hc = d_hv.cpu().numpy().transpose(1, 2, 0)             # [row][i][k] = (H e_k)[i]
    out['max_rel_difference_of_the_two_routes'] = float(np.max(np.abs(Hh - Hc)) / np.max(np.abs(Hc)))
    out['hess_flops'] = float(nT) * P * P * rows
    out['identity_columns_flops'] = 4.0 * nT * N * B * rows * P
    out['hess_fraction_of_f64_mfma_peak'] = out['hess_flops'] / (out['hess_ms'] * 1e-3) / PEAK
    out['identity_columns_fraction_of_f64_mfma_peak'] = out['identity_columns_flops'] / (out['identity_columns_ms'] * 1e-3) / PEAK
    out['speedup'] = out['identity_columns_ms'] / out['hess_ms']
    d.close()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'hess', 'peak_flops': PEAK,
           'C2': run('C2', 32, 300000, 32, a.calls, a.warmup),
           'C3_one_neuron': run('C3_one_neuron', 128, 600000, 1, a.calls, a.warmup),
           'C3': run('C3', 128, 600000, 128, a.calls, a.warmup)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
