"""Hessian-vector product against ll+grad of the same build, in one process: ms per pgl_ll_grad_dev, per
pgl_hvp_prepare_dev and per pgl_hvp_apply_dev at C3 (N = 128, nT = 600 000) and C2 (N = 32, nT = 300 000), the kernels
launched, and the apply's fraction of the 78.6 TFLOP/s f64 MFMA peak counted with 4 nT N^2 B flops.  Timing as
tools/map_bench.py / bench.py: warm-up, then the synchronised wall time over `--calls` queued calls (no per-call events).
Prints one JSON line.

    python tools/hvp_bench.py [--calls 20] [--warmup 3] [--out profiles/hvp_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from tests import helpers as H

PEAK = 78.6e12


def timed(fn, sync, calls, warmup):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls * 1e3


def run(name, N, nT, calls, warmup):
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
    theta = np.zeros((N, P))
    theta[:, 0] = 20.0 + 0.3 * rng.standard_normal(N)
    theta[:, 1:] = 0.05 * rng.standard_normal((N, P - 1))
    t = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    d_th, d_W, d_v = t(theta), t(np.ones((N, N))), t(rng.standard_normal((N, P)))
    d_ll, d_g, d_hv = torch.empty(N, dtype=torch.float64, device='cuda'), torch.empty_like(d_th), torch.empty_like(d_th)
    torch.cuda.synchronize()
    out = {'config': name, 'N': N, 'nT': nT, 'B': B, 'calls': calls}
    out['ll_grad_ms'] = timed(lambda: d.ll_grad_dev(d_th.data_ptr(), d_W.data_ptr(), d_ll.data_ptr(), d_g.data_ptr()),
                              d.sync, calls, warmup)
    out['ll_grad_kernels'] = d.last_kernels()
    out['hvp_prepare_ms'] = timed(lambda: d.hvp_prepare(d_th.data_ptr(), d_W.data_ptr()), d.sync, calls, warmup)
    out['hvp_prepare_kernels'] = d.last_kernels()
    out['hvp_apply_ms'] = timed(lambda: d.hvp_apply(d_v.data_ptr(), d_hv.data_ptr()), d.sync, calls, warmup)
    out['hvp_apply_kernels'] = d.last_kernels()
    flops = 4.0 * nT * N * N * B
    out['apply_over_ll_grad'] = out['hvp_apply_ms'] / out['ll_grad_ms']
    out['apply_fraction_of_f64_mfma_peak'] = flops / (out['hvp_apply_ms'] * 1e-3) / PEAK
    out['ll_grad_fraction_of_f64_mfma_peak'] = flops / (out['ll_grad_ms'] * 1e-3) / PEAK
    d.close()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'hvp', 'peak_flops': PEAK,
           'C3': run('C3', 128, 600000, a.calls, a.warmup), 'C2': run('C2', 32, 300000, a.calls, a.warmup)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
