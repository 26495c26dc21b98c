"""Rescaled inter-spike intervals on the device (pgl_rescale_dev) against the only route the library had before it -- one
pgl_state call per neuron (three (nT) host arrays each over PCIe) and a numpy cumsum of the rate -- in one process with
queued calls, as tools/hess_bench.py: C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000).

The share of the three k_rescale_* launches is the wall time of queued pgl_rescale_dev calls minus that of queued forward
passes alone (pgl_gibbs_prepare_all, whose two small uploads ride along), both measured around a stream synchronisation.
Prints one JSON line.

    python tools/gof_bench.py [--calls 5] [--warmup 2] [--out profiles/gof_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from tests import helpers as H


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
    Weff = np.ones((N, N))
    off = d.rescale_count()
    t = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(Weff)
    d_off = torch.tensor(off, dtype=torch.int64, device='cuda')
    d_tau = torch.empty((max(int(off[-1]), 1),), dtype=torch.float64, device='cuda')
    d_st = torch.empty((N, 4), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    out = {'config': name, 'N': N, 'nT': nT, 'B': B, 'P': P, 'calls': calls, 'intervals': int(off[-1]),
           'chunk_bins': _lib.RESCALE_CHUNK}
    call = lambda: d.rescale_dev(d_th.data_ptr(), d_W.data_ptr(), d_tau.data_ptr(), d_off.data_ptr(), d_st.data_ptr())

    def timed(fn):
        for _ in range(warmup):
            fn()
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    out['rescale_dev_ms'] = timed(call)
    out['kernels'] = d.last_kernels()
    out['forward_only_ms'] = timed(lambda: d.gibbs_prepare_all(theta, Weff))
    out['rescale_kernels_ms'] = out['rescale_dev_ms'] - out['forward_only_ms']
    out['rescale_kernels_over_forward'] = out['rescale_kernels_ms'] / out['forward_only_ms']
    out['rescale_kernels_below_forward'] = bool(out['rescale_kernels_ms'] < out['forward_only_ms'])
    out['gx_bytes'] = float(nT) * 16 * ((N + 15) // 16) * 8
    out['rescale_kernels_gx_read_gbps'] = out['gx_bytes'] / max(out['rescale_kernels_ms'], 1e-6) * 1e-6
    call()
    d.sync()
    tau, stats = d_tau.cpu().numpy(), d_st.cpu().numpy()
    # the route of the parent commit: N x pgl_state, cumsum and the differences at the event bins on the host
    t0 = time.perf_counter()
    ref = []
    for n in range(N):
        lam = d.state(n, theta[n], Weff[:, n])[0]
        cum = np.cumsum(lam)
        ev = np.flatnonzero(S[:, n])
        ref.append(dt * (cum[ev[1:]] - cum[ev[:-1]]))
    out['state_cumsum_ms'] = (time.perf_counter() - t0) * 1e3
    ref = np.concatenate(ref)
    out['max_rel_difference_of_the_two_routes'] = float(np.max(np.abs(tau[:ref.size] - ref) / ref))
    out['speedup'] = out['state_cumsum_ms'] / out['rescale_dev_ms']
    out['expected_over_observed_count'] = float(np.sum(stats[:, 0]) / np.sum(stats[:, 1]))
    d.close()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'gof', 'C2': run('C2', 32, 300000, a.calls, a.warmup), 'C3': run('C3', 128, 600000, a.calls, a.warmup)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
