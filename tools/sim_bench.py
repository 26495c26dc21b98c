"""Batched simulation on the device (pgl_simulate_batch_dev, one workgroup per replicate) against the only route the library
had before it: one pgl_simulate call per spike train on the host.  C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000)
on a seeded standard_glm draw that passes check_stability (the draw of harness/generate_synth_data.make_dataset).

Per configuration: wall time of the device call for n_rep = 1, one replicate per CU and four per CU with only the counts
coming back; of one replicate with its spikes copied to the host; of ONE pgl_simulate call on this machine's CPU -- the host
figure for n_rep replicates is that time multiplied by n_rep, an EXTRAPOLATION, and labelled so; microseconds per bin and
replicate; the spike rate of the draw (the cost of a bin grows with its spikes: each adds an N x R block to the ring).
No speedup is assumed: the ratios are reported as measured, the losing ones too.

Every configuration runs in a child process under a time limit.  Prints one JSON line.

    python tools/sim_bench.py [--configs C2,C3] [--per-cu 1,4] [--timeout 900] [--out profiles/sim_bench.json]"""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'C2': (32, 300000), 'C3': (128, 600000)}
SEED = 1234


def inputs(N, nT, dt=0.001, dt_stim=0.1):
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity, check_stability
    from theano_pyglm_amd.population import Population
    rng = np.random.RandomState(SEED + N)
    model = stabilize_sparsity(make_model('standard_glm', N=N, dt=dt))
    popn = Population(model)
    x = popn.sample(rng)
    assert check_stability(model, x, N), "the sampled network is unstable"
    T = nT * dt
    stim = rng.randn(int(round(T / dt_stim)), model['bkgd'].get('D_stim', 1))
    X0, AW = popn._simulation_inputs(x, (0.0, T), dt, stim, dt_stim, nT=nT)
    return X0, np.ascontiguousarray(np.transpose(AW, (0, 2, 1))), popn.glm.nlin_model.kind, dt


def worker(name, per_cu):
    import torch
    from theano_pyglm_amd import _lib
    N, nT = CONFIGS[name]
    X0, AW, kind, dt = inputs(N, nT)
    R = AW.shape[1]
    in_lds, ws_bytes = _lib.simulate_batch_plan(N, R)
    out = {'config': name, 'N': N, 'nT': nT, 'R': R, 'nlin': kind, 'ring_in_lds': in_lds, 'ring_bytes': R * N * 8}
    # the parent commit's route: one pgl_simulate call (its own generator: the reference's draw order)
    t0 = time.perf_counter()
    S, _, n_exc = _lib.simulate(X0, AW, kind, dt, seed=SEED)
    out['host_pgl_simulate_s'] = time.perf_counter() - t0
    out['host_us_per_bin'] = out['host_pgl_simulate_s'] / nT * 1e6
    out['spikes_per_bin'] = float(S.sum() / nT)
    out['rate_hz_mean'] = float(S.sum() / (nT * dt) / N)
    out['host_exceptions'] = n_exc
    del S
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out['compute_units'] = cus
    d_X0, d_AW = torch.from_numpy(X0).cuda(), torch.from_numpy(AW).cuda()

    def run(n_rep, spikes=False):
        d_c = torch.empty((n_rep, N), dtype=torch.int64, device='cuda')
        d_e = torch.empty(n_rep, dtype=torch.int64, device='cuda')
        d_ws = None if in_lds else torch.empty(n_rep * ws_bytes // 8, dtype=torch.float64, device='cuda')
        d_S = torch.empty((n_rep, nT, N), dtype=torch.uint8, device='cuda') if spikes else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.simulate_batch_dev(N, nT, R, kind, dt, d_X0.data_ptr(), d_AW.data_ptr(), n_rep, d_c.data_ptr(), d_e.data_ptr(),
                                seed=SEED, d_S=d_S.data_ptr() if spikes else 0, d_workspace=0 if d_ws is None else d_ws.data_ptr())
        torch.cuda.synchronize()
        counts = d_c.cpu().numpy()
        host_S = d_S.cpu().numpy() if spikes else None
        wall = time.perf_counter() - t0
        if spikes:
            assert np.array_equal(host_S.sum(axis=1, dtype=np.int64), counts)
        return wall, counts, int(d_e.cpu().numpy().sum())

    run(1)                                                        # warm-up: code object load, allocator
    runs = []
    for n_rep in [1] + [k * cus for k in per_cu]:
        wall, counts, exc = run(n_rep)
        runs.append({'n_rep': n_rep, 'device_s': wall, 'device_us_per_bin_per_rep': wall / nT / n_rep * 1e6,
                     'host_s_extrapolated': out['host_pgl_simulate_s'] * n_rep, 'host_is_extrapolated': n_rep > 1,
                     'host_over_device': out['host_pgl_simulate_s'] * n_rep / wall,
                     'device_wins': bool(out['host_pgl_simulate_s'] * n_rep > wall),
                     'spikes_per_bin': float(counts.sum() / nT / n_rep), 'exceptions': exc})
    out['counts_only'] = runs
    wall, _, _ = run(1, spikes=True)
    out['one_replicate_with_spikes_s'] = wall
    out['one_replicate_with_spikes_host_over_device'] = out['host_pgl_simulate_s'] / wall
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--per-cu', default='1,4', help='replicates per CU of the large runs')
    ap.add_argument('--timeout', type=int, default=900, help='seconds a configuration may take (child process)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    per_cu = [int(v) for v in a.per_cu.split(',') if v]
    if a.worker:
        print('RESULT ' + json.dumps(worker(a.worker, per_cu), sort_keys=True))
        sys.exit(0)
    import __graft_entry__ as ge
    ge.build_hip()
    res = {'bench': 'sim'}
    for name in a.configs.split(','):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', name, '--per-cu', a.per_cu],
                           stdout=subprocess.PIPE, timeout=a.timeout, check=True)
        res[name] = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('RESULT ')][-1][7:])
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
