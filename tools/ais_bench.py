"""The annealed importance sampling run (inference/batched_ais.py) per configuration, next to its floor, in one process.
Seeded inputs as tools/ncg_bench.py makes them (Poisson spikes at 20 Hz), standard_glm with the impulse prior replaced by
the Gaussian N(0, 1) -- the template's group lasso is not served: AIS starts from an exact prior draw -- started at the
lock-step BFGS MAP fit, Laplace mass.

    python tools/ais_bench.py [--configs C2,C3] [--mass laplace,laplace_dense] [--out profiles/ais_bench.json]

C2: N = 32, nT = 300 000; C3: N = 128, nT = 600 000.  Per configuration:
  run_s            wall time of ais_glms (K particles and the pilot; the mass is computed before, outside the clock)
  floor_s          the same number of bare pgl_ll_grad_dev calls of all rows on the same stream, in the same process
  run_over_floor   their ratio
  row_s            the row launches of the same run alone (every pgl_ais_* launch, no evaluation in between)
  neurons          per neuron: log_Z + log_prior_norm, its standard error, the ESS and the Laplace log evidence
  mass             with --mass laplace,laplace_dense: the same fit, seed, ladder, K and n_leapfrog under both masses in this
                   process -- per mass: wall time, launches, the ratio to the floor, accept rate and median step per
                   temperature, median ESS and standard error, AIS minus Laplace; for the dense mass also the seconds of
                   its factorisations and of its product launches alone, and dense_over_laplace, the ratio of the two runs
Records, sets no threshold.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS


def population(N, nT, seed=1234):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=N, dt=0.001)
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    popn = Population(model)
    rng = np.random.default_rng(seed)
    S = np.minimum(rng.poisson(20.0 * 0.001, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': 0.001, 'T': nT * 0.001, 'stim': None, 'dt_stim': 0.1})
    return popn


def row_launches_alone(popn, K, M, P, prm, betas, n_steps, n_leapfrog, with_pilot):
    """Seconds of every row launch of one run (the pilot's included), on zeroed evaluations."""
    import torch
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    f64 = torch.float64
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    J = len(betas) - 1
    try:
        with torch.cuda.stream(stream):
            total = 0.0
            for Kr, adapt in ([(1, True)] if with_pilot else []) + [(K, False)]:
                R = Kr * M
                st = torch.zeros(h.ais_state_doubles(R, P), dtype=f64, device=dev)
                Xt = torch.empty((R, P), dtype=f64, device=dev)
                buf = torch.zeros(R * (1 + P), dtype=f64, device=dev)
                acc = torch.zeros((J - 1, R), dtype=f64, device=dev)
                tab = torch.full((J - 1, M), 1e-3, dtype=f64, device=dev)
                ll, g, sp = buf.data_ptr(), buf[R:].data_ptr(), st.data_ptr()
                stream.synchronize()
                t0 = time.perf_counter()
                h.ais_init_dev(sp, Kr, M, P, 0, 0, prm, 1e-3, 1, Xt.data_ptr())
                h.ais_start_dev(sp, Kr, M, P, ll, g, prm)
                for j in range(1, J + 1):
                    h.ais_temper_dev(sp, Kr, M, P, prm, betas[j], tab[j - 1].data_ptr() if (j < J and not adapt) else 0)
                    if j == J:
                        break
                    for _ in range(n_steps):
                        h.ais_begin_dev(sp, Kr, M, P, 0, Xt.data_ptr())
                        for i in range(n_leapfrog):
                            h.ais_leap_dev(sp, Kr, M, P, 0, ll, g, prm, i == n_leapfrog - 1, adapt, Xt.data_ptr(),
                                           acc[j - 1].data_ptr(), 0)
                stream.synchronize()
                total += time.perf_counter() - t0
            return total
    finally:
        h.set_stream(None)


def summary(res, lap, N):
    """What a run says about the evidence: per-temperature accept rate and median step, ESS, standard error, AIS - Laplace."""
    fin = lambda v: float(v) if np.isfinite(v) else None
    d = np.array([res['log_Z'][n] + res['log_prior_norm'][n] - lap[n]['log_evidence'] for n in range(N)])
    ok = np.isfinite(d)
    return {'accept_rate_per_temperature': [float(v) for v in res['accept_rate'].mean(axis=1)],
            'step_median_per_temperature': [float(v) for v in np.median(res['step_sz'], axis=1)],
            'accept_rate': {'min': float(res['accept_rate'].min()), 'mean': float(res['accept_rate'].mean())},
            'ess_median': float(np.median(res['ess'])), 'ess_min': float(np.min(res['ess'])), 'ess_max': float(np.max(res['ess'])),
            'se_median': fin(np.nanmedian(res['log_Z_se'])),
            'ais_minus_laplace': {'rows': int(ok.sum()), 'min': fin(np.min(d[ok])) if ok.any() else None,
                                  'median': fin(np.median(d[ok])) if ok.any() else None,
                                  'max': fin(np.max(d[ok])) if ok.any() else None}}


def dense_parts_alone(popn, x, K, N, P, betas, st):
    """Seconds of the dense run's own work alone: its factorisations (tempered_factor, as many as the run made) and its
    product launches (pgl_tri_matvec_shared_dev, half of them with the pilot's one particle, half with K)."""
    import torch
    from theano_pyglm_amd.inference import batched_ais as BA
    from theano_pyglm_amd.inference.batched_bfgs import _Packing
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    f64 = torch.float64
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            pk = _Packing(popn, torch, [h], (0, N))
            t0 = time.perf_counter()
            G = BA._ll_hessians(popn, torch, dev, [h], x, 0, N, P)
            stream.synchronize()
            hess_s = time.perf_counter() - t0
            lam = torch.tensor(BA.prior_precision(pk.prior_params(), N, pk.B, pk.nbk), dtype=f64, device=dev)
            eye = torch.eye(P, dtype=f64, device=dev)

            def chol(Ar):
                Ar = Ar.contiguous()
                return (Ar,) + h.chol_factor(Ar)

            def tri_inv(Ls, info):
                h.tri_inverse(Ls, info)
                return Ls
            W = None
            for timed in (False, True):                         # (once to warm the allocator, then the clock)
                stream.synchronize()
                t0 = time.perf_counter()
                for i in range(st['factorisations'] if timed else 1):
                    W, _ = BA.tempered_factor(G, lam, float(betas[1 + i % (len(betas) - 2)]), 1e-8, chol, tri_inv, torch, eye)
                stream.synchronize()
                factor_s = time.perf_counter() - t0
            xs = torch.randn((K * N, P), dtype=f64, device=dev)
            ys = torch.empty((K * N, P), dtype=f64, device=dev)
            half = st['product_launches'] // 2
            stream.synchronize()
            t0 = time.perf_counter()
            for Kr in (1, K):
                for i in range(half):
                    h.tri_matvec_shared_dev(W.data_ptr(), N, Kr, P, i & 1, xs.data_ptr(), ys.data_ptr())
            stream.synchronize()
            return {'hessian_s': hess_s, 'factor_s': factor_s, 'product_s': time.perf_counter() - t0}
    finally:
        h.set_stream(None)


def run(name, K, n_temps, n_steps, n_leapfrog, masses=('laplace',)):
    import torch
    from theano_pyglm_amd.inference.batched_ais import ais_glms, reference_ladder
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch, _Packing
    from theano_pyglm_amd.inference.batched_hmc import _laplace_minv
    from theano_pyglm_amd.inference.laplace import laplace_glms
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    fit_glms_batched_torch(popn, x)
    betas = reference_ladder(n_temps)
    out = {'config': name, 'N': N, 'nT': nT, 'n_particles': K, 'n_temps': int(betas.size), 'n_steps': n_steps,
           'n_leapfrog': n_leapfrog, 'impulse_prior': 'gaussian(0, 1)'}
    t0 = time.perf_counter()
    minv = _laplace_minv(popn, x, 0, N, 1e-8)                   # what mass='laplace' computes: once, outside the clock
    out['laplace_mass_s'] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ais_glms(popn, x, n_particles=K, betas=betas, n_steps=n_steps, n_leapfrog=n_leapfrog, step_sz=0.1, mass=minv, seed=1)
    out['run_s'] = time.perf_counter() - t0
    st = popn.last_fit_stats
    out['launches'] = {k: st[k] for k in ('ll_grad_launches', 'row_launches', 'host_syncs_in_run')}
    # the floor: the same number of bare evaluations
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    P = popn.glm.P
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
        out['floor_s'] = time.perf_counter() - t0
    finally:
        h.set_stream(None)
    out['run_over_floor'] = out['run_s'] / out['floor_s']
    out['row_s'] = row_launches_alone(popn, K, N, P, _Packing(popn, None).prior_params(), betas, n_steps, n_leapfrog, True)
    out['row_share_of_run'] = out['row_s'] / out['run_s']
    out['accept_rate'] = {'min': float(res['accept_rate'].min()), 'mean': float(res['accept_rate'].mean())}
    out['step_sz'] = {'min': float(res['step_sz'].min()), 'median': float(np.median(res['step_sz'])),
                      'max': float(res['step_sz'].max())}
    lap = laplace_glms(popn, x)
    fin = lambda v: float(v) if np.isfinite(v) else None
    if 'laplace_dense' in masses:
        cmp_ = {'laplace': dict(summary(res, lap, N), run_s=out['run_s'], run_over_floor=out['run_over_floor'],
                                launches=out['launches'])}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = ais_glms(popn, x, n_particles=K, betas=betas, n_steps=n_steps, n_leapfrog=n_leapfrog, step_sz=0.1,
                      mass='laplace_dense', seed=1)
        run_s = time.perf_counter() - t0                        # (the Hessians of ll are inside this clock)
        sd = popn.last_fit_stats
        assert sd['ll_grad_launches'] == st['ll_grad_launches']
        dense = dict(summary(rd, lap, N), run_s=run_s, run_over_floor=run_s / out['floor_s'],
                     launches={k: sd[k] for k in ('ll_grad_launches', 'row_launches', 'factorisations', 'product_launches',
                                                  'host_syncs_in_run')},
                     dense_rows_share=float(rd['dense_rows'].mean()))
        dense.update(dense_parts_alone(popn, x, K, N, P, betas, sd))
        cmp_['laplace_dense'] = dense
        cmp_['dense_over_laplace'] = run_s / out['run_s']
        out['mass'] = cmp_
    out['neurons'] = [{'n': n, 'ais_log_evidence': fin(res['log_Z'][n] + res['log_prior_norm'][n]), 'se': fin(res['log_Z_se'][n]),
                       'ess': fin(res['ess'][n]), 'laplace_log_evidence': fin(lap[n]['log_evidence'])} for n in range(N)]
    d = np.array([(r['ais_log_evidence'] - r['laplace_log_evidence']) if None not in (r['ais_log_evidence'], r['laplace_log_evidence'])
                  else np.nan for r in out['neurons']])
    ok = np.isfinite(d)
    out['ais_minus_laplace'] = {'rows': int(ok.sum()), 'min': fin(np.min(d[ok])) if ok.any() else None,
                                'median': fin(np.median(d[ok])) if ok.any() else None, 'max': fin(np.max(d[ok])) if ok.any() else None}
    out['ess_median'] = float(np.median(res['ess']))
    out['se_median'] = fin(np.nanmedian(res['log_Z_se']))
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--particles', type=int, default=8)
    ap.add_argument('--temps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=1)
    ap.add_argument('--leapfrog', type=int, default=10)
    ap.add_argument('--mass', default='laplace', help="laplace (the record as it was) or laplace,laplace_dense (adds the "
                    "comparison under the key 'mass')")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    masses = tuple(a.mass.split(','))
    if 'laplace' not in masses or not set(masses) <= {'laplace', 'laplace_dense'}:
        ap.error("--mass: laplace or laplace,laplace_dense")
    res = {'bench': 'ais'}
    for name in a.configs.split(','):
        res[name] = run(name, a.particles, a.temps, a.steps, a.leapfrog, masses)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
