#!/usr/bin/env python
"""
bench.py -- population GLM ll+grad evals/s on MI355X (BASELINE.json metric).

One "step" = one population log-likelihood + gradient evaluation: for every
post-synaptic neuron n, ll_n and d ll_n / d theta_n (theta_n = bias + N*B impulse
weights) on a spike matrix already resident in HBM.  Workload at
every GPU count: standard_glm, N=128 neurons, T=600 s at 1 ms bins (C3, the
configuration the north-star target is quoted on), synthetic Poisson spikes.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints one JSON line (headline, ms_per_step, and the roofline of
the HIP events sampled inside the timed region).  --dump-outputs DIR writes the ll and gradient of the last timed step
as DIR/ll.npy and DIR/grad.npy (float64; the inputs are seeded, so two builds can be compared output for output).
--full adds everything else behind the timed region: the A/B loops, the narrow-shard step, the MAP / MCMC / stimulus
secondaries, the PMC traffic figures, the CPU baselines and, on N > 1 ranks, the neuron-sharded step, the sharded MAP
sweep and the check of the sharded evaluation against the single-rank one (the --no-* options prune that set).

`python bench.py --gpus N` with N > 1 and no launcher (WORLD_SIZE unset) starts the N ranks itself: the parent --
before torch or HIP are touched -- builds the library, spawns N fresh `python bench.py ...` processes with
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, relays rank 0's JSON record as the last line of stdout and exits
non-zero if any rank did.

N>1 (total work fixed -> "scaling": "strong"), two shardings of the same evaluation:
  --shard time (default): every rank evaluates all N neurons on its own range of time bins
      (the likelihood is additive over time segments, population.py:41-43; features reach R bins
      back, so the 77 MB spike matrix is replicated) and one RCCL all-reduce sums the packed
      (ll, grad) block (N x (1+P) doubles = 657 KB).  This is the time x neuron split SURVEY
      §8(e) prescribes when neuron sharding alone scales < 6x: feature generation is divided
      too, whereas with neurons sharded every GPU regenerates all features.
  --shard neurons: post-synaptic neurons block-partitioned (the reference's own pattern,
      parallel_coord_descent.py:137-147), all-gather of the per-neuron ll (1 KB) per step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix peak (BASELINE.md §4 / SURVEY.md §8d)


def make_workload(N, T, dt, seed):
    """C2-C5 synthetic inputs: S ~ Poisson(20 Hz * dt) clipped to 10, uint8;
    bias ~ N(20, 0.1) (standard_glm.py:16-21); w_ir ~ N(0, 0.5)."""
    rng = np.random.default_rng(seed)
    nT = int(round(T / dt))
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    return S


def make_theta(N, P, seed=99):
    """Parameters of every neuron (bias | impulse weights), seeded like the workload."""
    rng = np.random.default_rng(seed)
    theta = np.zeros((N, P))
    theta[:, 0] = 20.0 + 0.1 * rng.standard_normal(N)
    theta[:, 1:] = 0.5 * rng.standard_normal((N, P - 1))
    return theta


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """Write every array as out_dir/<name>.npy in float64.  When the total would exceed `limit`, the 2-D arrays keep
    every k-th row (k fixed by the sizes alone), so that two runs with the same arguments write the same rows."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = dict((k, np.ascontiguousarray(v, dtype=np.float64)) for k, v in arrays.items())
    rows = max([a.shape[0] for a in arrays.values() if a.ndim >= 2] or [1])
    stride = 1
    while stride < rows and sum((a[::stride] if a.ndim >= 2 else a).nbytes for a in arrays.values()) > limit:
        stride += 1
    arrays = dict((k, a[::stride] if a.ndim >= 2 else a) for k, a in arrays.items())
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)
    return arrays


def standard_ibasis(R=200):
    """standard_glm impulse basis: the committed 100-point orthonormal cosine basis
    (tests/golden, produced by the reference's create_basis) interpolated to R taps
    (impulse.py:92-103)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'basis_golden.npz'))
    basis = g['std_imp_basis']
    L, B = basis.shape
    ib = np.zeros((R, B))
    for b in range(B):
        ib[:, b] = np.interp(np.linspace(0, 1, R), np.linspace(0, 1, L), basis[:, b])
    return ib


def pmc_traffic(kernel_prefixes, fetch_scale=2.0):
    """HBM bytes per evaluation of the dominant kernel(s) from the committed rocprofv3 PMC summary
    (separate --pmc FETCH_SIZE / WRITE_SIZE passes of this same command, tools/profile_bench.sh).
    The hot path is two launches of one kernel template (pass 1 / pass 2): their bytes are summed.
    gfx950 correction (MI355X_MICROARCH.md, HBM section): FETCH_SIZE reports exactly half of the
    bytes of wide coalesced streaming reads (16 B per lane, global_load and LDS-DMA alike); the
    reads of k_fused5 are such streams (feature tiles by global_load_lds_dwordx4, Wmat fragments by
    global_load_dwordx4), so FETCH_SIZE is doubled -- cross-check: pass 2 then reads 2.14 GB against
    1.57 GB of feature tiles + 0.61 GB of residuals.  WRITE_SIZE is taken at face value (8-byte
    stores; pass 1 writes 0.69 GB = 0.61 GB residual slab + 0.08 GB of G partials).
    The newest top-level profiles/rNN_pmc.json wins (earlier iterations live in profiles/history/)."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_pmc.json'))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        tot, found = 0.0, 0
        for pref in kernel_prefixes:
            for k, v in d.items():
                if k.startswith(pref) and 'FETCH_SIZE' in v and 'WRITE_SIZE' in v:
                    tot += (fetch_scale * v['FETCH_SIZE']['avg'] + v['WRITE_SIZE']['avg']) * 1024.0
                    found += 1
                    break
        if found == len(kernel_prefixes):
            best = (f, tot)
    return best


def pmc_mfma_busy(kernel_prefixes, n_xcd=8, n_simd=1024):
    """MFMA pipe utilisation of the hot kernels from the committed PMC summary (the definition of
    rocprofv3's derived MfmaUtil): sum SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE per XCD x SIMDs).
    GRBM_GUI_ACTIVE is reported summed over the 8 XCDs."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_pmc.json'))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        busy, act, found = 0.0, 0.0, 0
        for pref in kernel_prefixes:
            for k, v in d.items():
                if k.startswith(pref) and 'SQ_VALU_MFMA_BUSY_CYCLES' in v and 'GRBM_GUI_ACTIVE' in v:
                    busy += v['SQ_VALU_MFMA_BUSY_CYCLES']['avg']
                    act += v['GRBM_GUI_ACTIVE']['avg']
                    found += 1
                    break
        if found == len(kernel_prefixes) and act > 0:
            best = busy / (act / n_xcd * n_simd)
    return best


def map_wall_clock(S, N, dt):
    """Secondary metric (BASELINE.json "MAP wall-clock"): one
    coord_descent(maxiter=1) sweep of standard_glm on the same spike matrix = all N per-neuron
    BFGS fits (<= 225 iterations each, coord_descent.py:161-204) advanced in lock-step with the
    optimizer state on the GPU; excludes data generation / upload."""
    import copy
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.inference import coord_descent as cd
    popn = Population(make_model('standard_glm', N=N, dt=dt))
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': S.shape[0] * dt, 'stim': None, 'dt_stim': 0.1})
    x0 = popn.sample(np.random.RandomState(0))
    lp0 = popn.compute_log_p(x0)
    walls = []
    assert cd.resolve_batched(popn, None) == 'torch'
    for rep in range(3):        # the first sweep also pays the feature-tile build and torch's lazy rocBLAS / kernel loading
        t0 = time.perf_counter()
        x = cd.coord_descent(popn, x0=copy.deepcopy(x0), maxiter=1)      # default path (GPU lock-step optimizer)
        walls.append(time.perf_counter() - t0)
    lp1 = popn.compute_log_p(x)
    stats = getattr(popn, 'last_fit_stats', None) or {}
    popn.release_data()
    return {"metric": "MAP wall-clock, coord_descent(maxiter=1), standard_glm", "value": min(walls[1:]),
            "first_call_s": walls[0], "first_over_steady": walls[0] / min(walls[1:]), "sweeps_s": walls,
            "path": "coord_descent default (batched=None -> GPU lock-step optimizer)",
            "unit": "s", "log_p_initial": lp0, "log_p_final": lp1,
            "bfgs_iterations": getattr(popn, 'last_fit_stats', {}).get('iterations'),
            "ll_grad_evaluations": getattr(popn, 'last_fit_stats', {}).get('evaluations'),
            "neuron_evaluations": getattr(popn, 'last_fit_stats', {}).get('neuron_evaluations'),
            "neurons_converged_gtol": getattr(popn, 'last_fit_stats', {}).get('converged_gtol'),
            "neurons_stalled": getattr(popn, 'last_fit_stats', {}).get('stalled'),
            "neurons_at_maxiter": getattr(popn, 'last_fit_stats', {}).get('maxiter'),
            "line_search_steps": stats.get('line_search_steps'), "neuron_iterations": stats.get('neuron_iterations'),
            "optimizer": "lock-step batched BFGS = scipy's algorithm for every neuron at once (H0 = I, More'-Thuente "
                         "strong-Wolfe search with scipy's constants and first trial step; one fused ll+grad launch per pending "
                         "trial step of the listed neurons; bookkeeping: %s, inverse Hessians %s; active set read back %s "
                         "launch(es) late: no host sync per launch), "
                         "initial inverse-Hessian scaling %s, maxiter 225, gtol 1e-5, GPU-resident state on one stream"
                         % (stats.get('bookkeeping', 'n/a'),
                            {'implicit': "implicit (the history of update vectors applied to the gradient, 4 k P numbers per "
                                         "product after k updates)",
                             'dense': "dense (one read-modify-write pass of 2 P^2 numbers per accepted iteration)"}
                            .get(stats.get('inverse_hessian'), 'n/a'), stats.get('lag', 'n/a'),
                            's.y/y.y' if stats.get('init_scaling') else 'none (identity)')}


def map_wall_clock_sharded(S, N, dt, device, rank, world):
    """The secondary metric on N > 1 ranks: the same coord_descent(maxiter=1) sweep with every evaluation time-sharded
    (each rank its own bins of all neurons, one all-reduce of the packed (ll, grad) block per trial step:
    inference/parallel_coord_descent.py shard='time').  Called on EVERY rank; rank 0 reports."""
    import copy
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.inference.parallel_coord_descent import parallel_coord_descent, parallel_compute_log_p
    popn = Population(make_model('standard_glm', N=N, dt=dt), device=device)
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': S.shape[0] * dt, 'stim': None, 'dt_stim': 0.1})
    x0 = popn.sample(np.random.RandomState(0))                  # same seed on every rank
    walls = []
    for rep in range(3):
        t0 = time.perf_counter()
        x = parallel_coord_descent(popn, x0=copy.deepcopy(x0), maxiter=1, shard='time')
        walls.append(time.perf_counter() - t0)
    popn.set_time_shard(rank, world)
    lp1, _ = parallel_compute_log_p(popn, x, shard='time')
    popn.set_time_shard(None)
    stats = getattr(popn, 'last_fit_stats', None) or {}
    popn.release_data()
    return {"metric": "MAP wall-clock, coord_descent(maxiter=1), standard_glm, time-sharded over %d ranks" % world,
            "value": min(walls[1:]), "first_call_s": walls[0], "sweeps_s": walls, "unit": "s", "log_p_final": lp1,
            "ll_grad_evaluations": stats.get('evaluations'), "bfgs_iterations": stats.get('iterations'),
            "neurons_converged_gtol": stats.get('converged_gtol'),
            "collective": "one all-reduce of the packed (ll, grad) block of the listed neurons per trial step"}


def narrow_shard_steps(dev, theta, d_Weff, N, P, steps=30):
    """The step of north star's own split at 8 ranks on THIS GPU: ll+grad of a 16-neuron shard against the whole feature row
    (one post tile: k_fused8), default f64 resident blocks and -- a labelled opt-in, never the headline -- the same blocks
    stored as f32 (PGL_OPT_FEATURE_F32 = 2: all arithmetic f64, only the stored feature rounded)."""
    import torch
    from theano_pyglm_amd import _lib
    a, b = 32, 48
    d_th = torch.from_numpy(np.ascontiguousarray(theta[a:b])).cuda()
    d_o = torch.zeros((b - a) * (1 + P), dtype=torch.float64, device='cuda')
    out = {}
    ref = None
    for name, opt in (("f64_blocks", 0), ("f32_blocks_opt_in", 2)):
        dev.set_option(_lib.OPT_FEATURE_F32, opt)
        for _ in range(3):
            dev.ll_grad_dev(d_th.data_ptr(), d_Weff.data_ptr(), d_o.data_ptr(), d_o[b - a:].data_ptr(), a, b)
        torch.cuda.synchronize()
        dev.timing_summary(reset=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            dev.ll_grad_dev(d_th.data_ptr(), d_Weff.data_ptr(), d_o.data_ptr(), d_o[b - a:].data_ptr(), a, b)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / steps * 1e3
        _, k_ms, _ = dev.timing_summary(reset=True)
        res = d_o.cpu().numpy().copy()
        info = dev.info(a, b)
        out[name] = {"ms_per_step": wall, "kernel_ms": k_ms, "resident_feature_gb": info['resident_feature_bytes'] / 1e9}
        if ref is None:
            ref = res
        else:
            out[name]["max_rel_dev_from_f64_blocks"] = {
                "ll": float(np.max(np.abs(res[:b - a] - ref[:b - a]) / np.abs(ref[:b - a]))),
                "grad": float(np.max(np.abs(res[b - a:] - ref[b - a:])) / np.max(np.abs(ref[b - a:])))}
    dev.set_option(_lib.OPT_FEATURE_F32, 0)
    out["shard"] = "neurons %d..%d of %d on the whole recording" % (a, b - 1, N)
    return out


def mcmc_inner_ll(S, N, dt):
    """Secondary metric for the MCMC configuration ("inner-ll batches/s, one batch = the 11 ll
    values -- 10 Gauss-Hermite nodes + w = 0 -- of one (n_pre, n_post) pair", gibbs.py:1002-1032) on the same
    spike matrix with sparse_weighted_model (Dirichlet impulses, Erdos-Renyi graph), and the wall-clock of one
    collapsed-Gibbs sweep over all N^2 pairs (gibbs.py:1229-1250 for every column)."""
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.inference import gibbs as G
    model = make_model('sparse_weighted_model', N=N, dt=dt)
    stabilize_sparsity(model)
    popn = Population(model)
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': S.shape[0] * dt, 'stim': None, 'dt_stim': 0.1})
    x = popn.sample(np.random.RandomState(4))
    # a raw prior draw W ~ N(0, 1) times the tall normalised impulses drives quadrature nodes to lam = 0
    # (the reference's "log_G not finie"); shrink the weights like harness/synth_mcmc.py does
    x['net']['weights']['W'] = 0.2 * np.asarray(x['net']['weights']['W'])
    upd = G.CollapsedGibbsNetworkColumnUpdate(rng=np.random.RandomState(2))
    upd.preprocess(popn)
    h = popn._handle(popn._current)
    A = np.asarray(x['net']['graph']['A']).reshape(N, N)
    W = np.asarray(x['net']['weights']['W'], dtype=float).reshape(N, N)
    h.gibbs_prepare_all(popn.theta_matrix(x), A * W)
    cols = np.arange(N)
    pre = (cols * 37 + 11) % N
    nodes = np.concatenate((np.sqrt(2) * upd.sigma_w * upd.GAUSS_HERMITE_ABSCISSAE + upd.mu_w, [0.0]))
    ws = np.tile(nodes, (N, 1))
    aw = (A * W)[pre, cols]
    h.gibbs_ll_cols(cols, pre, aw, ws)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        ll = h.gibbs_ll_cols(cols, pre, aw, ws)
    per_launch = (time.perf_counter() - t0) / reps
    # the launch shape of a sweep step: the pair (j -> n) of every n -- one presynaptic neuron for all columns
    pre1 = np.full(N, 11)
    aw1 = (A * W)[pre1, cols]
    h.gibbs_ll_cols(cols, pre1, aw1, ws)
    t0 = time.perf_counter()
    for _ in range(reps):
        h.gibbs_ll_cols(cols, pre1, aw1, ws)
    per_launch_step = (time.perf_counter() - t0) / reps
    sweeps = []
    for _ in range(2):
        upd.n_ars_evals = 0
        t0 = time.perf_counter()
        upd.update_all(x)
        sweeps.append(time.perf_counter() - t0)
    popn.release_data()
    return {"metric": "MCMC inner-ll batches/s (11 ll values per (n_pre, n_post) pair, sparse_weighted_model)",
            "value": N / per_launch, "unit": "batches/s", "pairs_per_launch": N, "ms_per_launch": per_launch * 1e3,
            "sweep_step": {"ms_per_launch": per_launch_step * 1e3, "batches_per_s": N / per_launch_step,
                           "note": "all columns share the presynaptic neuron (what update_all launches): pair currents "
                                   "from its filtered spike train instead of the event windows"},
            "finite_fraction": float(np.isfinite(ll).mean()),
            "sweep_s": sweeps[1], "first_sweep_s": sweeps[0], "pairs_per_sweep": N * N,
            "ars_launches_last_sweep": upd.n_ars_evals,
            "kernels": "k_gibbs_rate_cols (max(x,0) in f64 + log1p(exp(-|x|)) in f32 where |x| >= 12, compacted f64 band "
                       "through a one-step table) + "
                       "k_gibbs_spike_cols"}


def st_ibasis(key, R=300, dt=0.001):
    """spatiotemporal_glm bases (B=3, unit area): the committed 100-point tables interpolated to R taps, / dt_max
    (impulse.py:92-112 / bkgd.py:274-301 with norm)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'basis_golden.npz'))
    basis = g[key]
    L, B = basis.shape
    ib = np.zeros((R, B))
    for b in range(B):
        ib[:, b] = np.interp(np.linspace(0, 1, R), np.linspace(0, 1, L), basis[:, b])
    return ib / (R * dt)


def stim_stress(reps=20, with_map=True):
    """Secondary block for BASELINE config 5 ("stimulus-conv kernel stressed"): SURVEY 8(d)'s stress variant --
    spatiotemporal_glm N=64, T=300 s, D_stim=1024 pixels, identity spatial basis, Bt=3, frames of 100 bins -- on the
    separable device path (frame-rate stimulus kernels + impulse columns on resident tiles), ll+grad per evaluation,
    with the tap-rate kernels of the same handle beside it."""
    import torch
    from theano_pyglm_amd import _lib
    N, T, D, Bt, dt, dt_stim = 64, 300.0, 1024, 3, 0.001, 0.1
    nT = int(round(T / dt))
    rng = np.random.default_rng(1234 + 5)
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    stim = rng.standard_normal((int(round(T / dt_stim)), D))
    ib = st_ibasis('st_imp_basis')
    ibt = np.ascontiguousarray(np.load(os.path.join(ROOT, 'tests', 'golden', 'basis_golden.npz'))['lr2d_ibasis_t'])
    dev = _lib.DeviceGlm(N, nT, 3, 300, 'exp', dt, device=torch.cuda.current_device())
    dev.set_spikes(S)
    dev.set_basis(ib)
    dev.set_stimulus_separable(stim, dt_stim, ibt, None)
    P = dev.P
    theta = np.zeros((N, P))
    theta[:, 0] = 1.0 + 0.3 * rng.standard_normal(N)
    theta[:, 1:1 + Bt] = 0.3 * rng.standard_normal((N, Bt))
    theta[:, 1 + Bt:1 + Bt + D] = 0.05 * rng.standard_normal((N, D))
    theta[:, 1 + Bt + D:] = 0.02 * rng.standard_normal((N, N * 3))
    stream = torch.cuda.current_stream()
    dev.set_stream(stream.cuda_stream)
    d_theta = torch.from_numpy(theta).cuda()
    d_Weff = torch.ones((N, N), dtype=torch.float64, device='cuda')
    d_ll = torch.zeros(N, dtype=torch.float64, device='cuda')
    d_grad = torch.zeros((N, P), dtype=torch.float64, device='cuda')

    def timed(n):
        dev.set_option(_lib.OPT_TIMING, 0)
        for _ in range(3):
            dev.ll_grad_dev(d_theta.data_ptr(), d_Weff.data_ptr(), d_ll.data_ptr(), d_grad.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            dev.ll_grad_dev(d_theta.data_ptr(), d_Weff.data_ptr(), d_ll.data_ptr(), d_grad.data_ptr())
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    info = dev.info()
    ms = timed(reps)
    ll = d_ll.cpu().numpy().copy()
    dev.set_option(94, 2)                        # the tap-rate kernels (300 taps per bin) on the 3-phase path
    ms_tap = timed(5)
    ll_tap = d_ll.cpu().numpy().copy()
    dev.set_option(94, 0)
    dev.set_option(_lib.OPT_TIMING, 1)
    dev.close()
    # one MAP sweep of the same model and data through the host mirror (coord_descent default: STA warm start of the stimulus
    # weights on the device, then all 64 per-neuron BFGS fits in lock step -- HIP row kernels running scipy's algorithm,
    # neuron lists through the frame-rate stimulus kernels; the template's N(0, 0.001) impulse prior runs every fit into the
    # reference's maxiter = 225, exactly where a sequential scipy fit of the neuron stops)
    map_s = map_first = lp_init = lp_final = None
    map_stats = {}
    if not with_map:
        return _stim_record(locals())
    import copy
    from theano_pyglm_amd.models import templates
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.inference import coord_descent as cd
    tmpl = templates.spatiotemporal_glm()
    tmpl['bkgd']['D_stim'] = D
    tmpl['bkgd']['spatial_basis'] = {'type': 'identity', 'n_eye': D}
    popn = Population(make_model(tmpl, N=N, dt=dt))
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': T, 'stim': stim, 'dt_stim': dt_stim})
    x0 = popn.sample(np.random.RandomState(0))
    for g in x0['glms']:
        g['bkgd']['w_x'] = np.asarray(g['bkgd']['w_x']) * (0.4 / np.sqrt(D))
    lp_init = popn.compute_log_p(x0)
    t0 = time.perf_counter()
    cd.coord_descent(popn, x0=copy.deepcopy(x0), maxiter=1)
    map_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    xm = cd.coord_descent(popn, x0=copy.deepcopy(x0), maxiter=1)
    map_s = time.perf_counter() - t0
    map_stats = dict(getattr(popn, 'last_fit_stats', None) or {})
    map_stats.pop('per_neuron', None)
    lp_final = popn.compute_log_p(xm)
    popn.release_data()
    return _stim_record(locals())


def _stim_record(v):
    nT, N, Bt, D, ms, ms_tap, ll, ll_tap, info, stim, P = (v[k] for k in ('nT', 'N', 'Bt', 'D', 'ms', 'ms_tap', 'll', 'll_tap',
                                                                           'info', 'stim', 'P'))
    map_s, map_first, map_stats = v['map_s'], v['map_first'], v['map_stats']
    flops_imp = 4.0 * nT * (N * 3) * N
    return {"metric": "ll+grad evaluation, spatiotemporal_glm stress variant", "variant": "D_stim=1024 (32x32 pixels), "
            "identity spatial basis Bx=1024, Bt=3, dt_stim=0.1 s, N=64, T=300 s (nT=300000), exp nonlinearity",
            "value": ms, "unit": "ms per ll+grad (queued back to back, whole evaluation)", "evals_per_s": 1e3 / ms,
            "stim_path": int(info['stim_path']), "kernel_version": int(info['kernel_version']),
            "path": "k_gemm_kc (z = stim.w_x at the frame rate) + k_fused7<12,4,3> (impulse columns on resident tiles; the "
                    "stimulus current as five more k-steps of the forward contraction, its backward as eight more MFMAs "
                    "per tile on the residuals in registers) + k_sepf_finish_d + k_gemm_kc + k_finalize",
            "map_sweep": "coord_descent(maxiter=1) as the reference runs it: STA warm start, then all 64 BFGS fits in lock step",
            "tap_rate_kernels_ms": ms_tap,
            "max_rel_ll_diff_vs_tap_rate": float(np.max(np.abs(ll - ll_tap) / np.abs(ll_tap))),
            "impulse_contraction_flops": flops_imp,
            "impulse_contraction_frac_of_f64_mfma_peak": flops_imp / (ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS,
            "dense_equivalent_bytes": float(nT) * Bt * D * 8,
            "device_bytes_stimulus": 2.0 * stim.size * 8,
            "map_sweep_s": map_s, "map_first_call_s": map_first, "map_log_p_initial": v['lp_init'],
            "map_log_p_final": v['lp_final'], "map_launches": map_stats.get('evaluations'),
            "map_neurons_converged_gtol": map_stats.get('converged_gtol'), "map_neurons_at_maxiter": map_stats.get('maxiter'),
            "map_stats": map_stats,
            "map_path": "coord_descent(maxiter=1) default: pgl_sta warm start + lock-step BFGS (P = %d per neuron)" % P}


def usable_cores():
    """Host cores this process may actually use: the scheduler affinity mask capped by the cgroup CPU
    quota (a container that sees 256 logical CPUs may be limited to a few cores' worth of time)."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    quota = None
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:                         # cgroup v2: "<quota> <period>" | "max ..."
            q, per = f.read().split()[:2]
            if q != 'max':
                quota = float(q) / float(per)
    except Exception:
        try:
            with open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us') as f:
                q = float(f.read())
            with open('/sys/fs/cgroup/cpu/cpu.cfs_period_us') as f:
                per = float(f.read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    if quota is not None:
        n = max(1, min(n, int(np.ceil(quota))))
    return n, (os.cpu_count() or 1), quota


def cpu_baseline(S, ibasis, theta, Weff, dt, sample_bins):
    """CPU baselines of BASELINE.md section 3 on the host cores of this box, all on a bounded sample
    (the first `sample_bins` bins of the same spike matrix, all neurons; cost is linear in nT):
      B1  oracle/glm_oracle.c: the reference's per-neuron dataflow on materialised features (N passes
          over fS per evaluation), single thread = `value`; the same with OpenMP over neurons;
      B2  oracle/glm_blocked.c: all neurons in one time-tiled sweep over fS (F.W, rate epilogue and
          F^T r per tile; fS streamed once), OpenMP over time blocks on all cores -- the strong baseline;
      set_data: the copy of (fS, S) into the model's shared variables that the reference performs
          before EVERY evaluation (glm.py:99-110 via coord_descent.py:52-57), timed alone."""
    from oracle import c_oracle as CO
    nT, N = S.shape
    scale = nT / float(sample_bins)
    Ss = np.ascontiguousarray(S[:sample_bins])
    fS = CO.features(Ss, ibasis)
    t0 = time.time()
    CO.ll_grad(Ss, fS, theta, Weff, 'explinear', dt, 0, N, threads=1)
    per_eval_1 = (time.time() - t0) * scale
    cores, logical, quota = usable_cores()
    t0 = time.time()
    CO.ll_grad(Ss, fS, theta, Weff, 'explinear', dt, threads=cores)
    per_eval_m = (time.time() - t0) * scale
    CO.ll_grad_blocked(Ss[:20000], fS[:20000], theta, Weff, 'explinear', dt, threads=cores)   # thread pool warm-up
    t0 = time.time()
    CO.ll_grad_blocked(Ss, fS, theta, Weff, 'explinear', dt, threads=cores)
    per_eval_b2 = (time.time() - t0) * scale
    t0 = time.time()
    CO.ll_grad_blocked(Ss[:sample_bins // 8], fS[:sample_bins // 8], theta, Weff, 'explinear', dt, threads=1)
    per_eval_b2_1 = (time.time() - t0) * scale * 8
    copy_s = CO.set_data_copy_seconds(fS, Ss.astype(np.float64)) * scale
    return {
        "value": 1.0 / per_eval_1, "unit": "evals/s", "cores": 1, "kind": "port",
        "sample": "first %d of %d bins, all %d neurons, scaled linearly; B1 = C restatement of the "
                  "reference per-neuron dataflow on materialised fS (oracle/glm_oracle.c)"
                  % (sample_bins, nT, N),
        "host": {"logical_cpus": logical, "usable_cores": cores, "cgroup_cpu_quota": quota},
        "all_cores": {"value": 1.0 / per_eval_m, "cores": cores,
                      "sample": "B1, first %d bins, all neurons, OpenMP over neurons" % sample_bins},
        "b2_blocked": {"value": 1.0 / per_eval_b2, "cores": cores, "single_core_value": 1.0 / per_eval_b2_1,
                       "sample": "B2 = all neurons in one time-tiled sweep over fS, fused rate epilogue, "
                                 "OpenMP over time blocks (oracle/glm_blocked.c); first %d bins "
                                 "(single core: first %d)" % (sample_bins, sample_bins // 8)},
        "set_data_copy": {"seconds_per_eval": copy_s, "bytes_per_eval": float(nT) * N * (ibasis.shape[1] + 1) * 8,
                          "note": "the reference copies fS and S into Theano shared variables before every "
                                  "nlp / grad_nlp call (glm.py:99-110); one memcpy thread, scaled from the sample; "
                                  "not included in the figures above"},
    }


RENDEZVOUS_EXIT = 17          # a rank could not join the process group (port taken between probe and bind)


def self_launch(n, script=None, argv=None):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes (one per GPU, env
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), relay rank 0's record.  Runs before torch / HIP are imported: the
    parent never initialises a GPU, the children are plain Popen processes (no exec from a GPU process)."""
    if script is None:
        import __graft_entry__ as ge
        ge.build_hip()                              # once, here: the ranks find the library fresh
    return _self_launch_once(n, script, argv, attempts_left=2)


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def _self_launch_once(n, script, argv, attempts_left):
    import subprocess
    # (the port is free when probed; another process can take it before rank 0 binds it -- then the ranks fail at the
    #  rendezvous, before any work, and the launch is repeated once on a new port)
    port = _free_port()
    t_start = time.time()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        cmd = [sys.executable, script or os.path.abspath(__file__)] + (sys.argv[1:] if argv is None else argv)
        procs.append(subprocess.Popen(cmd, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # rank 0's stdout is drained by a thread; the parent watches the ranks: one that fails takes the others down (its
    # own children, by PID) instead of leaving them in a collective until the communicator times out
    import threading
    import time as _time
    chunks, killed = [], set()
    rd = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    while any(pr.poll() is None for pr in procs):
        if any(pr.poll() not in (None, 0) for pr in procs):
            _time.sleep(2.0)                        # (ranks that fail together, e.g. no GPU each, report their own codes)
            for i, pr in enumerate(procs):
                if pr.poll() is None:
                    pr.kill()
                    killed.add(i)
            break
        _time.sleep(0.2)
    codes = [pr.wait() for pr in procs]
    rd.join(timeout=10.0)
    out0 = ''.join(c or '' for c in chunks)
    lines = [ln for ln in out0.splitlines() if ln.strip()]
    rec = lines[-1:] if codes[0] == 0 else []       # a rank 0 that did not finish has no record
    for ln in lines[:len(lines) - len(rec)]:
        sys.stderr.write(ln + '\n')                 # anything rank 0 printed before its record (library banners)
    if rec:
        print(rec[0], flush=True)
    bad = [c for i, c in enumerate(codes) if c != 0 and i not in killed]      # the ranks that failed by themselves
    if bad or killed:
        ended = (" (ended by the parent: ranks %s)" % sorted(killed)) if killed else ""
        sys.stderr.write("bench.py: rank exit codes %s%s\n" % (codes, ended))
        if RENDEZVOUS_EXIT in bad and attempts_left > 1:
            sys.stderr.write("bench.py: rendezvous on port %d failed after %.0f s; launching again on a new port\n"
                             % (port, time.time() - t_start))
            return _self_launch_once(n, script, argv, attempts_left - 1)
        return 3 if 3 in bad else (bad[0] if bad else 1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--neurons', type=int, default=128)
    ap.add_argument('--seconds', type=float, default=600.0)
    ap.add_argument('--f32-features', type=int, default=0)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-map', action='store_true', help='skip the secondary MAP wall-clock measurement')
    ap.add_argument('--no-mcmc', action='store_true', help='skip the secondary MCMC inner-ll measurement')
    ap.add_argument('--no-stim', action='store_true', help='skip the secondary stimulus stress-variant measurement (config 5)')
    ap.add_argument('--no-stim-map', action='store_true',
                    help='skip the MAP sweep of the stress variant inside the stimulus block')
    ap.add_argument('--stim-map', action='store_true', help='(accepted for older scripts: the sweep is part of --full)')
    ap.add_argument('--no-ab', action='store_true',
                    help='skip the A/B loops after the timed region (in-kernel features, all-f64 epilogue): profiler '
                         'passes use it so that per-kernel averages and counters describe the headline kernel only')
    ap.add_argument('--full', action='store_true',
                    help='also run every measurement and check beyond the headline (see the module docstring)')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write the ll and gradient of the last timed step as DIR/<name>.npy (rank 0)')
    ap.add_argument('--shard', choices=['time', 'neurons'], default='time')
    # dev-only: exercise the N>1 code path on a 1-GPU box (all ranks on cuda:0, gloo collectives)
    ap.add_argument('--debug-single-device', action='store_true')
    ap.add_argument('--rccl-selftest', action='store_true',
                    help='dev: run the multi-rank code path (process group on nccl = RCCL, barrier, all-reduce of the packed '
                         '(ll, grad) block per step, per-rank gather) on ONE rank -- what a one-GPU box can execute of it')
    args = ap.parse_args()

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ and not args.rccl_selftest:
        sys.exit(self_launch(args.gpus))          # (nothing has touched torch or HIP in this process)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    multi = world > 1 or args.rccl_selftest       # the code path with a process group and collectives
    # Build (if stale) BEFORE torch or anything else touches the GPU: a compiler child must never be
    # spawned from a process that has initialised HIP, least of all under rocprofv3 (build_hip raises
    # when the library is stale under a profiler and scrubs the preload variables otherwise).
    import __graft_entry__ as ge
    if rank == 0:
        ge.build_hip()
        if args.full and not args.no_cpu_baseline and not multi:
            ge.build_oracle()

    import torch
    import torch.distributed as dist
    ndev = torch.cuda.device_count()         # (does not initialise the GPU)
    if not args.debug_single_device and (ndev < world or local_rank >= ndev):
        # fail loudly on every rank BEFORE any rendezvous: a missing GPU must not turn into a hung collective
        sys.stderr.write("bench.py: rank %d needs GPU %d of %d ranks but only %d device(s) are visible\n"
                         % (rank, local_rank, world, ndev))
        sys.exit(3)
    if world != args.gpus:
        if rank == 0:
            sys.stderr.write("warning: --gpus %d but WORLD_SIZE=%d; using WORLD_SIZE\n"
                             % (args.gpus, world))
    if args.debug_single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if multi:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29541')
        import datetime
        try:
            if args.debug_single_device:
                dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
            else:
                # device_id binds the communicator to this rank's GPU up front (no guessing from the global rank, eager init)
                dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local_rank),
                                        timeout=datetime.timedelta(seconds=600))
        except Exception as e:                    # port taken / store unreachable: the self-launcher retries on a new port
            sys.stderr.write("bench.py rank %d: rendezvous failed: %s\n" % (rank, e))
            sys.exit(RENDEZVOUS_EXIT)

    if multi:
        dist.barrier()                       # rank 0 has finished building
    from theano_pyglm_amd import _lib

    N, dt = args.neurons, 0.001
    S = make_workload(N, args.seconds, dt, seed=1234 + 3)
    nT = S.shape[0]
    ib = standard_ibasis()
    R, B = ib.shape
    P = 1 + N * B
    theta = make_theta(N, P)
    Weff = np.ones((N, N))

    from theano_pyglm_amd import parallel as PL
    dev = _lib.DeviceGlm(N, nT, B, R, 'explinear', dt, device=local_rank)
    dev.set_spikes(S)
    dev.set_basis(ib)
    if args.f32_features:
        dev.set_option(_lib.OPT_FEATURE_F32, 1)
    if args.shard == 'time' or not multi:
        n_lo, n_hi = 0, N
        t_lo, t_hi = PL.time_shard_bounds(nT, rank, world)
        dev.set_time_range(t_lo, t_hi)
    else:
        n_lo, n_hi = PL.shard_bounds(N, rank, world)
        t_lo, t_hi = 0, nT

    # A dedicated non-default stream is made current for everything below: torch's default stream
    # has handle 0 (the NULL stream), which pgl_set_stream cannot name -- kernels would silently run on
    # the handle's own stream, un-ordered with the RCCL collectives.
    bench_stream = torch.cuda.Stream()
    torch.cuda.set_stream(bench_stream)
    d_theta = torch.from_numpy(theta[n_lo:n_hi].copy()).cuda()
    d_Weff = torch.from_numpy(Weff).cuda()
    # one contiguous block [ll | grad] so that a single all-reduce moves both
    npost = n_hi - n_lo
    d_out = torch.zeros(npost * (1 + P), dtype=torch.float64, device='cuda')
    d_ll = d_out[:npost]
    d_grad = d_out[npost:].view(npost, P)
    pop_ll = [None]                       # --shard neurons: the gathered population ll of the last step
    torch.cuda.synchronize()

    # The library queues its kernels on torch's current stream -- the stream RCCL collectives are
    # ordered against -- so evaluation k, its all-reduce and evaluation k+1 serialise on the GPU
    # without a host synchronisation per step.  Every launch records its own HIP event set on
    # that stream; the mean kernel duration over the timed region is read back after the loop.
    assert torch.cuda.current_stream().cuda_stream == bench_stream.cuda_stream != 0
    dev.set_stream(bench_stream.cuda_stream)

    coll_events = []                      # (start, end) events around the collective of every 4th timed step (an event
    step_no = [0]                         # between two kernels costs ~6 us of GPU idle time: 2.5 % of a 1/8-recording step)

    def step(record):
        dev.ll_grad_dev(d_theta.data_ptr(), d_Weff.data_ptr(), d_ll.data_ptr(), d_grad.data_ptr(),
                        n_lo, n_hi)
        if record:
            record = step_no[0] % 4 == 0
            step_no[0] += 1
        if multi and record and not args.debug_single_device:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record(bench_stream)
        if multi:
            if args.debug_single_device:         # gloo: collectives on host copies
                dev.sync()
                if args.shard == 'time':
                    h = d_out.cpu()
                    dist.all_reduce(h)
                    d_out.copy_(h)
                else:
                    pop_ll[0] = PL.allgather_rows_t(d_ll, N)
            elif args.shard == 'time':
                dist.all_reduce(d_out)               # population (ll, grad) on every rank
            else:
                # population ll on every rank (1 KB): the product's padded all-gather (uneven shards, e.g. 100 neurons
                # on 8 ranks, are one all_gather_into_tensor of equal-sized pieces)
                pop_ll[0] = PL.allgather_rows_t(d_ll, N)
            if record and not args.debug_single_device:
                ev1 = torch.cuda.Event(enable_timing=True)
                ev1.record(bench_stream)
                coll_events.append((ev0, ev1))

    # HIP events around every TIMING_EVERY-th evaluation of the timed region (the kernel duration of `roofline` is their
    # mean): an event between two kernels costs ~6 us of GPU idle time, which is 4 % of a 1/8-recording step
    TIMING_EVERY = 4
    dev.set_option(_lib.OPT_TIMING, TIMING_EVERY)
    for _ in range(args.warmup):
        step(False)
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    dev.set_option(_lib.OPT_TIMING, TIMING_EVERY)    # (restarts the sampling phase: evaluation 0, 4, 8, ... of the region)
    dev.timing_summary(reset=True)                   # start the timing window of the timed region
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    local_elapsed = elapsed
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device='cpu' if args.debug_single_device else 'cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller, before any loop of --full reuses the buffers (time shards: the
        # all-reduced population; neuron shards: this rank's rows and the gathered population ll)
        outs = {'ll': d_ll.cpu().numpy(), 'grad': d_grad.cpu().numpy()}
        if pop_ll[0] is not None:
            outs['population_ll'] = pop_ll[0].cpu().numpy()
        dump_outputs(args.dump_outputs, outs)

    info = dev.info(n_lo, n_hi)
    n_timed, kern_ms, call_ms = dev.timing_summary(reset=True)
    dev.set_option(_lib.OPT_TIMING, 1)               # the short A/B loops below time every evaluation
    per_rank = None
    if multi:
        # what every rank paid per step: its own wall clock, its fused kernels, its whole evaluation (prep + fused +
        # finalize) and the collective (HIP events on the stream; includes waiting for the slowest rank)
        coll_ms = float(np.mean([a.elapsed_time(b) for a, b in coll_events])) if coll_events else None
        mine = {"rank": rank, "ms_per_step": 1e3 * local_elapsed / args.steps, "kernel_ms": kern_ms,
                "evaluation_ms": call_ms, "collective_ms": coll_ms, "bins": int(t_hi - t_lo), "neurons": int(n_hi - n_lo)}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    shard_neurons = None
    # ranks that exchanged over RCCL (backend nccl); a gloo run (--debug-single-device) reports 'ranks' only
    rccl_ranks = (dist.get_world_size() if dist.get_backend() == 'nccl' else 0) if multi else 1
    if args.full and multi and args.shard == 'time' and world > 1:
        # the split north_star names, measured behind the timed region: post-synaptic neurons block-partitioned
        # (parallel_coord_descent.py:137-147), every rank on the whole recording, all-gather of the ll shards per step
        a, b = PL.shard_bounds(N, rank, world)
        dev.set_time_range(0, nT)
        dn_theta = torch.from_numpy(theta[a:b].copy()).cuda()
        dn_ll = torch.zeros(b - a, dtype=torch.float64, device='cuda')
        dn_grad = torch.zeros((b - a, P), dtype=torch.float64, device='cuda')
        gat = [None]

        def nstep():
            dev.ll_grad_dev(dn_theta.data_ptr(), d_Weff.data_ptr(), dn_ll.data_ptr(), dn_grad.data_ptr(), a, b)
            if args.debug_single_device:
                dev.sync()
            gat[0] = PL.allgather_rows_t(dn_ll, N)   # padded: valid for uneven shards on nccl and gloo alike
        nsteps = max(1, min(args.steps, 20))
        for _ in range(2):
            nstep()
        dist.barrier()
        torch.cuda.synchronize()
        dev.timing_summary(reset=True)
        tn0 = time.perf_counter()
        for _ in range(nsteps):
            nstep()
        dist.barrier()
        torch.cuda.synchronize()
        tn = time.perf_counter() - tn0
        _, nk_ms, nc_ms = dev.timing_summary(reset=True)
        tt = torch.tensor([tn], dtype=torch.float64, device='cpu' if args.debug_single_device else 'cuda')
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        mine_n = {"rank": rank, "ms_per_step": 1e3 * tn / nsteps, "kernel_ms": nk_ms, "evaluation_ms": nc_ms,
                  "neurons": int(b - a), "bins": int(nT), "kernel_version": int(dev.info(a, b)['kernel_version'])}
        per_rank_n = [None] * world
        dist.all_gather_object(per_rank_n, mine_n)
        ll_gathered = gat[0].cpu().numpy()
        shard_neurons = {"ms_per_step": 1e3 * float(tt.item()) / nsteps, "steps": nsteps,
                         "evals_per_s": nsteps / float(tt.item()), "collective": "all-gather of the per-neuron ll (%d B)" % (8 * N),
                         "per_rank": per_rank_n, "_ll": ll_gathered}
        t_lo, t_hi = PL.time_shard_bounds(nT, rank, world)
        dev.set_time_range(t_lo, t_hi)
    alt = None
    if args.full and not multi and not args.f32_features and info['kernel_version'] == 5 and not args.no_ab:
        # the same evaluation with the features regenerated from the spike events inside the kernel
        # (the north star's fused filter kernel, PGL_OPT_KERNEL=3) -- reported beside the headline
        dev.set_option(_lib.OPT_KERNEL, 3)
        for _ in range(3):
            step(False)
        torch.cuda.synchronize()
        dev.timing_summary(reset=True)
        for _ in range(10):
            step(False)
        torch.cuda.synchronize()
        _, alt_ms, _ = dev.timing_summary(reset=True)
        alt_v = int(dev.info(n_lo, n_hi)['kernel_version'])
        alt = {"kernel": ("k_fused3 pass 1 + pass 2" if alt_v == 4 else "k_fused2 (K split over the waves of a post tile)") +
                         ", features generated in-kernel from the spike events",
               "kernel_ms": alt_ms, "achieved": info['flops'] / (alt_ms * 1e-3) / 1e12,
               "frac": info['flops'] / (alt_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS}
        dev.set_option(_lib.OPT_KERNEL, 0)
    allf64 = None
    if args.full and not multi and not args.f32_features and not args.no_ab:
        # the same evaluation with the all-f64 rate epilogue (PGL_OPT_EPI_F64: no single-precision exp(-x)
        # correction), so that the effect of that term is visible beside every headline number
        dev.set_option(_lib.OPT_EPI_F64, 1)
        for _ in range(3):
            step(False)
        torch.cuda.synchronize()
        dev.timing_summary(reset=True)
        for _ in range(10):
            step(False)
        torch.cuda.synchronize()
        _, f64_ms, _ = dev.timing_summary(reset=True)
        ll_f64 = d_ll.cpu().numpy().copy()
        dev.set_option(_lib.OPT_EPI_F64, 0)
        step(False)
        torch.cuda.synchronize()
        dev.timing_summary(reset=True)
        ll_def = d_ll.cpu().numpy()
        allf64 = {"kernel_ms": f64_ms, "achieved": info['flops'] / (f64_ms * 1e-3) / 1e12,
                  "frac": info['flops'] / (f64_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS,
                  "max_rel_ll_diff_vs_default": float(np.max(np.abs(ll_f64 - ll_def) / np.abs(ll_f64)))}
    assert n_timed == min((args.steps + TIMING_EVERY - 1) // TIMING_EVERY, 256), "timing window does not cover the timed steps" 
    achieved = info['flops'] / (kern_ms * 1e-3) / 1e12
    ll_host = d_ll.cpu().numpy()
    assert np.all(np.isfinite(ll_host)), "non-finite ll"
    if args.full and multi:
        # the sharded evaluation must equal the single-rank evaluation of the whole recording
        if args.shard == 'time':
            ll_pop = ll_host                                   # all-reduced: full ll of all N neurons
        else:
            ll_pop = pop_ll[0].cpu().numpy()
        if rank == 0:
            dev.set_time_range(0, nT)
            ll_ref, _ = dev.ll_grad(theta, Weff, 0, N, want_grad=False)
            assert np.allclose(ll_pop, ll_ref, rtol=1e-10, atol=0), \
                "sharded population ll differs from the single-rank evaluation"
            if shard_neurons is not None:
                assert np.allclose(shard_neurons.pop('_ll'), ll_ref, rtol=1e-10, atol=0), \
                    "neuron-sharded population ll differs from the single-rank evaluation"

    # N > 1: the MAP sweep under the same (time) sharding, on every rank, behind the timed region
    map_sharded = None
    if args.full and multi and world > 1 and args.shard == 'time' and not args.no_map:
        dev.set_stream(None)
        try:
            map_sharded = map_wall_clock_sharded(S, N, dt, local_rank, rank, world)
        except Exception as e:                         # (diagnostic run: report, do not lose the headline)
            map_sharded = {"error": "%s: %s" % (type(e).__name__, e)}
        dev.set_stream(bench_stream.cuda_stream)
    narrow = None
    if args.full and not multi and N == 128 and not args.f32_features and not args.no_ab:
        narrow = narrow_shard_steps(dev, theta, d_Weff, N, P)
    if rank == 0:
        out = {
            "metric": "population ll+grad evals/sec (N neurons x T bins)",
            "value": args.steps / elapsed,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": "standard_glm N=%d T=%gs dt=1ms (nT=%d), B=%d R=%d, explinear, "
                            "Poisson 20 Hz spikes, ll+grad of all N neurons per step"
                            % (N, args.seconds, nT, B, R),
                "sharding": ("time bins split over %d rank(s), all neurons per rank, S replicated, "
                             "all-reduce of the packed (ll, grad) block per step" % world)
                if (args.shard == 'time' or not multi) else
                            ("post-synaptic neurons block-partitioned over %d rank(s); S replicated; "
                             "all-gather of ll per step" % world),
                "feature_staging": "f32" if args.f32_features else "f64",
                "rate_epilogue": ("f64; in waves whose 256 currents are all > 12 the exp(-x) < 6.2e-6 inside "
                                  "softplus = x + log1p(exp(-x)) and sigmoid = 1/(1 + exp(-x)) comes from v_exp_f32: "
                                  "rate and residual within 5e-13 relative of the all-f64 epilogue (-DPGL_EPI_F32=0), "
                                  "parity tests unchanged at 1e-10 / 1e-9 against the oracle"),
                "features": ("resident f64 tiles built once per data set (the reference's data['fS'], "
                             "impulse.py:114-130): %.2f GB in HBM, streamed by LDS-DMA"
                             % (info['resident_feature_bytes'] / 1e9))
                if info['kernel_version'] == 5 else "regenerated from the spike events in every evaluation",
                "spike_events": int(info['events']),
            },
            "roofline": {
                "bound": "mfma",
                "kernel": "k_fused5 pass 1 + pass 2 on resident feature tiles (rank 0 shard: %d neurons x %d bins)"
                          % (n_hi - n_lo, t_hi - t_lo),
                "achieved": achieved,
                "peak": F64_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s",
                "frac": achieved / F64_MFMA_PEAK_TFLOPS,
                "traffic": None,
                "kernel_ms": kern_ms,
                "kernel_ms_source": "mean of HIP-event spans around the fused kernels of every %d-th evaluation of the "
                                    "timed region (%d samples), on the stream they are launched on; a sample mean: "
                                    "kernel_ms + prep + finalize may exceed ms_per_step (all steps) by the sampling "
                                    "noise of a few per cent" % (TIMING_EVERY, n_timed),
                "algorithmic_flops_per_launch": info['flops'],
                "algorithmic_bytes_per_launch": info['bytes'],
                "streamed_bytes_per_launch": info['streamed_bytes'],
            },
        }
        if alt is not None:
            out["roofline"]["alt_in_kernel_features"] = alt
        if allf64 is not None:
            out["roofline"]["all_f64_epilogue"] = allf64
        if per_rank is not None:
            out["per_rank"] = per_rank
            out["ranks"] = dist.get_world_size()
            out["rccl_ranks"] = rccl_ranks
            out["collective_backend"] = dist.get_backend()
        if shard_neurons is not None:
            out["sharding_neurons"] = shard_neurons
        if args.full and not multi and N == 128 and nT == 600000 and not args.f32_features:
            tr = pmc_traffic(['void k_fused5<18, 22, 1', 'void k_fused5<18, 22, 2'])
            if tr is not None:
                out["roofline"]["traffic"] = tr[1]
                out["roofline"]["traffic_source"] = os.path.relpath(tr[0], ROOT)
            mb = pmc_mfma_busy(['void k_fused5<18, 22, 1', 'void k_fused5<18, 22, 2'])
            if mb is not None:
                out["roofline"]["mfma_busy_pmc"] = mb
        if args.full and not multi and not args.no_map and not args.f32_features:
            out["secondary"] = map_wall_clock(S, N, dt)
        if map_sharded is not None:
            out["secondary"] = map_sharded
        if narrow is not None:
            out["secondary_narrow_shard"] = narrow
        if args.full and not multi and not args.no_mcmc and not args.f32_features:
            out["secondary_mcmc"] = mcmc_inner_ll(S, N, dt)
        if args.full and not multi and not args.no_stim and not args.f32_features:
            out["secondary_stim"] = stim_stress(with_map=not args.no_stim_map)
        if args.full and not multi and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(S, ib, theta, Weff, dt, sample_bins=min(nT, 300000))
        # RCCL prints a banner through C stdio: flush it first so that the JSON line is the last line of stdout
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    dev.close()
    if multi:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
