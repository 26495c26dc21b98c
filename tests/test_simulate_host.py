"""Host side of the batched simulation: pgl_simulate_streams (the reference of the device path) against a pure-numpy
restatement written here -- the stream formula of include/pyglm_hip.h in uint64 arithmetic and the per-bin loop -- plus the
properties of the streams, the ring planner and the decision margin of every case the GPU tests run.

The cases live here (CASES / case()); tests/test_gpu_simulate.py imports them, so the seeds whose margin is asserted below
are the seeds the device is compared on."""
import functools

import numpy as np
import pytest

from theano_pyglm_amd import _lib

G = np.uint64(0x9e3779b97f4a7c15)
DT = 0.001


# ---- the stream rule, restated ------------------------------------------------------------------------------------------
def _mix(z):
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64))      # (arrays: uint64 array arithmetic wraps silently)


def stream_keys(seed, rep, N):
    z = _mix(_u64(seed) + G)
    z = _mix(z + G * (_u64(rep) + np.uint64(1)))
    return _mix(z + G * (np.arange(N, dtype=np.uint64) + np.uint64(1)))


def uniforms(keys, k):
    z = _mix(_u64(keys) + G * (_u64(k) + np.uint64(1)))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def f_nlin(x, nlin):
    return np.exp(x) if nlin == 'exp' else np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def restate(X0, AW, nlin, dt, rep, seed):
    """pgl_simulate's loop on the per-neuron streams: (S, X, exceptions, thresholds drawn per neuron)."""
    X = np.array(X0, dtype=np.float64)
    nT, N = X.shape
    R = AW.shape[1]
    keys = stream_keys(seed, rep, N)
    k = np.zeros(N, dtype=np.uint64)
    thr = -np.log(uniforms(keys, k))
    k += np.uint64(1)
    drawn = [[v] for v in thr]
    S = np.zeros((nT, N), dtype=np.uint8)
    acc = np.zeros(N)
    exc = 0
    for t in range(nT):
        acc = acc + f_nlin(X[t], nlin) * dt
        spk = acc > thr
        S[t, spk] += 1
        t_imp = min(nT - t - 1, R)
        while spk.any():
            if np.any(S[t] >= 10):
                exc += 1
                break
            for n_pre in np.flatnonzero(spk):
                X[t + 1:t + 1 + t_imp] += AW[n_pre, :t_imp, :]
            acc[spk] -= thr[spk]
            acc[acc < 0] = 0
            thr[spk] = -np.log(uniforms(keys[spk], k[spk]))
            k[spk] += np.uint64(1)
            for n in np.flatnonzero(spk):
                drawn[n].append(thr[n])
            spk = acc > thr
            S[t, spk] += 1
    return S, X, exc, drawn


# ---- the cases (shared with the GPU tests) ------------------------------------------------------------------------------
#        name            N    R    nT   nlin         seed  reps
CASES = {'small_exp':   (3,   7,   400, 'exp',        11,  5),
         'small_expl':  (3,   7,   400, 'explinear',  12,  5),
         'n70':         (70,  33,  2000, 'explinear', 13,  2),     # more neurons than a wave, no multiple of anything; LDS
         'n130':        (130, 200, 1500, 'explinear', 14,  2),     # global ring by size
         'high_rate':   (3,   7,   400, 'exp',        15,  2),     # multi-spike rounds and cap exceptions
         'tail':        (3,   7,   400, 'explinear',  16,  1),     # a spike inside the last R bins
         # the sweep: full waves inside one series of pgl_lambda_only (REGIME), launch shapes (PLAN), edges of the time loop
         'n64_tail':    (64,  16,  300, 'explinear',  21,  1),
         'n64_mid':     (64,  16,  300, 'explinear',  22,  1),
         'n64_neg_mid': (64,  16,  300, 'explinear',  23,  1),
         'n128_mixed_waves': (128, 16, 300, 'explinear', 24, 1),
         'n65':         (65,  9,   300, 'explinear',  25,  1),     # one neuron in a second wave
         'n1':          (1,   5,   400, 'explinear',  26,  2),
         'lds_96k':     (96,  128, 300, 'explinear',  27,  1),     # 98304 B of LDS: above the 64 KiB a kernel gets unasked
         'lds_1024thr': (96,  200, 300, 'explinear',  28,  1),     # 153600 B of LDS, R N > 16384: 1024 threads
         'n300':        (300, 8,   200, 'explinear',  29,  1),     # N > 256: 1024 threads, five waves with neurons
         'n1024':       (1024, 2,  60,  'explinear',  30,  1),     # every thread owns a neuron, all 16 ballot masks
         'nt_lt_r':     (3,   7,   5,   'explinear',  31,  2),     # the recording is shorter than the ring
         'nt1':         (3,   7,   1,   'explinear',  32,  2),
         'r1':          (5,   1,   300, 'explinear',  33,  2)}
SMALL = ('small_exp', 'small_expl', 'high_rate', 'tail')
# currents of the regime cases: X0 uniform in [lo, hi] per wave of 64 neurons, coupling |AW| <= w, bin width dt.  The vote of
# pgl_lambda_only: e^-|x| < e^-9.25 in every lane -> the tail series, < 0.1 (|x| > 2.3) -> the atanh series, else general;
# a wave without a neuron-less lane (N a multiple of 64) takes a series only if the total currents X of all its neurons agree.
#                 name: ([(lo, hi) per wave], w, dt, (min X, max X) asserted per wave: 0.5 clear of the vote thresholds)
REGIME = {'n64_tail':    ([(11.0, 30.0)], 0.02, 0.001, [(9.75, 600.0)]),
          'n64_mid':     ([(3.4, 8.1)], 0.01, 0.005, [(2.8, 8.75)]),
          'n64_neg_mid': ([(-8.1, -3.4)], 0.01, 2.0, [(-8.75, -2.8)]),
          'n128_mixed_waves': ([(11.0, 30.0), (3.4, 8.1)], 0.01, 0.002, [(9.75, 600.0), (2.8, 8.75)])}
# the launch forms: name -> {flags: (ring in LDS, threads)}; threads = 256 if N <= 256 and R N <= 16384 else 1024
# (pgl_simulate_batch_dev), the ring in LDS up to PGL_SIM_LDS_MAX bytes unless flag bit 0 is set
LDS_MAX = 160 * 1024 - 1024
PLAN = {'n64_tail': {0: (True, 256), 1: (False, 256)}, 'n64_mid': {0: (True, 256)}, 'n64_neg_mid': {0: (True, 256)},
        'n128_mixed_waves': {0: (True, 256)}, 'n65': {0: (True, 256)}, 'n1': {0: (True, 256), 1: (False, 256)},
        'lds_96k': {0: (True, 256), 1: (False, 256)}, 'lds_1024thr': {0: (True, 1024), 1: (False, 1024)},
        'n300': {0: (True, 1024), 1: (False, 1024)}, 'n1024': {0: (True, 1024), 1: (False, 1024)},
        'nt_lt_r': {0: (True, 256), 1: (False, 256)}, 'nt1': {0: (True, 256), 1: (False, 256)},
        'r1': {0: (True, 256), 1: (False, 256)}}


def case_dt(name):
    return REGIME[name][2] if name in REGIME else DT


@functools.lru_cache(maxsize=None)
def case(name):
    """(X0 (nT, N), AW (N, R, N), nlin, seed) of a case; about 40 Hz per neuron at dt = 1 ms, signed coupling that decays
    over the R taps.  The REGIME cases: currents inside one series per wave, weak coupling."""
    N, R, nT, nlin, seed, _ = CASES[name]
    rng = np.random.RandomState(1000 + seed)
    if name in REGIME:
        waves, w, _, _ = REGIME[name]
        lo = np.repeat([a for a, _ in waves], 64)[None, :]
        hi = np.repeat([b for _, b in waves], 64)[None, :]
        X0 = lo + (hi - lo) * rng.rand(nT, N)
        AW = w * (2.0 * rng.rand(N, R, N) - 1.0) * np.exp(-np.arange(R) / (0.3 * R))[None, :, None]
        X0.setflags(write=False)
        AW.setflags(write=False)
        return X0, AW, nlin, seed
    rate = 40.0
    base = np.log(rate) if nlin == 'exp' else rate
    X0 = base + (0.3 if nlin == 'exp' else 10.0) * rng.randn(nT, N)
    W = rng.randn(N, N) * ((0.4 if nlin == 'exp' else 8.0) / np.sqrt(N))
    imp = np.exp(-np.arange(R) / (0.3 * R))[None, :, None] * (1.0 + 0.2 * rng.rand(N, R, N))
    AW = W[:, None, :] * imp
    if name == 'high_rate':
        X0 += np.log(25.0)                                   # ~1 spike per bin and neuron: multi-spike rounds
        X0[50::40] = np.log(14.0 / DT)                       # rate * dt = 14 in ten bins: more than the cap of 10 holds
        AW *= 0.1
    if name == 'tail':
        X0[-3:] = 3000.0                                     # rate * dt = 3 in the last three bins (R = 7)
    if name in ('nt_lt_r', 'nt1'):
        X0 += 1500.0                                         # rate * dt = 1.5: spikes in every bin
    X0.setflags(write=False)
    AW.setflags(write=False)
    return X0, AW, nlin, seed


@functools.lru_cache(maxsize=None)
def host_reference(name, rep):
    """(S, X, exceptions, closest_call) of pgl_simulate_streams; computed once, shared, read-only."""
    X0, AW, nlin, seed = case(name)
    S, X, exc, closest = _lib.simulate_streams(X0, AW, nlin, case_dt(name), rep=rep, seed=seed)
    S.setflags(write=False)
    X.setflags(write=False)
    return S, X, exc, closest


# ---- tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SMALL)
def test_streams_reference_equals_numpy_restatement(name):
    X0, AW, nlin, seed = case(name)
    for rep in (0, 3):
        S, X, exc, _ = _lib.simulate_streams(X0, AW, nlin, DT, rep=rep, seed=seed)
        S0, X1, exc0, _ = restate(X0, AW, nlin, DT, rep, seed)
        assert S.dtype == np.uint8 and np.array_equal(S, S0)
        assert exc == exc0
        assert np.allclose(X, X1, rtol=1e-13, atol=0.0)
    assert S.sum() > 0


def test_cases_reach_what_they_are_for():
    S, _, exc, _ = host_reference('high_rate', 0)
    assert exc >= 1 and S.max() == 10 and np.sum(S >= 2) > 20          # cap exceptions and multi-spike rounds
    S, _, exc, _ = host_reference('small_exp', 0)
    assert exc == 0 and S.sum() > 10
    R = CASES['tail'][1]
    S, X, _, _ = host_reference('tail', 0)
    assert S[-R:-1].sum() > 0                                          # a spike whose impulse the end truncates
    # replicates differ, and the seed matters
    assert not np.array_equal(host_reference('small_expl', 0)[0], host_reference('small_expl', 1)[0])
    X0, AW, nlin, seed = case('small_expl')
    assert not np.array_equal(_lib.simulate_streams(X0, AW, nlin, DT, rep=0, seed=seed + 1)[0], host_reference('small_expl', 0)[0])



def test_regime_cases_stay_inside_their_series_and_spike():
    """Every total current X of the host reference (X0 plus what the spikes added) lies inside the case's regime, per wave of
    64 neurons, at least 0.5 from the vote thresholds 9.25 and 2.3 of pgl_lambda_only -- and the case spikes."""
    for name, (waves, w, dt, want) in REGIME.items():
        N = CASES[name][0]
        assert N == 64 * len(waves)                                    # no lane without a neuron: the vote is the neurons'
        for rep in range(CASES[name][5]):
            S, X, exc, _ = host_reference(name, rep)
            for i, (lo, hi) in enumerate(want):
                Xw = X[:, 64 * i:64 * i + 64]
                print(name, 'wave', i, 'X in [%.3f, %.3f]' % (Xw.min(), Xw.max()), 'spikes', int(S[:, 64 * i:64 * i + 64].sum()))
                assert lo <= Xw.min() and Xw.max() <= hi, (name, i, Xw.min(), Xw.max())
                assert S[:, 64 * i:64 * i + 64].sum() >= 30, name
            assert np.any(X != case(name)[0])                          # the spikes did add to the currents
    assert REGIME['n64_neg_mid'][3][0][1] < 0 < REGIME['n64_mid'][3][0][0]


def test_edge_cases_reach_what_they_are_for():
    S, X, _, _ = host_reference('nt_lt_r', 0)
    N, R, nT = CASES['nt_lt_r'][:3]
    assert nT < R and np.all(S[:4].sum(axis=1) > 0)                    # spikes in bins 0 .. 3: impulses cut by the end
    assert np.any(X[1:] != case('nt_lt_r')[0][1:])
    S, X, _, _ = host_reference('nt1', 0)
    assert S.shape == (1, 3) and S.sum() > 0 and np.array_equal(X, case('nt1')[0])
    for name in ('r1', 'n1', 'n65', 'n300', 'n1024', 'lds_96k', 'lds_1024thr'):
        S, X, exc, _ = host_reference(name, 0)
        assert S.sum() > 10 and np.any(X != case(name)[0]), name
    assert host_reference('n65', 0)[0][:, 64].sum() > 0                # the neuron of the second wave spikes
    assert host_reference('n1024', 0)[0].any(axis=0).reshape(16, 64).any(axis=1).all()     # a spike in each of the 16 waves
    assert host_reference('n300', 0)[0][:, 256:].sum() > 0


def test_plan_of_the_sweep_cases():
    """Ring placement from pgl_simulate_batch_plan; the thread count by the documented rule of pgl_simulate_batch_dev (the
    plan call does not return it)."""
    for name, forms in PLAN.items():
        N, R = CASES[name][:2]
        ring = R * N * 8
        for flags, (in_lds, threads) in forms.items():
            assert _lib.simulate_batch_plan(N, R, flags) == (in_lds, 0 if in_lds else ring), (name, flags)
            assert in_lds == (flags == 0 and ring <= LDS_MAX), (name, flags)
            assert threads == (256 if N <= 256 and R * N <= 16384 else 1024), (name, flags)
    N, R = CASES['lds_96k'][:2]
    assert R * N * 8 == 98304 > 65536 and R * N <= 16384               # 256 threads, LDS beyond the default limit
    N, R = CASES['lds_1024thr'][:2]
    assert R * N * 8 == 153600 <= LDS_MAX and 16384 < R * N <= LDS_MAX // 8 == 20352
    assert CASES['n300'][0] > 256 and CASES['n1024'][0] == 1024 and CASES['n65'][0] == 65 and CASES['n1'][0] == 1
    assert CASES['r1'][1] == 1 and CASES['nt1'][2] == 1
    assert set(PLAN) == set(CASES) - {'small_exp', 'small_expl', 'n70', 'n130', 'high_rate', 'tail'}


def test_a_neurons_thresholds_do_not_depend_on_the_other_neurons():
    """Neuron m drives nobody (its AW rows are zero); a change of its own current can change only its own spikes.  With one
    shared stream in draw order the other neurons would see other thresholds."""
    X0, AW, nlin, seed = case('small_expl')
    m = 1
    AW = AW.copy()
    AW[m] = 0.0
    Xb = X0.copy()
    Xb[:, m] += 40.0
    Sa, Xa, _, _ = _lib.simulate_streams(X0, AW, nlin, DT, rep=2, seed=seed)
    Sb, _, _, _ = _lib.simulate_streams(Xb, AW, nlin, DT, rep=2, seed=seed)
    others = [n for n in range(X0.shape[1]) if n != m]
    assert not np.array_equal(Sa[:, m], Sb[:, m])
    assert np.array_equal(Sa[:, others], Sb[:, others])
    # and the restatement's record of the thresholds themselves: the same values, in the same order, for the others
    da = restate(X0, AW, nlin, DT, 2, seed)[3]
    db = restate(Xb, AW, nlin, DT, 2, seed)[3]
    for n in others:
        assert da[n] == db[n]
    assert len(da[m]) != len(db[m])
    k = min(len(da[m]), len(db[m]))
    assert da[m][:k] == db[m][:k]                                      # m's own stream is the same sequence, read further


def test_draw_values():
    n = 100000
    key = stream_keys(7, 3, 5)[2]
    u = uniforms(np.full(n, key, dtype=np.uint64), np.arange(n, dtype=np.uint64))
    assert u.min() > 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 4.0 * np.sqrt(1.0 / 12.0 / n)
    assert abs(u.var() - 1.0 / 12.0) <= 4.0 * np.sqrt(1.0 / 180.0 / n)    # var of the sample variance: (mu4 - sigma^4) / n
    # the largest and the smallest 53-bit value stay inside [0, 1]: never 0
    edge = (np.array([0, 2 ** 53 - 1], dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -53
    assert edge[0] > 0.0 and edge[1] <= 1.0
    # streams of different neurons / replicates / seeds are different sequences
    k10 = np.arange(10, dtype=np.uint64)
    a = uniforms(np.full(10, stream_keys(7, 3, 5)[2]), k10)
    for other in (stream_keys(7, 3, 5)[3], stream_keys(7, 4, 5)[2], stream_keys(8, 3, 5)[2]):
        assert not np.any(a == uniforms(np.full(10, other), k10))


def test_planner():
    assert _lib.simulate_batch_plan(64, 200) == (True, 0)
    assert _lib.simulate_batch_plan(128, 200) == (False, 200 * 128 * 8)
    assert _lib.simulate_batch_plan(5, 7, flags=1) == (False, 7 * 5 * 8)
    assert _lib.simulate_batch_plan(5, 7) == (True, 0)
    assert _lib.simulate_batch_plan(70, 33) == (True, 0)
    assert _lib.simulate_batch_plan(130, 200) == (False, 200 * 130 * 8)
    for bad in ((0, 7), (5, 0), (1025, 7)):
        with pytest.raises(_lib.PglError):
            _lib.simulate_batch_plan(*bad)


def test_bad_arguments_and_no_device():
    X0, AW, nlin, seed = case('small_exp')
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_batch(X0, AW, nlin, DT, 0)
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_batch(X0, AW, nlin, DT, 1, rep0=-1)
    with pytest.raises(_lib.PglError, match='nonlinearity'):
        _lib.simulate_batch(X0, AW, 7, DT, 1)
    with pytest.raises(_lib.PglError, match='argument'):
        _lib.simulate_streams(X0, AW, nlin, DT, rep=-1)
    if _lib.device_count() == 0:                                       # no quiet fall-back to the host loop
        with pytest.raises(_lib.PglError, match='device'):
            _lib.simulate_batch(X0, AW, nlin, DT, 1)


@pytest.mark.parametrize('name', sorted(CASES))
def test_decision_margin_of_the_gpu_cases(name):
    """No comparison acc > thr of the seeds the GPU tests use comes closer than 1e-9 (relative): a last-place difference
    between the device's and the host's exp / log, or in the order of a sum, cannot flip a spike decision."""
    for rep in range(CASES[name][5]):
        closest = host_reference(name, rep)[3]
        print(name, rep, closest)
        assert closest > 1e-9


def population(N, seed):
    from theano_pyglm_amd.models.model_factory import make_model, stabilize_sparsity
    from theano_pyglm_amd.population import Population
    popn = Population(stabilize_sparsity(make_model('standard_glm', N=N, dt=DT)))
    return popn, popn.sample(np.random.RandomState(seed))


POP = (4, 5, 3000, 21)         # N, parameter seed, nT, simulation seed of the GPU test that compares a Population's two routes


def test_decision_margin_of_the_population_case():
    N, pseed, nT, seed = POP
    popn, x = population(N, pseed)
    X0, AW = popn._simulation_inputs(x, (0, nT * DT), DT, None, 0.1)
    closest = _lib.simulate_streams(X0, np.ascontiguousarray(np.transpose(AW, (0, 2, 1))), popn.glm.nlin_model.kind, DT,
                                    rep=0, seed=seed)[3]
    print(closest)
    assert X0.shape == (nT, N) and closest > 1e-9


def test_population_simulate_batch_host_route():
    """Population.simulate_batch(device=False) loops the host reference on simulate's own X0 / AW; simulate itself keeps
    the reference's draw order (tests/test_host_logic.py holds it to the Python loop)."""
    N = 3
    popn, x = population(N, 3)
    out = popn.simulate_batch(x, (0, 1.0), DT, None, 0.1, 3, seed=5, rep0=2, currents=True, device=False)
    assert out['S'].shape == (3, 1000, N) and out['S'].dtype == np.uint8 and out['X'].shape == (3, 1000, N)
    assert np.array_equal(out['counts'], out['S'].sum(axis=1))
    X0, AW = popn._simulation_inputs(x, (0, 1.0), DT, None, 0.1)
    S, X, exc, _ = _lib.simulate_streams(X0, np.ascontiguousarray(np.transpose(AW, (0, 2, 1))), popn.glm.nlin_model.kind, DT,
                                         rep=3, seed=5)
    assert np.array_equal(out['S'][1], S) and np.array_equal(out['X'][1], X) and out['exceptions'][1] == exc
    none = popn.simulate_batch(x, (0, 1.0), DT, None, 0.1, 1, seed=5, rep0=3, spikes=False, device=False)
    assert none['S'] is None and none['X'] is None and np.array_equal(none['counts'][0], S.sum(axis=0))
