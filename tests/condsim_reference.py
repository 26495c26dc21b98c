"""What the tests of the clamped simulation share: the cases of tests/condsim_cases.json and their inputs, the gcc build of the
host mirror tests/csrc/condsim_host.c (the rules of csrc/pglm_condsim.h), a longdouble reference of the clamped currents.

A case: X0 (nT, N) at about 40 Hz per neuron (dt = 1 ms), signed coupling AW (N, R, N) that decays over the R taps, and a
recording S_obs (nT, N) of Poisson counts at about 60 Hz with a few bins forced to 2 and 3 spikes.  'silent': that neuron's
X0 is -40 (it never fires); 'silent_pre': that neuron has no recorded event; 'boost': added to X0 (rate * dt = 1.5: spikes in
every bin); 'burst' [t0, t1, x]: X0 = x in bins t0 .. t1 - 1 with a weak self-history (more own spike bins inside R than the
queue of the device holds: the fallback ring); 'exceptions': the high-rate currents of the batched simulation's case (bins with
rate * dt = 14: the neuron's cap of 10).  Every case but 'exceptions' has no exception and no spike decision closer than
1e-9 (relative) to its threshold; tests/test_condsim_cases.py asserts both on the CPU for the stream indices the GPU test runs."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.001
_lib = None


def load():
    with open(os.path.join(ROOT, 'tests', 'condsim_cases.json')) as f:
        return json.load(f)


CASES = load()
BY_NAME = dict((c['name'], c) for c in CASES)


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, 'tests', 'csrc', 'condsim_host.so')
        srcs = [os.path.join(ROOT, 'tests', 'csrc', 'condsim_host.c')] + \
            [os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', h) for h in ('pglm_condsim.h', 'pglm_hmc.h', 'pglm_linesearch.h')]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, srcs[0], '-lm'])
        L = ctypes.CDLL(so)
        vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        L.condsim_currents.restype = None
        L.condsim_currents.argtypes = [vp, vp, vp, vp, vp, ll, ci, ci, vp]
        L.condsim_run.restype = ctypes.c_double
        L.condsim_run.argtypes = [vp, vp, ll, ci, ci, ci, ctypes.c_double, ctypes.c_ulonglong, ci, ci, vp, vp, vp]
        L.condsim_fold.restype = None
        L.condsim_fold.argtypes = [vp, ci, ll, ci, ll, vp, vp, ci]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(X0, AW, S_obs) of a case, read-only"""
    c = BY_NAME[name]
    N, R, nT, nlin = c['N'], c['R'], c['nT'], c['nlin']
    rng = np.random.RandomState(2000 + c['seed'])
    rate = 40.0
    X0 = (np.log(rate) if nlin == 'exp' else rate) + (0.3 if nlin == 'exp' else 10.0) * rng.randn(nT, N)
    W = rng.randn(N, N) * ((0.4 if nlin == 'exp' else 8.0) / np.sqrt(N))
    AW = W[:, None, :] * np.exp(-np.arange(R) / (0.3 * R))[None, :, None] * (1.0 + 0.2 * rng.rand(N, R, N))
    S = rng.poisson(0.06, size=(nT, N)).astype(np.uint8)
    S[rng.randint(0, nT, size=4), rng.randint(0, N, size=4)] = 2
    S[rng.randint(0, nT), rng.randint(0, N)] = 3
    if 'silent' in c:
        X0[:, c['silent']] = -40.0
    if 'silent_pre' in c:
        S[:, c['silent_pre']] = 0
    if 'boost' in c:
        X0 += c['boost']
    if 'burst' in c:
        t0, t1, x = c['burst']
        AW *= 0.05
        X0[t0:t1] = x
    if c.get('exceptions'):
        X0 += np.log(25.0)
        X0[50::40] = np.log(14.0 / DT)
        AW *= 0.1
    for a in (X0, AW, S):
        a.setflags(write=False)
    return X0, AW, S


def nlin_kind(nlin):
    return {'exp': 0, 'explinear': 1}[nlin]


def host_currents(X0, AW, S):
    """the gcc mirror of the currents rule"""
    from theano_pyglm_amd._lib import spike_events
    X0 = np.ascontiguousarray(X0, dtype=np.float64)
    AW = np.ascontiguousarray(AW, dtype=np.float64)
    pre, cnt, off = spike_events(S)
    pre, cnt = np.append(pre, np.int32(0)), np.append(cnt, np.uint8(0))          # (never empty arrays for ctypes)
    Xc = np.empty_like(X0)
    lib().condsim_currents(_p(X0), _p(AW), _p(pre), _p(cnt), _p(off), X0.shape[0], X0.shape[1], AW.shape[1], _p(Xc))
    return Xc


def host_run(Xc, AW, nlin, dt, n_rep, seed, rep0):
    """the gcc mirror of the chains: (S (n_rep, nT, N) uint8, exceptions (N), closest decision margin)"""
    Xc = np.ascontiguousarray(Xc, dtype=np.float64)
    AW = np.ascontiguousarray(AW, dtype=np.float64)
    nT, N = Xc.shape
    R = AW.shape[1]
    S = np.empty((n_rep, nT, N), dtype=np.uint8)
    exc = np.zeros(N, dtype=np.int64)
    work = np.empty(nT + R)
    closest = lib().condsim_run(_p(Xc), _p(AW), nT, N, R, nlin_kind(nlin), float(dt), int(seed), int(rep0), int(n_rep), _p(S),
                                _p(exc), _p(work))
    return S, exc, float(closest)


def host_fold(S, obs, win, acc=None):
    """the gcc mirror of the accumulators: (6, n_win, N) int64, continuing acc where given"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    obs = np.ascontiguousarray(obs, dtype=np.int64)
    n_rep, nT, N = S.shape
    out = np.empty((6,) + obs.shape, dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64, order='C')
    lib().condsim_fold(_p(S), n_rep, nT, N, int(win), _p(obs), _p(out), 0 if acc is None else 1)
    return out


@functools.lru_cache(maxsize=None)
def mirror(name):
    """What the device must give for a case: Xc, S, counts (n_rep, N), exceptions, the six planes, the margin.  Computed
    once, shared, read-only."""
    from theano_pyglm_amd._lib import window_counts
    c = BY_NAME[name]
    X0, AW, S_obs = make_case(name)
    Xc = host_currents(X0, AW, S_obs)
    S, exc, closest = host_run(Xc, AW, c['nlin'], DT, c['n_rep'], c['seed'], c['rep0'])
    obs = window_counts(S_obs, c['win'])
    out = {'Xc': Xc, 'S': S, 'counts': S.sum(axis=1, dtype=np.int64), 'exceptions': exc, 'obs': obs,
           'acc': host_fold(S, obs, c['win']), 'closest': closest}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def diagonal_only(AW):
    """AW with only its [n, :, n] entries kept"""
    D = np.zeros_like(AW)
    i = np.arange(AW.shape[0])
    D[i, :, i] = AW[i, :, i]
    return D


def currents_longdouble(X0, AW, S):
    """(Xc in longdouble, the sum of the absolute terms, the number of additions) per element -- the mathematics, the order
    below its precision"""
    X = np.array(X0, dtype=np.longdouble)
    A = np.abs(X)
    M = np.zeros(X.shape, dtype=np.int64)
    nT, N = X.shape
    R = AW.shape[1]
    AWl = np.array(AW, dtype=np.longdouble)
    for p in range(N):
        a = AWl[p].copy()
        a[:, p] = 0
        for s in np.flatnonzero(S[:, p]):
            n = min(R, nT - s - 1)
            X[s + 1:s + 1 + n] += int(S[s, p]) * a[:n]
            A[s + 1:s + 1 + n] += int(S[s, p]) * np.abs(a[:n])
            M[s + 1:s + 1 + n, np.arange(N) != p] += int(S[s, p])
    return X, A, M


def longest_own_spike_run(S, R):
    """the largest number of distinct spike bins of one chain inside any R consecutive bins; S (..., nT, N)"""
    b = (np.asarray(S) > 0).astype(np.int64)
    c = np.cumsum(b, axis=-2)
    lead = np.zeros_like(c[..., :1, :])
    c = np.concatenate([lead, c], axis=-2)
    nT = b.shape[-2]
    w = min(R, nT)
    return int((c[..., w:, :] - c[..., :nT - w + 1, :]).max())
