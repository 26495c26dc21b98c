"""The case table of the rate-window tests (tests/rate_cases.json), its reference, a numpy statement of the fold over draws
and the host mirror of the rule (test infrastructure, no GPU): tests/test_rate_cases.py keeps the reference honest on the
CPU, tests/test_rate_host.py holds the C rule to the numpy statement, tests/test_gpu_rate_windows.py runs the table on the
device.

Reference, independent of the device: currents from the oracle's features as in tests/rescale_reference.py (a direct
time-domain convolution of the spikes, one matrix product per case, plus the dense stimulus columns where a case has them),
the rate in numpy.longdouble (rescale_reference.rate_longdouble), and
    Lam[w] = dt * sum_{t in window w} lam_t,      obs[w] = sum_{t in window w} S[t]
summed in longdouble in the PLAIN order: one running sum per window, no pieces.  Windows: win bins counted from t_lo, the
last one short.

Bound on Lam (the pointwise sweep's, tests/pointwise_reference.py: same rate function, shorter sums):
|Lam_dev - Lam_ref| <= REL |Lam_ref| + ABS_A A_w with A_w the sum of the absolute terms -- here every term is positive, so
A_w = Lam_ref.

The fold over draws is stated in numpy in the order of csrc/pglm_ratewin.h (fold_numpy): Welford with the fused M2 step formed
exactly (fractions), min, max, the running mean of the Poisson mid-p value with its terms built by the recurrence.

A case: name, N, nT, kind, Dstim (dense stimulus columns), seed, rate_hz, bias (resized to N), silent (a neuron without
spikes), plant [[bin, neuron, count], ..], ranges ([t_lo, t_hi) or null = the whole recording), wins."""
import ctypes as C
import fractions
import functools
import json
import math
import os
import subprocess
import tempfile

import numpy as np

from oracle import glm_oracle as O
from tests import helpers as H
from tests import pointwise_reference as PR
from tests import rescale_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'rate_cases.json')
FIELDS = ('name', 'N', 'nT', 'kind', 'Dstim', 'seed', 'rate_hz', 'bias', 'silent', 'plant', 'ranges', 'wins')
PIECE = 256                    # PGL_RW_PIECE
NACC = 5                       # PGL_RW_NACC: mean, M2, min, max, pit
MAX_COUNT = 1024               # PGL_RW_MAX_COUNT
MAX_LAM = 700.0                # PGL_RW_MAX_LAM
REL, ABS_A = PR.REL, PR.ABS_A  # the bound of the pointwise block sums
N_DRAWS = 5


def load_cases():
    with open(CASES) as f:
        cases = json.load(f)
    for c in cases:
        assert sorted(c) == sorted(FIELDS), (c.get('name'), sorted(set(c) ^ set(FIELDS)))
    return cases


def ranges(c):
    """[(t_lo, t_hi)] of a case"""
    return [(0, c['nT']) if r is None else tuple(r) for r in c['ranges']]


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = [c for c in load_cases() if c['name'] == name][0]
    p = H.Problem(c['N'], c['nT'], RR.basis(), kind=c['kind'], rate_hz=c['rate_hz'], seed=c['seed'], weighted=True,
                  Dstim=c['Dstim'])
    p.S[:, c['silent']] = 0
    for t, n, k in c['plant']:
        p.S[t, n] = k
    p.theta[:, 0] = np.resize(np.asarray(c['bias'], dtype=float), c['N'])
    p._fS = O.convolve_with_basis(p.S.astype(float), p.ibasis)
    p.S.setflags(write=False)
    p.theta.setflags(write=False)
    return p


def problem(c):
    """helpers.Problem of the case (built once, shared, S and theta read-only)"""
    return _problem(c['name'])


def currents_of(p, theta):
    """total currents (nT, N) of the problem at the rows theta (N, P), float64"""
    N, B, D = p.N, p.B, p.Dstim
    w = theta[:, 1 + D:].reshape(N, N, B)                       # [post, pre, b]
    Wm = (p.Weff.T[:, :, None] * w).reshape(N, N * B).T         # [(pre, b), post]
    x = p.fS.reshape(p.nT, N * B).dot(Wm) + theta[:, 0][None, :]
    if D > 0:
        x = x + p.fstim.dot(theta[:, 1:1 + D].T)
    return x


def window_starts(n, win):
    """first bins (relative to t_lo) of the windows of win bins over a range of n bins"""
    return np.arange(0, n, win)


def n_windows(n, win):
    return -(-n // win)


def counts(x, S, kind, dt, win):
    """(Lam (n_win, N), obs (n_win, N)) float64 from the currents x (n, N) and spike counts S (n, N) of a range: longdouble
    rates, one plain longdouble running sum per window"""
    starts = window_starts(x.shape[0], win)
    lam = RR.rate_longdouble(x, kind)
    Lam = np.asarray(dt * np.add.reduceat(lam, starts, axis=0), dtype=np.float64)
    obs = np.add.reduceat(np.asarray(S, dtype=np.int64), starts, axis=0).astype(np.float64)
    return Lam, obs


@functools.lru_cache(maxsize=None)
def _reference(name, t_lo, t_hi, win):
    p = _problem(name)
    Lam, obs = counts(currents_of(p, p.theta)[t_lo:t_hi], p.S[t_lo:t_hi], p.kind, p.dt, win)
    Lam.setflags(write=False)
    obs.setflags(write=False)
    return Lam, obs


def reference(c, t_lo, t_hi, win):
    """(Lam, obs), each (n_win, N), over [t_lo, t_hi) in windows of win bins; computed once, read-only"""
    return _reference(c['name'], t_lo, t_hi, win)


def ratio(Lam, Lam_ref):
    """worst |Lam - Lam_ref| / ((REL + ABS_A) Lam_ref) (every term of the sum is positive: the absolute sum is Lam_ref); a
    value that is not finite, or a shape that differs, counts as infinitely far"""
    if Lam.shape != Lam_ref.shape:
        return np.inf
    d = np.abs(Lam - Lam_ref) / ((REL + ABS_A) * np.abs(Lam_ref))
    return float(np.max(np.where(np.isfinite(d), d, np.inf)))


@functools.lru_cache(maxsize=None)
def _draws(name):
    p = _problem(name)
    rng = np.random.default_rng(7000 + p.N + p.nT)
    th = np.repeat(p.theta[None], N_DRAWS, axis=0)
    z = rng.standard_normal(th.shape)
    th[:, :, 0] += 0.1 * np.maximum(1.0, np.abs(p.theta[None, :, 0])) * z[:, :, 0]
    th[:, :, 1:] += 0.05 * np.maximum(np.abs(p.theta[None, :, 1:]), 0.05) * z[:, :, 1:]
    th.setflags(write=False)
    return th


def draws(c):
    """(5, N, P) parameter rows: theta plus a seeded jitter of 10 % of max(1, |bias|) on the bias and 5 % on the weights"""
    return _draws(c['name'])


# ---- the Poisson mid-p value and the fold over draws, in the header's order ------------------------------------------------
def midp(lam, y):
    """u = F(y - 1) + 0.5 f(y) of the counts y under Poisson(lam), elementwise float64 in the header's order: term_0 =
    exp(-lam) (math.exp: the C library's), term_k = term_{k-1} * lam / k, the cdf added in ascending k from 0; NaN where
    lam > 700, y > 1024 or lam is not finite"""
    lam = np.asarray(lam, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    out = np.full(lam.shape, np.nan)
    for i in np.ndindex(lam.shape):
        l, n = float(lam[i]), float(y[i])
        if not (l <= MAX_LAM) or not (n <= MAX_COUNT):
            continue
        term, cdf = math.exp(-l), 0.0
        for k in range(1, int(n) + 1):
            cdf += term
            term = term * l / float(k)
        out[i] = cdf + 0.5 * term
    return out


def _fma(a, b, c):
    """round(a b + c), exactly"""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def fold_numpy(lam, y):
    """the state (5,) + y.shape -- mean, M2, min, max, pit -- after folding the draws lam (S, ...) against the counts y (...)
    in order, by the rule of csrc/pglm_ratewin.h, elementwise in float64"""
    lam = np.asarray(lam, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    acc = np.empty((NACC,) + y.shape)
    for i in np.ndindex(y.shape):
        mean = m2 = mn = mx = pit = 0.0
        for s in range(lam.shape[0]):
            l = float(lam[(s,) + i])
            if not np.isfinite(l) or (s > 0 and not np.isfinite(mean)):
                mean = m2 = mn = mx = pit = np.nan
                continue
            u = float(midp(l, y[i]))
            if s == 0:
                mean, m2, mn, mx, pit = l, 0.0, l, l, u
                continue
            d = l - mean
            mean = mean + d / float(s + 1)
            m2 = _fma(d, l - mean, m2)
            mn, mx = min(mn, l), max(mx, l)
            pit = pit + (u - pit) / float(s + 1)
        acc[(slice(None),) + i] = (mean, m2, mn, mx, pit)
    return acc


def poisson_pmf_check(lam, kmax):
    """(the recurrence's terms term_0 .. term_kmax in float64, an independent statement of the same pmf): scipy.stats.poisson
    where it is installed, math.lgamma otherwise"""
    term = [math.exp(-lam)]
    for k in range(1, kmax + 1):
        term.append(term[-1] * lam / float(k))
    k = np.arange(kmax + 1)
    try:
        from scipy.stats import poisson
        ref = poisson.pmf(k, lam)
    except ImportError:
        ref = np.array([math.exp(-lam + i * math.log(lam) - math.lgamma(i + 1.0)) if lam > 0 else float(i == 0) for i in k])
    return np.array(term), ref


def ks_uniform(u):
    """KS distance of the sample u from the uniform law on [0, 1]"""
    u = np.sort(np.asarray(u, dtype=float))
    n = u.size
    return float(max(np.max(np.arange(1, n + 1) / n - u), np.max(u - np.arange(n) / n)))


# ---- host mirror of the rule (csrc/pglm_ratewin.h through tests/csrc/ratewin_host.c) ----------------------------------------
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='ratewin_host_'), 'ratewin_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so,
                               os.path.join(ROOT, 'tests', 'csrc', 'ratewin_host.c'), '-lm'])
        Lb = C.CDLL(so)
        Lb.rw_max_lam.restype = C.c_double
        Lb.rw_windows.restype = C.c_longlong
        Lb.rw_windows.argtypes = [C.c_longlong, C.c_longlong]
        Lb.rw_midp.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        Lb.rw_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
        Lb.rw_run.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
        Lb.rw_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_double, C.c_void_p, C.c_void_p]
        _LIB = Lb
    return _LIB


def host_midp(lam, y):
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    y = np.ascontiguousarray(np.broadcast_to(y, lam.shape), dtype=np.float64)
    u = np.empty(lam.shape)
    lib().rw_midp(lam.ctypes.data, y.ctypes.data, lam.size, u.ctypes.data)
    return u


def host_fold(lam, y, garbage=True):
    """the state (5,) + y.shape after folding the draws lam (S, ...) against y (...) in order with the host build of the
    rule; the state starts as NaN-free garbage (draw 0 must initialise it)"""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    assert lam.shape[1:] == y.shape
    acc = np.full((NACC, y.size), 12345.678 if garbage else 0.0)
    lib().rw_run(lam.ctypes.data, y.ctypes.data, lam.shape[0], y.size, acc.ctypes.data)
    return acc.reshape((NACC,) + y.shape)


def host_counts(lam_t, spikes, win, dt):
    """(Lam (n_win), obs (n_win)) of one neuron from float64 rates and int spike counts over a range, in the header's pieced
    order"""
    lam_t = np.ascontiguousarray(lam_t, dtype=np.float64)
    sp = np.ascontiguousarray(spikes, dtype=np.int32)
    nw = n_windows(lam_t.size, win)
    Lam, obs = np.empty(nw), np.empty(nw)
    lib().rw_counts(lam_t.ctypes.data, sp.ctypes.data, lam_t.size, int(win), float(dt), Lam.ctypes.data, obs.ctypes.data)
    return Lam, obs
