"""The case table of the goodness-of-fit sweep (tests/ks_cases.json), its longdouble references and numpy mirrors of the
kernels with switchable faults (test infrastructure, no GPU): tests/test_ks_cases.py keeps the table honest on the CPU,
tests/test_gof_correct_host.py checks the gcc build of csrc/pglm_gof.h (tests/csrc/gof_host.c), tests/test_gpu_ks.py runs the
table on the device.

Corrected intervals (rule: include/pyglm_hip.h, pgl_rescale_corr).  Reference: currents as tests/rescale_reference.py forms
them (its plant / bias / basis builders by import), the rate and numpy.cumsum in numpy.longdouble, open_k = dt (cum[t_k - 1] -
cum[t_{k-1}]), e_k = -log1p(u expm1(-q_k)) in longdouble, u from an integer restatement of the formula (uniform below).
Bound: rescale_reference's, |tau' - ref| <= 1e-10 ref + 1e-12 Lambda_ref.

KS (rule: csrc/pglm_gof.h).  Reference: z = -expm1(-tau) and the two maxima in longdouble on numpy.sort; bound on D: 1e-14.

Contents of a KS case (seeded): uniform (tau ~ Exp(1), z uniform), equal (one value), half_tied (half of the values 0.05,
the rest 0.1 + Exp(1), shuffled: the largest distance lies at the tied values), clumped (every z in [1 - 1e-12, 1]: tau =
27.7 .. 40), zero (tau = 0), one_inf / one_nan / one_negative (Exp(1) with one such value in the middle), sorted / reversed (Exp(1) in that order)."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

from oracle import glm_oracle as O
from tests import helpers as H
from tests import rescale_reference as RR

ROOT = RR.ROOT
CASES = os.path.join(ROOT, 'tests', 'ks_cases.json')
LD = np.longdouble
L = RR.L
TILE = 4096                     # PGL_KS_TILE
KS_TOL = 1e-14
G = 0x9e3779b97f4a7c15
MASK = (1 << 64) - 1
CORR_FAULTS = ('sub_q', 'j_from_range', 'grid_from_range')
KS_FAULTS = ('tie_lt', 'pad_zero', 'tile_edge')


@functools.lru_cache(maxsize=None)
def load():
    with open(CASES) as f:
        t = json.load(f)
    assert sorted(t) == ['corr', 'ks', 'multi']
    for c in t['ks']:
        assert sorted(c) == ['content', 'hits', 'n', 'name', 'seed'], c
    for c in t['corr']:
        assert sorted(c) == sorted(RR.FIELDS), c
    return t


# ---- the uniforms -----------------------------------------------------------------------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def uniform(seed, draw, n, j):
    """u of (seed, draw, neuron, event index) in Python integers: exact"""
    z = _mix((seed + G) & MASK)
    for v in (draw, n, j):
        z = _mix((z + G * (v + 1)) & MASK)
    return (float(z >> 11) + 0.5) * 2.0 ** -53


# ---- corrected intervals ------------------------------------------------------------------------------------------------------
def corr_ranges(c):
    return RR.ranges(c)


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = [c for c in load()['corr'] if c['name'] == name][0]
    p = H.Problem(c['N'], c['nT'], RR.basis(), kind=c['kind'], rate_hz=c['rate_hz'], seed=c['seed'], weighted=True,
                  w_scale=c['w_scale'])
    RR.plant(p.S, c)
    p.theta[:, 0] = RR._biases(c, np.random.default_rng(500 + c['seed']))
    p._fS = O.convolve_with_basis(p.S.astype(float), p.ibasis)
    N, B = p.N, p.B
    w = p.theta[:, 1:].reshape(N, N, B)
    Wm = (p.Weff.T[:, :, None] * w).reshape(N, N * B).T
    p.x = p.fS.reshape(p.nT, N * B).dot(Wm) + p.theta[:, 0][None, :]
    for a in (p.S, p.theta, p.x):
        a.setflags(write=False)
    return p


def problem(c):
    return _problem(c['name'])


def first_index(p, n, t_lo):
    """index of the first event of [t_lo, ..) in neuron n's whole list"""
    return int(np.count_nonzero(p.S[:t_lo, n]))


@functools.lru_cache(maxsize=None)
def _corr_reference(name, t_lo, t_hi, seed, draw):
    p = _problem(name)
    q = LD(p.dt) * RR.rate_longdouble(p.x[t_lo:t_hi], p.kind)
    cum = np.cumsum(q, axis=0)
    taus, opens, qs, lam = [], [], [], np.asarray(cum[-1], dtype=np.float64)
    for n in range(p.N):
        ev = RR.events(p.S, n, t_lo, t_hi)
        j0 = first_index(p, n, t_lo)
        if ev.size < 2:
            taus.append(np.zeros(0)); opens.append(np.zeros(0)); qs.append(np.zeros(0))
            continue
        op = cum[ev[1:] - 1, n] - cum[ev[:-1], n]
        qk = q[ev[1:], n]
        u = np.array([uniform(seed, draw, n, j0 + i) for i in range(1, ev.size)], dtype=LD)
        e = -np.log1p(u * np.expm1(-qk))
        taus.append(np.asarray(op + e, dtype=np.float64))
        opens.append(np.asarray(op, dtype=np.float64))
        qs.append(np.asarray(qk, dtype=np.float64))
    for a in taus + opens + qs:
        a.setflags(write=False)
    return tuple(taus), tuple(opens), tuple(qs), lam


def corr_reference(c, t_lo, t_hi, seed=0, draw=0):
    """(tau' per neuron, open per neuron, q of the later event's bin per neuron, Lambda (N)); computed once, read-only"""
    return _corr_reference(c['name'], t_lo, t_hi, seed, draw)


def corr_ratio(tau, off, ref):
    """worst |dtau'| / (1e-10 ref + 1e-12 Lambda_ref); a value that is not finite counts as infinitely far"""
    w = 0.0
    for n, tr in enumerate(ref[0]):
        if tr.size:
            d = np.abs(tau[off[n]:off[n + 1]] - tr) / (RR.REL * tr + RR.ABS_LAMBDA * ref[3][n])
            w = max(w, float(np.max(np.where(np.isfinite(d), d, np.inf))))
    return w


def own_class(x):
    """the series of log1p a lane's own current allows: 2 tail (|x| > 9.25), 1 mid (|x| > 2.3), 0 full"""
    a = np.abs(x)
    return np.where(a > RR.VOTE_TAIL, 2, np.where(a > RR.VOTE_MID, 1, 0))


def vote_class(c, t_lo, t_hi):
    """(bins, N): the series pgl_lambda_only would use at every (bin, neuron) of the range under the geometry of
    k_rcorr_chunk -- a lane per (absolute chunk from t_lo // 256, column of the padded row of xs = 16 ceil(N / 16)), 64
    consecutive lanes a wave, every lane walking its chunk from its first bin inside the range in groups of 8 rows, the rows
    past its chunk at the bare bias: the weakest series any lane of the wave allows at that step."""
    p = problem(c)
    N, xs = p.N, RR.xs_of(p.N)
    c0 = t_lo // L
    nch = -(-t_hi // L) - c0
    out = np.full((t_hi - t_lo, N), -1)
    bias_cls = own_class(p.theta[:, 0])
    lanes = [(ch, j) for ch in range(nch) for j in range(xs)]
    for w in range(0, len(lanes), 64):
        wave = [(ch, j) for ch, j in lanes[w:w + 64] if j < N]
        geo = []
        for ch, j in wave:
            a = max((c0 + ch) * L, t_lo)
            b = min((c0 + ch + 1) * L, t_hi)
            geo.append((j, a, b - a, -(-(b - a) // RR.UNROLL) * RR.UNROLL))
        for k in range(max(g[3] for g in geo)):
            act = [g for g in geo if k < g[3]]
            cls = min(int(own_class(p.x[a + k, j])) if k < ln else int(bias_cls[j]) for j, a, ln, _ in act)
            for j, a, ln, _ in act:
                if k < ln:
                    out[a + k - t_lo, j] = cls
    assert out.min() >= 0
    return out


def _ssum(v):
    """the serial sum 0 + v[0] + v[1] + .. in float64 (numpy.cumsum adds in order)"""
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def corr_mirror(c, t_lo, t_hi, seed=0, draw=0, fault=None):
    """(tau' concatenated, offsets) by the kernels' decomposition in float64 on the rates O.nlin(x): chunks on the ABSOLUTE
    grid of 256 bins, serial in-chunk sums that start anew behind every event; an interval is the sum behind the earlier
    event to the end of its chunk, the whole chunks between one by one in order, the later event's chunk up to its bin
    (same chunk: the one sum between the two events); tau' = dt s + (-log1p(u expm1(-dt lam_b))).
    Faults: 'sub_q' forms the whole interval up to and including the event bin from running sums, as the uncorrected kernels
    do, and subtracts q_k from it; 'j_from_range' counts the event index from the time range; 'grid_from_range' anchors the
    chunk grid at t_lo."""
    assert fault is None or fault in CORR_FAULTS
    p = problem(c)
    dt = p.dt
    lam = O.nlin(p.x[t_lo:t_hi], p.kind)
    g0 = 0 if fault == 'grid_from_range' else t_lo             # bins of the range are relative: chunk of bin t = (g0 + t) // L
    lo = lambda ch: max(ch * L - g0, 0)                        # first bin of absolute chunk ch, relative, clipped to the range
    taus = []
    for n in range(p.N):
        ev = RR.events(p.S, n, t_lo, t_hi)
        j0 = 0 if fault == 'j_from_range' else first_index(p, n, t_lo)
        out = np.zeros(max(ev.size - 1, 0))
        col = lam[:, n]
        for i in range(1, ev.size):
            a, b = int(ev[i - 1]), int(ev[i])
            ca, cb = (g0 + a) // L, (g0 + b) // L
            qb = col[b]
            if fault == 'sub_q':
                run = lambda t: _ssum(col[lo((g0 + t) // L):t + 1])             # inclusive running sum of t's chunk
                if ca == cb:
                    s = run(b) - run(a)
                else:
                    s = _ssum(col[lo(ca):lo(ca + 1)]) - run(a)
                    for ch in range(ca + 1, cb):
                        s = s + _ssum(col[lo(ch):lo(ch + 1)])
                    s = s + run(b)
            elif ca == cb:
                s = _ssum(col[a + 1:b])
            else:
                s = _ssum(col[a + 1:lo(ca + 1)])
                for ch in range(ca + 1, cb):
                    s = s + _ssum(col[lo(ch):lo(ch + 1)])
                s = s + _ssum(col[lo(cb):b])
            u = uniform(seed, draw, n, j0 + i)
            e = -np.log1p(u * np.expm1(-(dt * qb)))
            out[i - 1] = (dt * s - dt * qb) + e if fault == 'sub_q' else dt * s + e
        taus.append(out)
    return np.concatenate(taus) if taus else np.zeros(0), RR.offsets(taus)


# ---- KS -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _content(content, n, seed):
    rng = np.random.default_rng(9000 + seed)
    tau = rng.exponential(size=n)
    if content == 'equal':
        tau = np.full(n, 0.6931471805599453)
    elif content == 'half_tied':
        tau += 0.1
        tau[:n // 2] = 0.05
        tau = tau[rng.permutation(n)]
    elif content == 'clumped':
        tau = rng.uniform(27.7, 40.0, size=n)
    elif content == 'zero':
        tau = np.zeros(n)
    elif content == 'one_inf':
        tau[n // 2] = np.inf
    elif content == 'one_nan':
        tau[n // 2] = np.nan
    elif content == 'one_negative':
        tau[n // 2] = -1e-300
    elif content == 'sorted':
        tau = np.sort(tau)
    elif content == 'reversed':
        tau = np.sort(tau)[::-1].copy()
    else:
        assert content == 'uniform', content
    tau.setflags(write=False)
    return tau


def ks_tau(c):
    return _content(c['content'], c['n'], c['seed'])


@functools.lru_cache(maxsize=None)
def multi():
    """(tau, off) of the 300-segment call"""
    m = load()['multi']
    lens = [m['lengths'][i % len(m['lengths'])] for i in range(m['segments'])]
    parts = [_content('uniform' if i % 5 else 'half_tied', n, 100 * m['seed'] + i) for i, n in enumerate(lens)]
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    tau = np.concatenate(parts)
    tau.setflags(write=False)
    return tau, off


def ks_reference(tau):
    """(D, D+, D-, n) of one segment in longdouble; NaN distances for n < 2 or a NaN / negative tau"""
    tau = np.asarray(tau, dtype=np.float64)
    n = tau.size
    if n < 2 or not np.all(tau >= 0.0):
        return np.array([np.nan, np.nan, np.nan, n])
    z = np.sort(-np.expm1(-tau.astype(LD)))
    dp = (np.arange(1, n + 1, dtype=LD) / LD(n) - z).max()
    dm = (z - np.arange(0, n, dtype=LD) / LD(n)).max()
    return np.array([float(max(dp, dm)), float(dp), float(dm), n])


def ks_from_sorted(z):
    """numpy's arithmetic of inference/gof.py on a sorted float64 sample: (D, D+, D-)"""
    n = z.size
    dp = (np.arange(1.0, n + 1) / n - z).max()
    dm = (z - np.arange(0.0, n) / n).max()
    return max(dp, dm), dp, dm


def network_steps(P):
    """[(k, j)] of the network on P slots: j = 0 is the flip step of merge k"""
    steps, k = [], 2
    while k <= P:
        steps.append((k, 0))
        j = k >> 2
        while j >= 1:
            steps.append((k, j))
            j >>= 1
        k <<= 1
    return steps


def ks_mirror(tau, fault=None):
    """(D, D+, D-, n, zsorted) by the kernel's rule in float64: z, the network on the index space padded to a power of two
    (the slots >= n a +inf that never moves), the maxima with numpy's arithmetic.  Faults: 'tie_lt' ranks a value by the
    number of values strictly below it in both maxima; 'pad_zero' pads with 0; 'tile_edge' runs the steps j >= TILE on
    global memory and the steps j < TILE / 2 on the tile: the half-cleaner j = TILE / 2 falls between the two."""
    assert fault is None or fault in KS_FAULTS
    tau = np.asarray(tau, dtype=np.float64)
    n = tau.size
    nan = np.nan
    if n < 2 or not np.all(tau >= 0.0):
        return nan, nan, nan, n, -np.expm1(-tau)
    P = 1
    while P < n:
        P <<= 1
    a = np.full(P, 0.0 if fault == 'pad_zero' else np.inf)
    a[:n] = -np.expm1(-tau)
    p = np.arange(P // 2)
    for k, j in network_steps(P):
        if fault == 'tile_edge' and j == TILE // 2:
            continue
        if j == 0:
            h = k >> 1
            b, r = (p & ~(h - 1)) << 1, p & (h - 1)
            i, l = b + r, b + k - 1 - r
        else:
            i = ((p & ~(j - 1)) << 1) | (p & (j - 1))
            l = i + j
        lo, hi = np.minimum(a[i], a[l]), np.maximum(a[i], a[l])
        a[i], a[l] = lo, hi
    z = a[:n]
    if fault == 'tie_lt':
        rank = np.searchsorted(z, z, side='left').astype(float)
        dp, dm = ((rank + 1.0) / n - z).max(), (z - rank / n).max()
        return max(dp, dm), dp, dm, n, z
    D, dp, dm = ks_from_sorted(z)
    return D, dp, dm, n, z


# ---- the gcc build of csrc/pglm_gof.h ---------------------------------------------------------------------------------------------
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='gof_host_'), 'gof_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'gof_host.c'), '-lm'])
        Lb = C.CDLL(so)
        Lb.gof_uniform.argtypes = [C.c_uint64] * 4
        Lb.gof_uniform.restype = C.c_double
        Lb.gof_event_term.argtypes = [C.c_double, C.c_double]
        Lb.gof_event_term.restype = C.c_double
        Lb.gof_ks.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        Lb.gof_ks.restype = None
        Lb.gof_corr.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_uint64,
                                C.c_longlong, C.c_double, C.c_void_p]
        _LIB = Lb
    return _LIB


def host_ks(tau, off):
    """(ks (M, 4), zs) of the host build"""
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    M = off.size - 1
    ks, zs = np.full((M, 4), -7.0), np.full(max(tau.size, 1), -7.0)
    tt = tau if tau.size else np.zeros(1)
    lib().gof_ks(tt.ctypes.data, off.ctypes.data, M, ks.ctypes.data, zs.ctypes.data)
    return ks, zs[:tau.size]


def host_corr(c, t_lo, t_hi, seed=0, draw=0):
    """(tau' concatenated, offsets) of the host build on the float64 rates O.nlin(x)"""
    p = problem(c)
    lam = np.ascontiguousarray(O.nlin(p.x[t_lo:t_hi], p.kind))
    taus = []
    for n in range(p.N):
        ev = np.ascontiguousarray(RR.events(p.S, n, t_lo, t_hi), dtype=np.int32)
        out = np.full(max(ev.size - 1, 1), np.nan)
        rc = lib().gof_corr(lam[:, n:].ctypes.data, p.N, t_hi - t_lo, t_lo, ev.ctypes.data, int(ev.size), first_index(p, n, t_lo), n,
                            seed, draw, p.dt, out.ctypes.data)
        assert rc == 0
        taus.append(out[:max(ev.size - 1, 0)])
    return np.concatenate(taus) if taus else np.zeros(0), RR.offsets(taus)
