"""The case table of the time-rescaling sweep (tests/rescale_cases.json), its reference and a numpy mirror of the kernels'
three-step decomposition (test infrastructure, no GPU): tests/test_rescale_cases.py keeps the table honest on the CPU,
tests/test_gpu_rescale_sweep.py runs it on the device.

Reference, independent of the device: currents x = F theta from the oracle's features (a direct time-domain convolution of
the spikes; one matrix product per case: x[:, n] = bias_n + sum_{n', b} fS[:, n', b] (Weff[n', n] w[n, n', b]), the product
tests/test_gpu_gof.py forms row by row with hvp_reference.feature_rows), the rate in numpy.longdouble -- exp(x), or
max(x, 0) + log1p(exp(-|x|)) -- numpy.cumsum in longdouble, intervals by the definition in include/pyglm_hip.h.

Bound (tests/test_gpu_gof.py's): |tau_dev - tau_ref| <= 1e-10 tau_ref + 1e-12 Lambda_ref per interval, |Lambda_dev -
Lambda_ref| <= (1e-10 + 1e-12) Lambda_ref.  The second term covers the f64 summation: the kernels add at most 256 (chunk)
+ ceil(nchunks / 64) (segment) + 64 (scan) terms into any prefix, (256 + 3 + 64) 2^-53 = 3.6e-14 of Lambda at the largest
case.

Spikes of a case: helpers.Problem's seeded Poisson background, then the `plant` entries in order (each clears its column
first unless "keep" is set):
  bins    [[bin, count], ...]
  chunks  [chunk, ...]: one event per listed chunk of the grid that starts at bin 0, at bin 256 chunk + (37 i mod 256)
  span    true: events on bin 3 and on bin nT - 2 (chunk 0 and the last chunk, nothing in between)
  dense   [first, last): an event on every bin, two spikes on every seventh
Biases of a case (`bias`): null = helpers.Problem's (20 +- 0.3), or {"lo", "hi", "sign"}: values evenly spread over
[lo, hi] in a seeded order, taken as they are ('+'), negated ('-') or negated for odd neurons ('alt'), or {"list": [...]}
repeated over the neurons."""
import functools
import json
import os

import numpy as np

from oracle import glm_oracle as O
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'rescale_cases.json')
FIELDS = ('name', 'N', 'nT', 'kind', 'rate_hz', 'w_scale', 'bias', 'seed', 'plant', 'ranges')
L = 256                        # PGL_RS_CHUNK
SEGS = 64                      # PGL_RS_SEGS
UNROLL = 8                     # PGL_RS_UNROLL
STRIDE = 256                   # threads of k_rescale_finish
REL, ABS_LAMBDA = 1e-10, 1e-12
VOTE_TAIL, VOTE_MID = 9.25, -np.log(0.1)      # pgl_lambda_only: e^-|x| < e^-9.25 / < 0.1, by a vote of the wave
FAULTS = ('no_cum', 'scan_late', 'no_tail_mask', 'stride_once')


def load_cases():
    with open(CASES) as f:
        cases = json.load(f)
    for c in cases:
        assert sorted(c) == sorted(FIELDS), (c.get('name'), sorted(set(c) ^ set(FIELDS)))
        for r in c['ranges']:
            assert sorted(r) == ['hits', 't'], (c['name'], r)
    return cases


def ranges(c):
    """[(t_lo, t_hi, hits)] of a case; "t": null is the whole recording"""
    return [((0, c['nT']) if r['t'] is None else tuple(r['t'])) + (r['hits'],) for r in c['ranges']]


def basis():
    return np.ascontiguousarray(H.std_ibasis(32))


def _biases(c, rng):
    b = c['bias']
    N = c['N']
    if 'list' in b:
        return np.resize(np.asarray(b['list'], dtype=float), N)
    mag = np.linspace(b['lo'], b['hi'], N)[rng.permutation(N)]
    if b['sign'] == 'alt':
        return mag * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    return mag if b['sign'] == '+' else -mag


def plant(S, c):
    nT = S.shape[0]
    for e in c['plant']:
        n = e['n']
        if not e.get('keep'):
            S[:, n] = 0
        for t, k in e.get('bins', ()):
            S[t, n] = k
        for i, ch in enumerate(e.get('chunks', ())):
            S[L * ch + (37 * i) % L, n] = 1
        if e.get('span'):
            S[3, n] = 1
            S[nT - 2, n] = 1
        if 'dense' in e:
            a, b = e['dense']
            S[a:b, n] = 1
            S[a:b:7, n] = 2


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = [c for c in load_cases() if c['name'] == name][0]
    kw = {} if c['w_scale'] is None else {'w_scale': c['w_scale']}
    p = H.Problem(c['N'], c['nT'], basis(), kind=c['kind'], rate_hz=c['rate_hz'], seed=c['seed'], weighted=True, **kw)
    plant(p.S, c)
    if c['bias'] is not None:
        p.theta[:, 0] = _biases(c, np.random.default_rng(500 + c['seed']))
    p._fS = O.convolve_with_basis(p.S.astype(float), p.ibasis)
    p.S.setflags(write=False)
    p.theta.setflags(write=False)
    return p


def problem(c):
    """helpers.Problem of the case (built once, shared, S and theta read-only)"""
    return _problem(c['name'])


@functools.lru_cache(maxsize=None)
def _currents(name):
    p = _problem(name)
    N, B = p.N, p.B
    w = p.theta[:, 1:].reshape(N, N, B)                         # [post, pre, b]  (Dstim = 0)
    Wm = (p.Weff.T[:, :, None] * w).reshape(N, N * B).T         # [(pre, b), post]
    x = p.fS.reshape(p.nT, N * B).dot(Wm) + p.theta[:, 0][None, :]
    x.setflags(write=False)
    return x


def currents(c, t_lo=0, t_hi=None):
    """total currents (bins, N) of the case over [t_lo, t_hi), float64"""
    return _currents(c['name'])[t_lo:t_hi]


def rate_longdouble(x, kind):
    x = np.asarray(x, dtype=np.longdouble)
    if kind == 'exp':
        return np.exp(x)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def events(S, n, t_lo, t_hi):
    """event bins of neuron n relative to t_lo"""
    return np.flatnonzero(S[t_lo:t_hi, n])


@functools.lru_cache(maxsize=None)
def _reference(name, t_lo, t_hi):
    p = _problem(name)
    cum = np.cumsum(rate_longdouble(_currents(name)[t_lo:t_hi], p.kind), axis=0)
    taus, stats = [], np.zeros((p.N, 3))
    for n in range(p.N):
        ev = events(p.S, n, t_lo, t_hi)
        tau = np.asarray(p.dt * (cum[ev[1:], n] - cum[ev[:-1], n]), dtype=np.float64) if ev.size > 1 else np.zeros(0)
        tau.setflags(write=False)
        taus.append(tau)
        stats[n] = (float(p.dt * cum[-1, n]), ev.size, int(np.sum(p.S[t_lo:t_hi, n] > 1)))
    stats.setflags(write=False)
    return tuple(taus), stats


def reference(c, t_lo, t_hi):
    """(taus per neuron, stats (N, 3): Lambda, events, multi-spike bins) over [t_lo, t_hi); computed once, read-only"""
    return _reference(c['name'], t_lo, t_hi)


def offsets(taus):
    return np.concatenate(([0], np.cumsum([t.size for t in taus]))).astype(np.int64)


def ratios(tau, off, lam, ref):
    """(worst |dtau| / (1e-10 tau_ref + 1e-12 Lambda_ref), worst |dLambda| / ((1e-10 + 1e-12) Lambda_ref)); a value that
    is not finite counts as infinitely far."""
    taus_ref, stats_ref = ref
    wt = 0.0
    for n, tr in enumerate(taus_ref):
        if tr.size:
            d = np.abs(tau[off[n]:off[n + 1]] - tr) / (REL * tr + ABS_LAMBDA * stats_ref[n, 0])
            wt = max(wt, float(np.max(np.where(np.isfinite(d), d, np.inf))))
    dl = np.abs(lam - stats_ref[:, 0]) / ((REL + ABS_LAMBDA) * stats_ref[:, 0])
    return wt, float(np.max(np.where(np.isfinite(dl), dl, np.inf)))


# ---- the geometry the kernels derive from a range ------------------------------------------------------------------------
def geometry(t_lo, t_hi):
    """(nchunks, per, live segments, bins of the last chunk)"""
    n = t_hi - t_lo
    nchunks = -(-n // L)
    per = -(-nchunks // SEGS)
    return nchunks, per, -(-nchunks // per), n - (nchunks - 1) * L


def xs_of(N):
    """row stride of the current slab: 16 doubles per post tile"""
    return 16 * ((N + 15) // 16)


# ---- numpy mirror of k_rescale_chunk / _scan / _finish in float64, with switchable faults ---------------------------------
def mirror(c, t_lo, t_hi, fault=None):
    """(tau concatenated, offsets, Lambda (N)) by the kernels' decomposition on the float64 rates O.nlin(x):
      chunk   per 256-bin chunk the running sum in time order, its value at every event bin (pre) and the chunk total (tot);
      scan    64 segments of `per` consecutive chunks, each summed in order, the segment sums scanned in order, the exclusive
              prefix of every chunk written back from its segment's start (cum; row nchunks = the total);
      finish  ca == cb: pre_b - pre_a;  else tot[ca] - pre_a (+ cum[cb] - cum[ca + 1] if cb > ca + 1) + pre_b.
    Faults: 'no_cum' drops the cum term; 'scan_late' starts the write-back of a segment one chunk late (its running sum
    skips the segment's first total); 'no_tail_mask' adds the rate at the bare bias for the rows between the end of the
    range and the next multiple of 8; 'stride_once' leaves every event past a neuron's first 256 unwritten (NaN)."""
    assert fault is None or fault in FAULTS
    p = problem(c)
    N, dt = p.N, p.dt
    nchunks, per, _, last = geometry(t_lo, t_hi)
    lam = np.zeros((nchunks * L, N))
    lam[:t_hi - t_lo] = O.nlin(currents(c, t_lo, t_hi), p.kind)
    if fault == 'no_tail_mask':
        pad = (-last) % UNROLL
        lam[t_hi - t_lo:t_hi - t_lo + pad] = O.nlin(p.theta[:, 0], p.kind)[None, :]
    run = np.cumsum(lam.reshape(nchunks, L, N), axis=1)          # (numpy's cumsum adds in order; + 0.0 past the end is exact)
    tot = run[:, -1, :]
    seg = np.zeros((SEGS, N))
    for s in range(SEGS):
        for ch in range(min(s * per, nchunks), min(s * per + per, nchunks)):
            seg[s] += tot[ch]
    start, acc = np.zeros((SEGS, N)), np.zeros(N)
    for s in range(SEGS):
        start[s] = acc
        acc = acc + seg[s]
    cum = np.zeros((nchunks + 1, N))
    for s in range(SEGS):
        c0, c1 = min(s * per, nchunks), min(s * per + per, nchunks)
        r = start[s].copy()
        for ch in range(c0, c1):
            cum[ch] = r
            if not (fault == 'scan_late' and ch == c0):
                r = r + tot[ch]
        if s == SEGS - 1:
            cum[nchunks] = r
    taus = []
    for n in range(N):
        ev = events(p.S, n, t_lo, t_hi)
        if ev.size < 2:
            taus.append(np.zeros(0))
            continue
        ch, pre = ev // L, run[ev // L, ev % L, n]
        ca, cb, pa, pb = ch[:-1], ch[1:], pre[:-1], pre[1:]
        far = cb > ca + 1
        s = tot[ca, n] - pa
        if fault != 'no_cum':
            s = s + np.where(far, cum[cb, n] - cum[np.minimum(ca + 1, nchunks), n], 0.0)
        s = np.where(ca == cb, pb - pa, s + pb)
        if fault == 'stride_once':
            s[STRIDE - 1:] = np.nan                             # interval i belongs to event i + 1: events 256 .. unwritten
        taus.append(dt * s)
    return np.concatenate(taus) if taus else np.zeros(0), offsets(taus), dt * cum[nchunks]
