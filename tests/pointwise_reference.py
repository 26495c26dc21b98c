"""The case table of the pointwise log-likelihood sweep (tests/pointwise_cases.json), its reference, a numpy mirror of the
kernels' chunk -> block decomposition and the host mirror of the accumulation over draws (test infrastructure, no GPU):
tests/test_pointwise_host.py keeps the table honest on the CPU, tests/test_gpu_pointwise.py runs it on the device.

Reference, independent of the device: currents from the oracle's features as in tests/rescale_reference.py (a direct
time-domain convolution of the spikes, one matrix product per case), the rate and its logarithm in numpy.longdouble --
exp(x) with log lam = x, or max(x, 0) + log1p(exp(-|x|)) with log of that --, the per-bin term
    term_t = -dt lam_t + S[t,n] log lam_t        (a bin with S = 0: -dt lam_t alone)
and its sums over the blocks in longdouble, the running sum restarted at every block.  Blocks: chunks of 256 bins counted from t_lo, block_chunks
consecutive chunks per block, the last block short.

Bound (the rescaling sweep's): |l_dev - l_ref| <= 1e-10 |l_ref| + 1e-12 A_b, A_b = sum_{t in b} (dt lam_t + S |log lam_t|):
the two parts of the term cancel, so the absolute sum is the scale of the summation error.

A case is a case of tests/rescale_cases.json (same fields, same builders) whose ranges carry "block_chunks": [...]; a plant
entry may also hold  dense3 [first, last): an event on every bin, two spikes on every seventh, three on every eleventh.

Draws for the accumulator test: theta plus a seeded jitter (draws), S = 33."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'pointwise_cases.json')
L, UNROLL = RR.L, RR.UNROLL
REL, ABS_A = 1e-10, 1e-12
FAULTS = ('no_tail_mask', 'drop_short_block', 'grid_from_zero')
N_DRAWS = 33
POISON_DRAW = 5
SPREAD = 1e-3                  # every block's sd over the draws is at least this fraction of its |mean|


def load_cases():
    with open(CASES) as f:
        cases = json.load(f)
    for c in cases:
        assert sorted(c) == sorted(RR.FIELDS), (c.get('name'), sorted(set(c) ^ set(RR.FIELDS)))
        for r in c['ranges']:
            assert sorted(r) == ['block_chunks', 'hits', 't'], (c['name'], r)
    return cases


def ranges(c):
    """[(t_lo, t_hi, block_chunks list, hits)] of a case; "t": null is the whole recording"""
    return [((0, c['nT']) if r['t'] is None else tuple(r['t'])) + (r['block_chunks'], r['hits']) for r in c['ranges']]


def plant(S, c):
    for e in c['plant']:
        RR.plant(S, {'plant': [dict((k, v) for k, v in e.items() if k != 'dense3')]})
        if 'dense3' in e:
            a, b = e['dense3']
            S[a:b, e['n']] = 1
            S[a:b:7, e['n']] = 2
            S[a:b:11, e['n']] = 3


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = [c for c in load_cases() if c['name'] == name][0]
    kw = {} if c['w_scale'] is None else {'w_scale': c['w_scale']}
    p = H.Problem(c['N'], c['nT'], RR.basis(), kind=c['kind'], rate_hz=c['rate_hz'], seed=c['seed'], weighted=True, **kw)
    plant(p.S, c)
    if c['bias'] is not None:
        p.theta[:, 0] = RR._biases(c, np.random.default_rng(500 + c['seed']))
    p._fS = O.convolve_with_basis(p.S.astype(float), p.ibasis)
    p.S.setflags(write=False)
    p.theta.setflags(write=False)
    return p


def problem(c):
    """helpers.Problem of the case (built once, shared, S and theta read-only)"""
    return _problem(c['name'])


def currents_of(p, theta):
    """total currents (nT, N) of the problem at the rows theta (N, P), float64"""
    N, B = p.N, p.B
    w = theta[:, 1:].reshape(N, N, B)                           # [post, pre, b]  (Dstim = 0)
    Wm = (p.Weff.T[:, :, None] * w).reshape(N, N * B).T         # [(pre, b), post]
    return p.fS.reshape(p.nT, N * B).dot(Wm) + theta[:, 0][None, :]


@functools.lru_cache(maxsize=None)
def _currents(name):
    p = _problem(name)
    x = currents_of(p, p.theta)
    x.setflags(write=False)
    return x


def currents(c, t_lo=0, t_hi=None):
    return _currents(c['name'])[t_lo:t_hi]


def terms_longdouble(x, S, kind, dt):
    """(term, absolute term) per bin in longdouble: -dt lam + S log lam and dt lam + S |log lam|"""
    lam = RR.rate_longdouble(x, kind)
    with np.errstate(divide='ignore'):
        loglam = np.asarray(x, dtype=np.longdouble) if kind == 'exp' else np.log(lam)
    Sl = S.astype(np.longdouble)
    spike = np.where(S > 0, Sl * np.where(S > 0, loglam, 0), 0)
    return -dt * lam + spike, dt * lam + np.abs(spike)


def geometry(t_lo, t_hi, bc):
    """(nchunks, n_blocks, bins of the last chunk)"""
    n = t_hi - t_lo
    nchunks = -(-n // L)
    return nchunks, -(-nchunks // bc), n - (nchunks - 1) * L


def block_sums(a, bc):
    """sums of the rows of a (bins, N) over blocks of bc * 256 rows, in a's type: the cumulative sum restarts at every block
    (a difference of two long prefixes would lose a block that is tiny next to the ones before it)"""
    n = a.shape[0]
    nchunks = -(-n // L)
    starts = np.arange(0, nchunks, bc) * L
    return np.add.reduceat(a, starts, axis=0)


@functools.lru_cache(maxsize=None)
def _reference(name, t_lo, t_hi, bc):
    p = _problem(name)
    term, aterm = terms_longdouble(_currents(name)[t_lo:t_hi], p.S[t_lo:t_hi], p.kind, p.dt)
    ll = np.asarray(block_sums(term, bc), dtype=np.float64)
    A = np.asarray(block_sums(aterm, bc), dtype=np.float64)
    ll.setflags(write=False)
    A.setflags(write=False)
    return ll, A


def reference(c, t_lo, t_hi, bc):
    """(ll_blk (n_blocks, N), A (n_blocks, N)) over [t_lo, t_hi) in blocks of bc chunks; computed once, read-only"""
    return _reference(c['name'], t_lo, t_hi, bc)


def ratio(ll, ref):
    """worst |l - l_ref| / (1e-10 |l_ref| + 1e-12 A_b); a value that is not finite, or a shape that differs, counts as
    infinitely far"""
    ll_ref, A = ref
    if ll.shape != ll_ref.shape:
        return np.inf
    d = np.abs(ll - ll_ref) / (REL * np.abs(ll_ref) + ABS_A * A)
    return float(np.max(np.where(np.isfinite(d), d, np.inf)))


# ---- numpy mirror of k_pw_chunk / k_pw_block in float64, with switchable faults ---------------------------------------------
def mirror(c, t_lo, t_hi, bc, fault=None):
    """ll_blk (n_blocks, N) by the kernels' decomposition on float64 terms: per 256-bin chunk from t_lo the sum in time order,
    per block its chunks' sums in chunk order.  Faults: 'no_tail_mask' adds the term at the bare bias for the rows between
    the end of the range and the next multiple of 8; 'drop_short_block' never writes a last block of fewer than bc chunks
    (NaN); 'grid_from_zero' cuts the chunks on the grid that starts at bin 0 instead of t_lo."""
    assert fault is None or fault in FAULTS
    p = problem(c)
    N, dt = p.N, p.dt
    nchunks, n_blocks, last = geometry(t_lo, t_hi, bc)
    x, S = currents(c, t_lo, t_hi), p.S[t_lo:t_hi]
    lam = O.nlin(x, p.kind)
    with np.errstate(divide='ignore'):
        loglam = x if p.kind == 'exp' else np.log(lam)
    term = -dt * lam + np.where(S > 0, S * np.where(S > 0, loglam, 0.0), 0.0)
    n = t_hi - t_lo
    lead = (t_lo % L) if fault == 'grid_from_zero' else 0        # bins of the first chunk that lie before t_lo
    nch = -(-(lead + n) // L)
    full = np.zeros((nch * L, N))                                # (+ 0.0 past the end is exact)
    full[lead:lead + n] = term
    if fault == 'no_tail_mask':
        full[n:n + (-last) % UNROLL] = -dt * O.nlin(p.theta[:, 0], p.kind)[None, :]
    part = np.cumsum(full.reshape(nch, L, N), axis=1)[:, -1, :]
    out = np.full((n_blocks, N), np.nan)
    for b in range(n_blocks):
        c0, c1 = b * bc, min(b * bc + bc, nch)
        if (fault == 'drop_short_block' and b * bc + bc > nchunks) or c0 >= nch:
            continue
        acc = np.zeros(N)
        for ch in range(c0, c1):
            acc = acc + part[ch]
        out[b] = acc
    return out


# ---- the draws of the accumulator test -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _draws(name):
    p = _problem(name)
    rng = np.random.default_rng(9000 + p.N + p.nT)
    th = np.repeat(p.theta[None], N_DRAWS, axis=0)
    z = rng.standard_normal(th.shape)
    th[:, :, 0] += 0.1 * np.maximum(1.0, np.abs(p.theta[None, :, 0])) * z[:, :, 0]
    th[:, :, 1:] += 0.05 * np.maximum(np.abs(p.theta[None, :, 1:]), 0.05) * z[:, :, 1:]
    th.setflags(write=False)
    return th


def draws(c):
    """(33, N, P) parameter rows: theta plus a seeded jitter of 10 % of max(1, |bias|) on the bias and 5 % on the weights"""
    return _draws(c['name'])


def poisoned(c):
    """(draw, neuron) whose bias is NaN in the accumulator test: flat index 1 of the (block, neuron) grid, neuron 1 (the only
    neuron where N = 1)"""
    return POISON_DRAW, min(1, c['N'] - 1)


def draw_blocks(c, t_lo, t_hi, bc):
    """float64 block sums (33, n_blocks, N) of the draws by the reference's definition (for the spread condition)"""
    p = problem(c)
    out = []
    for th in draws(c):
        term, _ = terms_longdouble(currents_of(p, th)[t_lo:t_hi], p.S[t_lo:t_hi], p.kind, p.dt)
        out.append(np.asarray(block_sums(term, bc), dtype=np.float64))
    return np.array(out)


# ---- host mirror of the accumulation (csrc/pglm_pointwise.h through tests/csrc/pointwise_host.c) ---------------------------
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='pointwise_host_'), 'pointwise_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so,
                               os.path.join(ROOT, 'tests', 'csrc', 'pointwise_host.c'), '-lm'])
        Lb = C.CDLL(so)
        Lb.pw_fold.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
        Lb.pw_run.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
        _LIB = Lb
    return _LIB


def host_accumulate(ll, garbage=True):
    """the state (4,) + ll.shape[1:] after folding the draws ll (S, ...) in order with the host build of the rule; the
    state starts as NaN-free garbage (draw 0 must initialise it)"""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    S, n = ll.shape[0], int(np.prod(ll.shape[1:]))
    acc = np.full((4, n), 12345.678 if garbage else 0.0)
    lib().pw_run(ll.ctypes.data, S, n, acc.ctypes.data)
    return acc.reshape((4,) + ll.shape[1:])


def accumulate_longdouble(ll):
    """(lse = log sum_s exp(l_s), mean, M2) of ll (S, ...) in longdouble, two passes; NaN where a draw is not finite"""
    a = np.asarray(ll, dtype=np.longdouble)
    bad = ~np.all(np.isfinite(a), axis=0)
    a = np.where(bad[None], 0, a)
    m = a.max(axis=0)
    lse = np.log(np.sum(np.exp(a - m[None]), axis=0)) + m
    mean = a.mean(axis=0)
    m2 = np.sum((a - mean[None]) ** 2, axis=0)
    nan = lambda v: np.where(bad, np.nan, v)
    return nan(lse), nan(mean), nan(m2)
