"""Rank-normalised split-R-hat, bulk / tail / mean ESS and MCSE of one column of draws in np.longdouble, written from Vehtari,
Gelman, Simpson, Carpenter & Buerkner (2021) (eqs. 1-4, 10, 14; section 3.2 and the rule of Stan / the posterior package it
describes) and independently of theano_pyglm_amd/inference/diagnostics.py: a sort for the order statistics and the ranks,
scipy.special.ndtri for Phi^-1, every sum in longdouble, the whole rho sequence computed before Geyer's rule walks it.  Beside
it: the case table of the sweep, built in code; the smallest margin of every decision a case hangs on; the host mirror of
csrc/pglm_diag.h through ctypes; the error measures and the bounds the host mirror and the device are held to.

Decisions made on the float64 inputs (ranks, ties, the fold |x - median| with the float64 median) are exact facts of the
input, the same here as in every float64 implementation; everything after is extended precision."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
from scipy.special import ndtri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MAX_DRAWS = 4096                    # PGL_DIAG_MAX_DRAWS (test_diag_host checks it against the headers)
ROWS = ('mean', 'sd', 'median', 'q025', 'q975', 'rhat_plain', 'rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean',
        'lag_bulk', 'lag_q05', 'lag_q95', 'lag_mean')
LAGS = ROWS[11:]
MARGIN_FLOOR = 1e-9                 # a case counts only if no decision is closer to its threshold than this


def ranks64(v):
    """average ranks of the float64 values v: #{smaller} + (#{equal} + 1) / 2, from a sort"""
    v = np.asarray(v, dtype=np.float64)
    sv = np.sort(v)
    lo = np.searchsorted(sv, v, side='left')
    hi = np.searchsorted(sv, v, side='right')
    return lo + (hi - lo + 1) / 2.0


def scores(r, S):
    """Phi^-1((r - 3/8) / (S + 1/4)), the tail probability formed in longdouble and on the nearer side"""
    r = np.asarray(r, dtype=LD)
    lower = r <= LD(S + 1) / 2
    p = np.where(lower, (r - LD(0.375)) / (LD(S) + LD(0.25)), (LD(S) - r + LD(0.625)) / (LD(S) + LD(0.25)))
    z = ndtri(p.astype(np.float64)).astype(LD)
    return np.where(lower, z, -z)


def quantile_ld(sv, a, b):
    S = len(sv)
    k, rem = divmod(a * (S - 1), b)
    lo, hi = LD(sv[k]), LD(sv[min(k + 1, S - 1)])
    return lo + (hi - lo) * (LD(rem) / LD(b))


def quantile64(sv, a, b):
    """the float64 value of the rule (numpy's lerp): what the fold subtracts"""
    S = len(sv)
    k, rem = divmod(a * (S - 1), b)
    lo, hi = sv[k], sv[min(k + 1, S - 1)]
    g = rem / float(b)
    return lo + (hi - lo) * g if g < 0.5 else hi - (hi - lo) * (1.0 - g)


def halves(y, drop_middle=True):
    """(C, n) -> (2 C, h)"""
    Cn, n = y.shape
    h = n // 2
    out = []
    for c in range(Cn):
        out.append(y[c, :h])
        out.append(y[c, n - h:] if drop_middle else y[c, h:h + h])
    return np.array(out, dtype=LD)


def series_ld(y, margins, defect=None):
    """(rhat, ess, lag) of the series y (C, n) in longdouble; margins collects the distance of every discontinuous decision
    from its threshold: |P_t| at every step of the initial positive sequence, |rho_T| where the final odd term hangs on it"""
    sp = halves(np.asarray(y, dtype=LD), drop_middle=defect != 'keep_middle')
    m, h = sp.shape
    mean = sp.sum(axis=1) / LD(h)
    yc = sp - mean[:, None]
    stop = 1 if defect == 'lag_short' else 0                 # (the defect: the sum over the draws stops one short of h)
    am = np.empty(h, dtype=LD)
    for t in range(h):
        k = h - t - (stop if t else 0)
        am[t] = np.sum(np.sum(yc[:, :k] * yc[:, t:t + k], axis=1) / LD(h)) / LD(m)
    W = am[0] * LD(h) / LD(h - 1)
    gm = mean.sum() / LD(m)
    bh = np.sum((mean - gm) ** 2) / LD(m - 1)
    vp = W * LD(h - 1) / LD(h) + bh
    with np.errstate(all='ignore'):
        rhat = np.sqrt(vp / W)
    if not vp > 0:
        return rhat, LD(0), 0
    rho = LD(1) - (W - am) / vp
    rho[0] = LD(1)
    t = 0
    while t < h - 5 and rho[t] + rho[t + 1] > 0:
        margins.append(float(abs(rho[t] + rho[t + 1])))
        t += 2
    T = t
    margins.append(float(abs(rho[T] + rho[T + 1])))          # (the stop, and the final odd term's first condition)
    if not rho[T] + rho[T + 1] >= 0:
        margins.append(float(abs(rho[T])))
    r = rho.copy()
    last = r[T] if (r[T] + r[T + 1] >= 0 or r[T] > 0) else LD(0)
    if defect != 'no_monotone':
        for t in range(2, T - 1, 2):                         # (a minimum: continuous across its decision, so no margin is kept;
            if r[t] + r[t + 1] > r[t - 2] + r[t - 1]:
                r[t] = r[t + 1] = (r[t - 2] + r[t - 1]) / LD(2)  # sparse indicators tie here exactly, harmlessly)
    N = LD(m * h)
    tau = LD(-1) + LD(2) * (np.sum(r[:T]) if T > 0 else last) + last
    tau = max(tau, LD(1) / np.log10(N))
    return rhat, N / tau, T


def column_ld(x, defect=None):
    """({row: value}, smallest margin) of one column x (C, n) of float64 draws"""
    x = np.asarray(x, dtype=np.float64)
    Cn, n = x.shape
    S = Cn * n
    nan = LD(np.nan)
    if not np.all(np.isfinite(x)):
        return dict((k, nan) for k in ROWS), np.inf
    p = x.reshape(S)
    if p.max() == p.min():
        out = dict((k, LD(0)) for k in ROWS)
        out.update(mean=LD(p[0]), median=LD(p[0]), q025=LD(p[0]), q975=LD(p[0]), rhat_plain=nan, rhat=nan, mcse_mean=nan)
        return out, np.inf
    margins = []
    pl = p.astype(LD)
    mean = pl.sum() / LD(S)
    sd = np.sqrt(np.sum((pl - mean) ** 2) / LD(S - 1))
    sv = np.sort(p)
    q025, q05, med, q95, q975 = [quantile_ld(sv, a, b) for a, b in ((1, 40), (1, 20), (1, 2), (19, 20), (39, 40))]
    if defect == 'no_tie_average':
        r = (np.argsort(np.argsort(p, kind='stable'), kind='stable') + 1).astype(float)
    else:
        r = ranks64(p)
    z = scores(r, S).reshape(Cn, n)
    med64 = quantile64(sv, 1, 2)
    zf = scores(ranks64(np.abs(p - med64)), S).reshape(Cn, n)
    for q in (q05, q95):                                     # the indicators' decisions: x against the quantile
        d = np.abs(pl - q)
        d = d[pl != q]
        if d.size:
            margins.append(float(d.min() / max(1.0, float(abs(q)))))
    rb, eb, lb = series_ld(z, margins, defect)
    rf, _, _ = series_ld(zf, [], defect)
    _, e05, l05 = series_ld((pl <= q05).astype(LD).reshape(Cn, n), margins, defect)
    _, e95, l95 = series_ld((pl <= q95).astype(LD).reshape(Cn, n), margins, defect)
    rp, em, lm = series_ld(pl.reshape(Cn, n), margins, defect)
    with np.errstate(all='ignore'):
        out = {'mean': mean, 'sd': sd, 'median': med, 'q025': q025, 'q975': q975, 'rhat_plain': rp,
               'rhat': rf if (rf > rb or np.isnan(rb)) else rb, 'ess_bulk': eb, 'ess_tail': min(e05, e95), 'ess_mean': em,
               'mcse_mean': sd / np.sqrt(em), 'lag_bulk': LD(lb), 'lag_q05': LD(l05), 'lag_q95': LD(l95), 'lag_mean': LD(lm)}
    return out, (min(margins) if margins else np.inf)


def reference(x, defect=None):
    """(out (15, K) longdouble, smallest margin) of the float64 draws x (C, n, K); defect 'swap_strides' reads x as (n, C, K)"""
    x = np.asarray(x, dtype=np.float64)
    if defect == 'swap_strides':
        x = np.ascontiguousarray(x.reshape(x.shape[1], x.shape[0], x.shape[2]).transpose(1, 0, 2))
    K = x.shape[2]
    out = np.empty((len(ROWS), K), dtype=LD)
    margin = np.inf
    for k in range(K):
        col, mg = column_ld(x[:, :, k], defect)
        margin = min(margin, mg)
        for i, name in enumerate(ROWS):
            out[i, k] = col[name]
    return out, margin


# ---- the case table ----------------------------------------------------------------------------------------------------
def _ar1(rng, rho, C_, n, K, scale=1.0):
    e = rng.normal(0.0, 1.0, (C_, n, K))
    y = np.empty((C_, n, K))
    y[:, 0] = e[:, 0]
    for i in range(1, n):
        y[:, i] = rho * y[:, i - 1] + np.sqrt(1.0 - rho * rho) * e[:, i]
    return scale * y


def _content(kind, C_, n, K, rng):
    if kind == 'normal':
        return rng.normal(0.0, 1.0, (C_, n, K))
    if kind.startswith('ar'):
        return 3.0 + _ar1(rng, {'ar50': 0.5, 'ar99': 0.99, 'arm90': -0.9}[kind], C_, n, K)
    if kind == 'shifted':                                    # chains with different means: rhat >> 1
        return rng.normal(0.0, 1.0, (C_, n, K)) + 3.0 * np.arange(C_)[:, None, None]
    if kind == 'wide_chain':                                 # one chain with a larger variance: folded above bulk
        y = rng.normal(0.0, 1.0, (C_, n, K))
        y[0] *= 4.0
        return y
    if kind == 'integers':
        return np.round(_ar1(rng, 0.5, C_, n, K, 3.0))
    if kind == 'two_valued':
        return (_ar1(rng, 0.5, C_, n, K) > 0.8).astype(float)
    if kind == 'constant':
        return np.full((C_, n, K), 2.75)
    if kind == 'const_in_halves':                            # W = 0, B > 0
        h = n // 2
        y = np.empty((C_, n, K))
        for c in range(C_):
            y[c, :h] = 2.0 * c + 1.0
            y[c, h:] = 2.0 * c + 2.0
        return y + np.arange(K)[None, None, :]
    if kind == 'nonfinite':                                  # column k: one bad value at the first / a middle / the last draw
        y = rng.normal(0.0, 1.0, (C_, n, K))
        bad = (np.inf, -np.inf, np.nan)
        pos = ((0, 0), (C_ // 2, n // 2), (C_ - 1, n - 1))
        for k in range(K):
            if k % 4 != 3:                                   # (every fourth column stays clean)
                c, i = pos[(k // 4) % 3]
                y[c, i, k] = bad[k % 4]
        return y
    raise ValueError(kind)


def _cases():
    out = []

    def add(name, kind, C_, n, K=3):
        out.append({'name': name, 'kind': kind, 'C': C_, 'n': n, 'K': K})
    for n in (8, 9, 15, 16, 511, 512, 513, 1000):           # h = 4, 4, 7, 8, 255, 256, 256, 500
        add('n%d' % n, 'ar50', 2, n)
    for C_ in (1, 3, 4, 8):
        add('C%d' % C_, 'normal', C_, 64)
    add('S255', 'normal', 1, 255)
    add('S256', 'ar50', 1, 256)
    add('S257', 'normal', 1, 257)
    add('S1023', 'ar50', 3, 341)
    add('S1024', 'normal', 4, 256)
    add('S1025', 'ar50', 1, 1025)
    add('Smax', 'ar50', 4, MAX_DRAWS // 4, K=1)
    add('h257', 'normal', 1, 514)                            # (h = 255 and 256 are n511 and n512)
    add('K1', 'ar50', 2, 100, K=1)
    add('K161', 'ar50', 2, 40, K=161)
    add('normal', 'normal', 4, 200)
    add('ar50', 'ar50', 4, 200)
    add('ar99', 'ar99', 4, 400)
    add('arm90', 'arm90', 4, 200)
    add('shifted', 'shifted', 4, 100)
    add('wide_chain', 'wide_chain', 4, 200)
    add('integers', 'integers', 4, 100)
    add('two_valued', 'two_valued', 4, 100)
    add('constant', 'constant', 2, 20)
    add('const_in_halves', 'const_in_halves', 2, 20)
    add('nonfinite', 'nonfinite', 2, 21, K=12)
    return out


CASES = _cases()


def draws(case):
    """(C, n, K) float64"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case['name']))
    return np.ascontiguousarray(_content(case['kind'], case['C'], case['n'], case['K'], np.random.default_rng(seed)))


def device_layout(x, pad=0, fill=np.nan):
    """(C, n, K) -> the samplers' (n, C, ld) with ld = K + pad, the padding filled"""
    Cn, n, K = x.shape
    a = np.full((n, Cn, K + pad), fill)
    a[:, :, :K] = x.transpose(1, 0, 2)
    return a


_REF = {}


def case_reference(case):
    """(x (C, n, K), out (15, K) longdouble, margin): computed once per case and shared; callers must not write into them"""
    if case['name'] not in _REF:
        x = draws(case)
        out, margin = reference(x)
        for a in (x, out):
            a.setflags(write=False)
        _REF[case['name']] = (x, out, margin)
    return _REF[case['name']]


# ---- error measures and the bounds --------------------------------------------------------------------------------------
SUMS = ('mean', 'sd', 'median', 'q025', 'q975')             # fixed-order sums and two-term interpolations
COMPOSED = ('rhat_plain', 'rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean')


def errors_cols(out, ref):
    """{row: the relative difference per column} for the SUMS and COMPOSED rows; 0 where both sides are the same NaN, infinity
    or zero, inf where one side is finite / NaN / inf / zero and the other is not the same, and inf in every row of a column
    whose truncation lags differ"""
    out = np.asarray(out, dtype=LD)
    ref = np.asarray(ref, dtype=LD)
    lags_ok = np.all((out[11:] == ref[11:]) | (np.isnan(out[11:]) & np.isnan(ref[11:])), axis=0)
    e = {}
    for i, name in enumerate(ROWS[:11]):
        a, b = out[i], ref[i]
        same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))) | ((a == 0) & (b == 0))
        fin = np.isfinite(a) & np.isfinite(b) & ~same
        d = np.where(same, LD(0), LD(np.inf))
        with np.errstate(all='ignore'):
            d = np.where(fin, np.abs(a - b) / np.abs(b), d)
        e[name] = np.where(lags_ok, d, LD(np.inf)).astype(float)
    return e


def errors(out, ref):
    """{row: the worst of errors_cols over the columns}"""
    return dict((k, float(v.max())) for k, v in errors_cols(out, ref).items())


def sum_bounds_cols(x):
    """The derived bound of a fixed-order sum, 8 n 2^-53 sum |terms|, relative to the result, per column, for the rows of SUMS:
      mean      S terms x_s:  8 S u sum |x| / |mean|;
      sd        the S squares (x_s - mean)^2, all positive, so sum |terms| is the result: 8 S u on the sum, and the same on the
                sd, whose square root halves it and leaves room for the root, the division and the subtractions' own roundings;
                the computed mean's error d enters as S d^2, second order (sum (x - mean) = 0);
      quantiles two terms, the order statistics x_(k) and x_(k+1):  16 u (|x_(k)| + |x_(k+1)|) / |Q|; where Q = 0 the bound is 0
                (errors_cols gives 0 there only for an exact zero).
    Columns holding a non-finite draw and constant columns (their outputs are exact) get 0."""
    Cn, n, K = x.shape
    S = Cn * n
    p64 = x.reshape(S, K)
    u = LD(2.0) ** -53
    out = dict((k, np.zeros(K)) for k in SUMS)
    for k in range(K):
        col = p64[:, k]
        if not np.all(np.isfinite(col)) or col.max() == col.min():
            continue
        pl = col.astype(LD)
        mean = pl.sum() / S
        with np.errstate(all='ignore'):
            out['mean'][k] = float(8 * S * u * np.abs(pl).sum() / abs(mean)) if mean != 0 else 0.0
        out['sd'][k] = float(8 * S * u)
        sv = np.sort(col)
        for name, (a, b) in (('median', (1, 2)), ('q025', (1, 40)), ('q975', (39, 40))):
            q = quantile_ld(sv, a, b)
            i = a * (S - 1) // b
            out[name][k] = float(16 * u * (abs(LD(sv[i])) + abs(LD(sv[min(i + 1, S - 1)]))) / abs(q)) if q != 0 else 0.0
    return out


# e0: the worst relative difference of the float64 numpy statement (inference/diagnostics.chain_diagnostics) from the
# longdouble reference over the whole case table, per composed row, as test_diag_host.test_error_scale measures and checks it
# (recorded 2026-10-20).  The bound for the host mirror and for the device is 100 e0 per row: both differ from the numpy
# statement in a different but fixed summation order and in the exp / log of another library inside Phi^-1.
E0 = {'rhat_plain': 2.9e-16, 'rhat': 2.6e-16, 'ess_bulk': 5.5e-15, 'ess_tail': 5.7e-15, 'ess_mean': 5.6e-15, 'mcse_mean': 2.6e-15}
BOUND = dict((q, 100.0 * E0[q]) for q in COMPOSED)


def ratios(out, ref, x):
    """{row: the worst ratio over the columns of the error to its bound}: the COMPOSED rows against BOUND, the SUMS rows against
    sum_bounds_cols column by column (0 where error and bound are both 0, inf where only the bound is)"""
    e = errors_cols(out, ref)
    sb = sum_bounds_cols(x)
    r = dict((q, float(e[q].max() / BOUND[q])) for q in COMPOSED)
    for q in SUMS:
        with np.errstate(all='ignore'):
            v = np.where(e[q] == 0, 0.0, np.where(sb[q] > 0, e[q] / np.where(sb[q] > 0, sb[q], 1.0), np.inf))
        r[q] = float(v.max())
    return r


def within(out, ref, x):
    return all(v <= 1.0 for v in ratios(out, ref, x).values())


# ---- host mirror (csrc/pglm_diag.h through tests/csrc/diag_host.c) ------------------------------------------------------
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='diag_host_'), 'diag_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'diag_host.c'), '-lm'])
        Lb = C.CDLL(so)
        Lb.diag_run.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]
        Lb.diag_score.argtypes = [C.c_double, C.c_double]
        Lb.diag_score.restype = C.c_double
        Lb.diag_max_draws.restype = C.c_longlong
        _LIB = Lb
    return _LIB


def host_mirror(x, pad=0):
    """out (15, K) of the host build of the rule on x (C, n, K), through the samplers' layout"""
    Cn, n, K = x.shape
    a = device_layout(x, pad)
    out = np.full((len(ROWS), K), 12345.678)
    assert lib().diag_run(a.ctypes.data, n, Cn, K, K + pad, out.ctypes.data) == 0
    return out
