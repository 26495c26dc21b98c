"""What the filter-band tests share: the case table tests/filter_cases.json with its generator, a numpy.longdouble reference of
the rule of csrc/pglm_filters.h, the gcc build of the host mirror tests/csrc/filters_host.c and the comparison of bits.

The reference states the MATHEMATICS in longdouble (64-bit mantissa on x86) from the weights: h = basis w, its mean and sd
(S - 1) over the draws, the effective weight -- the order of a sum is below its precision.  The order statistics are taken by
numpy.partition from the float64 curves the statement itself forms (curves(): one expression, nothing to get wrong twice).

Bounds of mean / sd / weight.  The error of the numpy statement against longdouble is MEASURED per case (measure(), run by
`python tests/filter_reference.py`) in these units, A = mean_s sum_b |basis_b w_sb| the size of the terms:
    mean, weight_mean:  |err| / (u A);          sd, weight_sd:  |err| / (u (sd + A^2 / sd))   (the cancellation of the deviations)
and stored in the JSON as 'measured': [mean, sd]; the test allows max(4 x measured, 4) -- the margin covers another numpy
build; the device is held to the statement's bits, never to this bound.  Where sd_ref = 0 (all draws equal) the sd is the
rounding error of the mean, held to the bound of its serial sums, 2 (256 + S / 256 + 1) u A (0 exactly where the sums are exact: the 'const_group' lags, a zero basis row), and
the 'wide' case (squares that overflow or underflow float64) is checked for its bits and order statistics only."""
import ctypes
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -53
DT = 0.001

_table = None
_lib = None
_made = {}


def table():
    global _table
    if _table is None:
        with open(os.path.join(ROOT, 'tests', 'filter_cases.json')) as f:
            _table = json.load(f)
    return _table


def load():
    return table()['cases']


def make_case(c):
    """-> dict(x (n, C M, P) in the samplers' layout, basis (R, B), c (B,), P) of a case of the table (made once, read-only).
    'ties': every odd draw repeats the draw before it; 'const_group': [m, g] holds 1.0 in every draw and the basis is rounded to
    eighths (every sum is exact: sd = 0 at every lag); 'zero_lag': that basis row is 0; 'nan' / 'inf': [m, g] has one such
    weight in one draw of one chain; 'wide': group g of every row is scaled by 1e-300, 1, 1e300 for g = 0, 1, 2."""
    if c['name'] in _made:
        return _made[c['name']]
    rng = np.random.default_rng(c['seed'])
    n, C, M, B, R, G, first = c['n'], c['C'], c['M'], c['B'], c['R'], c['G'], c['first']
    P = first + G * B + 2
    x = rng.normal(size=(n, C * M, P))
    basis = 0.5 * rng.normal(size=(R, B))
    if c.get('ties'):
        x[1::2] = x[0:2 * (n // 2):2]
    if 'const_group' in c:
        m, g = c['const_group']
        basis = np.round(basis * 8.0) / 8.0
        for ch in range(C):
            x[:, ch * M + m, first + g * B:first + (g + 1) * B] = 1.0
    if 'zero_lag' in c:
        basis[c['zero_lag']] = 0.0
    if c.get('wide'):
        for g in range(G):
            x[:, :, first + g * B:first + (g + 1) * B] *= (1e-300, 1.0, 1e300)[g % 3]
    if 'nan' in c:
        m, g = c['nan']
        x[0, m, first + g * B] = np.nan
    if 'inf' in c:
        m, g = c['inf']
        x[min(1, n - 1), (C - 1) * M + m, first + (g + 1) * B - 1] = np.inf
    d = {'x': x, 'basis': basis, 'c': DT * basis.sum(axis=0), 'P': P}
    for a in (x, basis, d['c']):
        a.setflags(write=False)
    _made[c['name']] = d
    return d


def args(c):
    d = make_case(c)
    return d['x'], c['C'], c['first'], c['G'], d['basis'], d['c'], c['level']


def pooled_group(c, m, g):
    """(S, B) weights of group g of row m, pooled s = chain n + draw"""
    d = make_case(c)
    n, C, M, B = c['n'], c['C'], c['M'], c['B']
    o = c['first'] + g * B
    return d['x'].reshape(n, C, M, -1).transpose(1, 0, 2, 3).reshape(C * n, M, -1)[:, m, o:o + B]


def bad_group(c, m, g):
    return c.get('nan') == [m, g] or c.get('inf') == [m, g]


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, 'tests', 'csrc', 'filters_host.so')
        srcs = [os.path.join(ROOT, 'tests', 'csrc', 'filters_host.c')] + \
            [os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', h) for h in ('pglm_filters.h', 'pglm_wald.h', 'pglm_hmc.h',
                                                                         'pglm_linesearch.h')]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, srcs[0], '-lm'])
        L = ctypes.CDLL(so)
        vp, ll = ctypes.c_void_p, ctypes.c_longlong
        L.filters_run.restype = None
        L.filters_run.argtypes = [vp, ll, ll, ll, ll, ll, ll, ctypes.c_int, vp, ll, vp, ctypes.c_double, vp, vp, vp]
        _lib = L
    return _lib


def host_bands(x, C, first, G, basis, c, level):
    """the gcc mirror: -> (out (M, G, R, 5), grp (M, G, 8))"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    n, M, P = x.shape[0], x.shape[1] // C, x.shape[2]
    R, B = basis.shape
    out, grp = np.empty((M, G, R, 5)), np.empty((M, G, 8))
    work = np.empty((B + 2) * n * C)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib().filters_run(p(x), n, C, M, P, first, G, B, p(basis), R, p(c), float(level), p(out), p(grp), p(work))
    return out, grp


def same_bits(a, b):
    """a and b hold NaN at the same places and the same bits everywhere else"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the longdouble reference -----------------------------------------------------------------------------------------------
def reference_group(w, basis, c):
    """longdouble mean and sd (R + 1,) of the curves and of the effective weight (the last entry), and A (R + 1,)"""
    rows = np.concatenate([basis, c[None]], axis=0).astype(LD)
    wl = w.astype(LD)
    S = w.shape[0]
    h = wl.dot(rows.T)                                        # (S, R + 1)
    A = np.abs(wl).dot(np.abs(rows).T).sum(axis=0) / S
    mean = h.sum(axis=0) / S
    sd = np.sqrt(((h - mean) ** 2).sum(axis=0) / (S - 1))
    return mean, sd, A


def error_ratios(out, grp, w, basis, c):
    """(largest mean ratio, largest sd ratio) of one group's outputs in the units of the module text; the bound of the lags
    with sd_ref = 0 is asserted here."""
    mean_r, sd_r, A = reference_group(w, basis, c)
    mean = np.concatenate([out[:, 0], grp[1:2]])
    sd = np.concatenate([out[:, 1], grp[2:3]])
    zero = sd_r == 0
    S = w.shape[0]                                            # (all draws equal: the sd is the error of the mean of S equal
    assert np.all(sd[zero] <= 2.0 * (256 + S // 256 + 1) * U * A[zero])   # terms, serial pieces of 256, times sqrt(S / (S - 1)))
    live = ~zero & (A > 0)
    rm = np.abs(mean.astype(LD) - mean_r)[A > 0] / (U * A[A > 0])
    rs = np.abs(sd.astype(LD) - sd_r)[live] / (U * (sd_r[live] + A[live] ** 2 / sd_r[live]))
    assert np.all(mean[A == 0] == 0.0)
    return float(rm.max()) if rm.size else 0.0, float(rs.max()) if rs.size else 0.0


def order_statistics(h, level):
    """q_lo, median, q_hi (K,) of the columns of h (S, K) by numpy.partition and the rule's interpolation, and
    k = ceil(level S)"""
    S = h.shape[0]
    qs = []
    for p in ((1.0 - level) / 2.0, 0.5, (1.0 + level) / 2.0):
        pos = p * float(S - 1)
        k = min(int(pos), S - 1)
        k1 = min(k + 1, S - 1)
        part = np.partition(h, sorted(set((k, k1))), axis=0)
        lo, hi, g = part[k] + 0.0, part[k1] + 0.0, pos - k
        qs.append(lo if g == 0.0 else (lo + (hi - lo) * g if g < 0.5 else hi - (hi - lo) * (1.0 - g)))
    t = level * float(S)
    k = int(t) + (int(t) < t)
    return qs, min(max(k, 1), S)


def ratios_d(h, out):
    """r (S, R) = |h - mean| / sd with the statement's outputs (NaN where sd is not > 0), and d (S,)"""
    with np.errstate(all='ignore'):
        r = np.abs(h - out[:, 0]) / out[:, 1]
        r[:, ~(out[:, 1] > 0.0)] = np.nan
        d = np.fmax.reduce(np.concatenate([np.zeros((h.shape[0], 1)), r], axis=1), axis=1)
    return r, d


def measure(c):
    """[mean, sd]: the numpy statement's largest error ratios over the groups of a case"""
    from theano_pyglm_amd.inference.filters import filter_bands_numpy
    d = make_case(c)
    out, grp = filter_bands_numpy(*args(c))
    best = [0.0, 0.0]
    for m in range(c['M']):
        for g in range(c['G']):
            if bad_group(c, m, g):
                continue
            r = error_ratios(out[m, g], grp[m, g], pooled_group(c, m, g), d['basis'], d['c'])
            best = [max(best[0], r[0]), max(best[1], r[1])]
    return best


if __name__ == '__main__':                                    # rewrite the measured ratios of the table
    import sys
    sys.path.insert(0, ROOT)
    t = table()
    for c in t['cases']:
        if not c.get('wide'):
            c['measured'] = [float('%.4g' % v) for v in measure(c)]
            print(c['name'], c['measured'])
    with open(os.path.join(ROOT, 'tests', 'filter_cases.json'), 'w') as f:
        f.write('{\n  "comment": %s,\n  "cases": [\n' % json.dumps(t['comment']))
        f.write(',\n'.join('    ' + json.dumps(c) for c in t['cases']))
        f.write('\n  ]\n}\n')
