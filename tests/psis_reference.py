"""PSIS-LOO of a column of pointwise log-likelihoods in np.longdouble, written from the papers (Vehtari, Gelman & Gabry 2017,
section 2.2 and appendix; Vehtari, Simpson, Gelman, Yao & Gabry 2024; Zhang & Stephens 2009, section 4 with the loo package's
prior) and independently of theano_pyglm_amd/inference/model_compare.py; the case table of the sweep, built in code (every
case names what it reaches; tests/test_psis_host.py proves it does); the host mirror of csrc/pglm_psis.h through ctypes; the
error measures and the bound the host mirror and the device are held to.

Ordering and tie decisions are made on the raw float64 inputs (the rule's step 2), so tail membership is the same exact
fact here as in every float64 implementation; everything after is extended precision."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
LOG_DBL_MIN = np.log(LD(np.finfo(np.float64).tiny))
MAX_DRAWS = 4096                    # PGL_PSIS_MAX_DRAWS (test_psis_host checks it against the header)


def tail_len(S):
    """ceil(min(S / 5, 3 sqrt(S))) in integers"""
    if 5 * 3 * 3 * 5 >= S:                                                  # S / 5 <= 3 sqrt(S)  <=>  S <= 225
        return -(-S // 5)
    m = int(np.sqrt(9.0 * S))
    while m * m < 9 * S:
        m += 1
    while (m - 1) * (m - 1) >= 9 * S:
        m -= 1
    return m


def gpd_fit_ld(e):
    """Zhang & Stephens' posterior-mean fit of the generalized Pareto law to ascending excesses e: (khat, sigma), longdouble"""
    e = np.asarray(e, dtype=LD)
    n = len(e)
    m = 30 + int(np.floor(np.sqrt(n)))
    quart = e[int(np.floor(n / 4 + 0.5)) - 1]
    theta = np.array([LD(1) / e[n - 1] + (LD(1) - np.sqrt(LD(m) / (LD(j) - LD(0.5)))) / (LD(3) * quart) for j in range(1, m + 1)])
    kk = np.array([np.sum(np.log1p(-t * e)) / LD(n) for t in theta])
    prof = LD(n) * (np.log(-theta / kk) - kk - LD(1))
    wt = np.array([LD(1) / np.sum(np.exp(prof - p)) for p in prof])
    keep = wt >= LD(10) * LD(np.finfo(np.float64).eps)
    wt = wt[keep] / np.sum(wt[keep])
    tb = np.sum(wt * theta[keep])
    k = np.sum(np.log1p(-tb * e)) / LD(n)
    return (LD(n) * k + LD(5)) / (LD(n) + LD(10)), -k / tb


def column_ld(l64):
    """(elpd, khat, n_eff, n, lw) of one float64 column in longdouble"""
    l64 = np.asarray(l64, dtype=np.float64)
    S = len(l64)
    if not np.all(np.isfinite(l64)):
        nan = LD(np.nan)
        return nan, nan, nan, nan, np.full(S, nan)
    order = np.lexsort((np.arange(S), -l64))                # ascending ratio; among equals the smaller draw index first
    l = l64.astype(LD)
    r = -l
    x = r - r.max()
    M = tail_len(S)
    cut = order[S - M - 1]
    xc = max(x[cut], LOG_DBL_MIN)
    tail = np.array([s for s in order if l64[s] < l64[cut]], dtype=int)
    n = len(tail)
    khat = LD(np.inf)
    with np.errstate(all='ignore'):
        if n >= 5:
            khat, sigma = gpd_fit_ld(np.exp(x[tail]) - np.exp(xc))
            if np.isfinite(khat):
                i = np.arange(1, n + 1).astype(LD)
                p = (i - LD(0.5)) / LD(n)
                if abs(khat) < LD(np.finfo(np.float64).eps):
                    q = -np.log1p(-p)
                else:
                    q = np.expm1(-khat * np.log1p(-p)) / khat
                x = x.copy()
                x[tail] = np.log(np.exp(xc) + sigma * q)
        x = np.minimum(x, LD(0))
        mx = x.max()
        lw = x - (mx + np.log(np.sum(np.exp(x - mx))))
        t = lw + l
        a = t.max()
        return a + np.log(np.sum(np.exp(t - a))), khat, LD(1) / np.sum(np.exp(2 * lw)), LD(n), lw


def reference(ll):
    """out (4, C) and lw (S, C), longdouble, of the float64 matrix ll (S, C)"""
    ll = np.asarray(ll, dtype=np.float64)
    S, ncol = ll.shape
    out = np.empty((4, ncol), dtype=LD)
    lw = np.empty((S, ncol), dtype=LD)
    for c in range(ncol):
        out[0, c], out[1, c], out[2, c], out[3, c], lw[:, c] = column_ld(ll[:, c])
    return out, lw


# ---- the case table ----------------------------------------------------------------------------------------------------
SIZES = (2, 24, 25, 26, 63, 64, 65, 100, 225, 226, 1000, 1024, 1025, MAX_DRAWS)


def _content(kind, S, ncol, rng):
    if kind == 'normal':
        return -40.0 + rng.normal(0.0, 1.0, (S, ncol))
    if kind == 'heavy':                                     # ratios exp(Cauchy), clipped: khat > 1
        return -40.0 - np.clip(rng.standard_cauchy((S, ncol)), -30.0, 30.0)
    if kind == 'bounded':                                   # ratios in [1, 2]: khat < 0
        return -40.0 - np.log1p(rng.uniform(0.0, 1.0, (S, ncol)))
    if kind == 'constant':
        return np.full((S, ncol), -37.25)
    if kind == 'ties_cutoff':                               # S = 100, M = 20: column 0 keeps 3 tail elements, 1 keeps 15, 2 keeps 5
        a = np.zeros((S, ncol))
        for c, n in enumerate((3, 15, 5)[:ncol]):
            idx = rng.permutation(S)[:n]
            a[idx, c] = -np.arange(1, n + 1) * 0.37 - rng.uniform(0.0, 0.1, n)
        return a - 12.0
    if kind == 'ties_tail':                                 # quarter steps: equal values inside the tail and at the cutoff
        return -40.0 + np.round(rng.normal(0.0, 1.0, (S, ncol)) * 4.0) / 4.0
    if kind == 'range1e4':                                  # x spans 10^4: the cutoff lies far below log(DBL_MIN)
        return -1.0e4 * rng.uniform(0.0, 1.0, (S, ncol))
    if kind == 'offset':
        return -1.0e6 + rng.normal(0.0, 1.0, (S, ncol))
    raise ValueError(kind)


def _cases():
    out = []
    for S in SIZES:
        out.append({'name': 'S%d' % S, 'S': S, 'C': 1 if S == MAX_DRAWS else 3, 'kind': 'normal',
                    'reach': {'M': tail_len(S), 'fit': tail_len(S) >= 5}})
    for ncol in (1, 65):
        out.append({'name': 'C%d' % ncol, 'S': 100, 'C': ncol, 'kind': 'normal', 'reach': {'M': 20, 'fit': True}})
    out.append({'name': 'heavy', 'S': 200, 'C': 3, 'kind': 'heavy', 'reach': {'khat_above': 1.0}})
    out.append({'name': 'bounded', 'S': 200, 'C': 3, 'kind': 'bounded', 'reach': {'khat_below': 0.0}})
    out.append({'name': 'constant', 'S': 100, 'C': 3, 'kind': 'constant', 'reach': {'n': [0, 0, 0], 'uniform': True}})
    out.append({'name': 'ties_cutoff', 'S': 100, 'C': 3, 'kind': 'ties_cutoff', 'reach': {'n': [3, 15, 5]}})
    out.append({'name': 'ties_tail', 'S': 200, 'C': 3, 'kind': 'ties_tail', 'reach': {'tied_tail': True}})
    out.append({'name': 'range1e4', 'S': 200, 'C': 3, 'kind': 'range1e4', 'reach': {'floor': True}})
    out.append({'name': 'offset', 'S': 200, 'C': 3, 'kind': 'offset', 'reach': {'fit': True}})
    return out


CASES = _cases()


def matrix(case):
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case['name']))
    return np.ascontiguousarray(_content(case['kind'], case['S'], case['C'], np.random.default_rng(seed)))


_REF = {}


def case_reference(case):
    """(ll, out, lw): computed once per case and shared; callers must not write into them"""
    if case['name'] not in _REF:
        ll = matrix(case)
        out, lw = reference(ll)
        for a in (ll, out, lw):
            a.setflags(write=False)
        _REF[case['name']] = (ll, out, lw)
    return _REF[case['name']]


# ---- error measures and the bound ---------------------------------------------------------------------------------------
QUANTITIES = ('elpd', 'khat', 'n_eff', 'lw')


def errors(out, lw, ref_out, ref_lw):
    """{'elpd': relative to max(1, |elpd|), 'khat': absolute, 'n_eff': relative, 'lw': absolute on the reference's entries above
    log(DBL_MIN)}, the worst over the columns; inf where one side is finite / NaN / inf and the other is not the same; the
    tail lengths must be equal (inf in every quantity otherwise)."""
    out = np.asarray(out, dtype=LD)
    ref_out = np.asarray(ref_out, dtype=LD)

    def dist(a, b, scale):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b)))
        fin = np.isfinite(a) & np.isfinite(b)
        d = np.where(same, LD(0), LD(np.inf))
        with np.errstate(all='ignore'):
            d = np.where(fin, np.abs(a - b) / scale, d)
        return float(d.max()) if d.size else 0.0

    e = {'elpd': dist(out[0], ref_out[0], np.maximum(LD(1), np.abs(ref_out[0]))),
         'khat': dist(out[1], ref_out[1], LD(1)),
         'n_eff': dist(out[2], ref_out[2], np.abs(ref_out[2]))}
    if lw is None:
        e['lw'] = 0.0
    else:
        lw, ref_lw = np.asarray(lw, dtype=LD), np.asarray(ref_lw, dtype=LD)
        live = ~(ref_lw <= LOG_DBL_MIN)                     # (NaN entries stay in: they must match)
        e['lw'] = dist(lw[live], ref_lw[live], LD(1))
    if not np.array_equal(np.asarray(out[3], dtype=float), np.asarray(ref_out[3], dtype=float), equal_nan=True):
        e = dict((q, float('inf')) for q in QUANTITIES)
    return e


# e0: the worst error of the float64 numpy statement (model_compare.psis_loo_from_pointwise) against the longdouble reference
# over the whole case table, per quantity, as test_psis_host.test_error_scale measures and checks it (recorded 2026-10-20).
# The bound for the host mirror and for the device is 100 * max(e0, 1e-13): both differ from the float64 statement only in
# the order of their sums and in libm, which is of the size of that statement's own rounding; the factor covers the
# amplification by n (up to 200 tail points) inside L_i.
E0 = {'elpd': 3.6e-16, 'khat': 8.9e-15, 'n_eff': 1.7e-15, 'lw': 2.6e-14}
BOUND = dict((q, 100.0 * max(E0[q], 1e-13)) for q in QUANTITIES)


def within(e, bound=None):
    bound = BOUND if bound is None else bound
    return all(e[q] <= bound[q] for q in QUANTITIES)


# ---- host mirror (csrc/pglm_psis.h through tests/csrc/psis_host.c) -----------------------------------------------------
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='psis_host_'), 'psis_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'psis_host.c'), '-lm'])
        Lb = C.CDLL(so)
        Lb.psis_run.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
        Lb.psis_tail.argtypes = [C.c_longlong]
        Lb.psis_tail.restype = C.c_longlong
        Lb.psis_max_draws.restype = C.c_longlong
        _LIB = Lb
    return _LIB


def host_mirror(ll):
    """(out (4, C), lw (S, C)) of the host build of the rule"""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    S, ncol = ll.shape
    out = np.full((4, ncol), 12345.678)
    lw = np.full((S, ncol), 12345.678)
    assert lib().psis_run(ll.ctypes.data, S, ncol, out.ctypes.data, lw.ctypes.data) == 0
    return out, lw
