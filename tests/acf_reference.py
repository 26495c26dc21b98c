"""Longdouble reference of the independence rule of theano_pyglm_amd/csrc/pglm_acf.h, the case table tests/acf_cases.json and
the gcc build of the host mirror tests/csrc/acf_host.c.

The reference states the MATHEMATICS of the rule in numpy.longdouble (64-bit mantissa on x86): the scores by AS 241 PPND16
with its coefficients read as longdoubles, the sums as plain longdouble sums -- the order of a sum is below its precision.  Its
normal quantile is held to 1e-15 of mpmath's in tests/test_acf_cases.py.

Bounds (derived from the formats, not from the code under test):
  SCORE_RTOL 4e-15  relative: PPND16's stated 1e-16, a few ulp of log / exp / expm1 / sqrt and the 16 roundings of the two
                    Horner forms in double.
  R_TOL 1e-12       absolute, n <= 1e5: the piecewise sum carries at most (256 + n / 256) eps per unit of sum |terms| and
                    sum |d_i d_{i+k}| <= c_0, so r_k is off by about 1.5e-13 times a small factor.
  Q_RTOL 1e-9       relative: Q = n (n + 2) sum r_k^2 / n_k, every r_k^2 off by 2 |r_k| 1e-12 relatively 2e-12 / |r_k|, which the
                    lags that carry Q (|r_k| of the order 1 / sqrt(n) >= 3e-3) keep below 1e-9.
"""
import ctypes
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
LD_IS_WIDER = np.finfo(LD).eps < np.finfo(np.float64).eps
SCORE_RTOL = 4e-15
R_TOL = 1e-12
Q_RTOL = 1e-9
NHEAD = 6
PIECE = 256
MAX_LAG = 64
DBL_MIN = np.finfo(np.float64).tiny
LN2_HI = LD('0.6931471805599453094172321214581765680755')        # the longdouble nearest log 2 ..
LN2_LO = LD('-1.14583527267987328109353e-20')                     # .. and log 2 minus it

_A = ('3.3871328727963666080e0', '1.3314166789178437745e2', '1.9715909503065514427e3', '1.3731693765509461125e4',
      '4.5921953931549871457e4', '6.7265770927008700853e4', '3.3430575583588128105e4', '2.5090809287301226727e3')
_B = ('1.0', '4.2313330701600911252e1', '6.8718700749205790830e2', '5.3941960214247511077e3', '2.1213794301586595867e4',
      '3.9307895800092710610e4', '2.8729085735721942674e4', '5.2264952788528545610e3')
_C = ('1.42343711074968357734e0', '4.63033784615654529590e0', '5.76949722146069140550e0', '3.64784832476320460504e0',
      '1.27045825245236838258e0', '2.41780725177450611770e-1', '2.27238449892691845833e-2', '7.74545014278341407640e-4')
_D = ('1.0', '2.05319162663775882187e0', '1.67638483018380384940e0', '6.89767334985100004550e-1', '1.48103976427480074590e-1',
      '1.51986665636164571966e-2', '5.47593808499534494600e-4', '1.05075007164441684324e-9')
_E = ('6.65790464350110377720e0', '5.46378491116411436990e0', '1.78482653991729133580e0', '2.96560571828504891230e-1',
      '2.65321895265761230930e-2', '1.24266094738807843860e-3', '2.71155556874348757815e-5', '2.01033439929228813265e-7')
_F = ('1.0', '5.99832206555887937690e-1', '1.36929880922735805310e-1', '1.48753612908506148525e-2', '7.86869131145613259100e-4',
      '1.84631831751005468180e-5', '1.42151175831644588870e-7', '2.04426310338993978564e-15')


def _horner(c, u):
    v = np.full(u.shape, LD(c[-1]), dtype=LD)
    for a in c[-2::-1]:
        v = v * u + LD(a)
    return v


def ppnd_central(q):
    """Phi^-1(1/2 + q), |q| <= 0.425, in longdouble"""
    q = np.asarray(q, dtype=LD)
    u = LD('0.180625') - q * q
    return q * _horner(_A, u) / _horner(_B, u)


def ppnd_tail(r):
    """-Phi^-1(r) for a tail probability r < 0.075, in longdouble"""
    r = np.asarray(r, dtype=LD)
    u = np.sqrt(-np.log(r))
    return np.where(u <= 5, _horner(_C, u - LD('1.6')) / _horner(_D, u - LD('1.6')), _horner(_E, u - 5) / _horner(_F, u - 5))


def quantile(p=None, upper=None):
    """Phi^-1 at the probability p, or at 1 - upper where the upper tail probability is given (scalars)"""
    if upper is not None:
        return -quantile(p=upper)
    p = LD(p)
    q = p - LD('0.5')
    if abs(q) <= LD('0.425'):
        return ppnd_central(np.array([q]))[0]
    return -ppnd_tail(np.array([p]))[0] if q < 0 else ppnd_tail(np.array([1 - p]))[0]


def scores(tau):
    """the normal scores of the rule in longdouble (NaN where tau is NaN)"""
    tau = np.asarray(tau, dtype=np.float64)
    t = tau.astype(LD)
    g = np.full(t.shape, np.nan, dtype=LD)
    with np.errstate(all='ignore'):
        z = -np.expm1(-t)
        q = z - LD('0.5')
        mid = np.abs(q) <= LD('0.425')
        g[mid] = ppnd_central(-np.expm1((LN2_HI - t[mid]) + LN2_LO) / 2)
        tail = ~mid & ~np.isnan(t)
        r = np.where(q[tail] < 0, z[tail], np.exp(-t[tail]))
        r = np.maximum(r, LD(DBL_MIN))
        v = ppnd_tail(r)
        g[tail] = np.where(q[tail] < 0, -v, v)
    return g


def branch(tau):
    """'central', 'tail' or 'clamp' per element, as the double rule takes them"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(all='ignore'):
        z = -np.expm1(-tau)
        q = z - 0.5
        r = np.where(q < 0.0, z, np.exp(-tau))
    return np.where(np.abs(q) <= 0.425, 'central', np.where(r < DBL_MIN, 'clamp', 'tail'))


def run_ends(run_lens):
    ends = np.cumsum(run_lens)
    return np.concatenate([np.full(int(l), int(e)) for l, e in zip(run_lens, ends)]) if len(run_lens) else np.zeros(0, dtype=np.int64)


def pair_counts(run_lens, L):
    k = np.arange(1, L + 1)
    ls = np.asarray(run_lens, dtype=np.int64).reshape(-1)
    return np.sum(np.maximum(ls[:, None] - k[None, :], 0), axis=0) if ls.size else np.zeros(L, dtype=np.int64)


def reference(tau, run_lens, L, g=None):
    """one segment -> (NHEAD + L) longdoubles: n, mean, c_0, Q, dof, 0, r_1 .. r_L by the mathematics of the rule"""
    tau = np.asarray(tau, dtype=np.float64)
    n = tau.size
    out = np.full(NHEAD + L, np.nan, dtype=LD)
    out[0] = n
    if np.any(~(tau >= 0.0)):
        return out
    out[5] = 0
    out[4] = 0
    if n == 0:
        out[2] = 0
        return out
    g = scores(tau) if g is None else np.asarray(g, dtype=LD)
    mean = np.sum(g) / n
    d = g - mean
    c0 = LD(0) if np.all(tau == tau[0]) else np.sum(d * d)          # a constant segment: exactly 0 in the reals
    out[1], out[2] = mean, c0
    if n < 3 or c0 == 0:
        return out
    end = run_ends(run_lens)
    i = np.arange(n)
    nk = pair_counts(run_lens, L)
    Q, dof = LD(0), 0
    for k in range(1, L + 1):
        ok = i + k < end
        assert int(np.sum(ok)) == int(nk[k - 1])
        if nk[k - 1] < 1:
            continue
        r = np.sum(d[ok] * d[i[ok] + k]) / c0
        Q += r * r * LD(n) * LD(n + 2) / LD(int(nk[k - 1]))
        dof += 1
        out[NHEAD + k - 1] = r
    out[3], out[4] = Q, dof
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------
_cases = None


def load():
    global _cases
    if _cases is None:
        with open(os.path.join(ROOT, 'tests', 'acf_cases.json')) as f:
            _cases = json.load(f)['cases']
    return _cases


_SPECIAL = {'inf': np.inf, 'nan': np.nan}


def case_tau(c):
    """the intervals of a case: Exp(1) draws (seeded), AR(1)-like where 'rho' is given, then the values of 'set'"""
    n = int(sum(c['runs']))
    rng = np.random.default_rng(c['seed'])
    if 'const' in c:
        tau = np.full(n, float(c['const']))
    elif 'rho' in c:
        tau = copula_ar1(rng, n, c['rho'])
    else:
        tau = rng.exponential(size=n)
    for i, v in c.get('set', {}).items():
        tau[int(i)] = _SPECIAL[v] if isinstance(v, str) else float(v)
    return tau


def copula_ar1(rng, n, rho):
    """tau = -log(1 - Phi(g)), g a stationary Gaussian AR(1) of coefficient rho"""
    from scipy import special
    e = rng.standard_normal(n)
    g = np.empty(n)
    g[0] = e[0]
    s = np.sqrt(1.0 - rho * rho)
    for i in range(1, n):
        g[i] = rho * g[i - 1] + s * e[i]
    return -special.log_ndtr(-g)                                   # -log(1 - Phi(g)) without the cancellation


def offsets(run_lens_per_segment):
    """(run_off, seg_run) of a list of segments, each a list of run lengths"""
    lens = [l for seg in run_lens_per_segment for l in seg]
    run_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    seg_run = np.concatenate(([0], np.cumsum([len(seg) for seg in run_lens_per_segment]))).astype(np.int64)
    return run_off, seg_run


def crowd(c, n_others=300, at=150):
    """the case's segment among n_others seeded ones (every seventh empty, some of several runs): (tau, segments, at)"""
    rng = np.random.default_rng(99)
    segs, parts = [], []
    for m in range(n_others + 1):
        if m == at:
            segs.append(list(c['runs']))
            parts.append(case_tau(c))
            continue
        runs = [] if m % 7 == 0 else [int(v) for v in rng.integers(0, 40, size=1 + m % 3)]
        segs.append(runs)
        parts.append(rng.exponential(size=int(sum(runs))))
    return np.concatenate(parts), segs, at


# ---- the host mirror --------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, 'tests', 'csrc', 'acf_host.so')
        srcs = [os.path.join(ROOT, 'tests', 'csrc', 'acf_host.c')] + \
            [os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', h) for h in ('pglm_acf.h', 'pglm_gof.h', 'pglm_diag.h', 'pglm_hmc.h')]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, srcs[0], '-lm'])
        L = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        L.acf_score.restype = ctypes.c_double
        L.acf_score.argtypes = [ctypes.c_double]
        L.acf_segments.argtypes = [vp, vp, vp, ctypes.c_longlong, ctypes.c_int, vp, vp]
        L.acf_from_scores.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, ctypes.c_int, vp]
        _lib = L
    return _lib


def _arrs(tau, segs):
    run_off, seg_run = offsets(segs)
    t = np.ascontiguousarray(tau, dtype=np.float64)
    assert run_off[-1] == t.size
    return (t if t.size else np.zeros(1)), run_off, seg_run


def host_acf(tau, segs, L):
    """the mirror on segments of runs: (out (M, NHEAD + L), scores)"""
    t, run_off, seg_run = _arrs(tau, segs)
    out = np.full((len(segs), NHEAD + L), -7.0)
    g = np.full(t.size, np.nan)
    assert lib().acf_segments(t.ctypes.data, run_off.ctypes.data, seg_run.ctypes.data, len(segs), L, out.ctypes.data, g.ctypes.data) == 0
    return out, g[:int(run_off[-1])]


def host_from_scores(tau, g, segs, L):
    t, run_off, seg_run = _arrs(tau, segs)
    gg = np.ascontiguousarray(g, dtype=np.float64)
    gg = gg if gg.size else np.zeros(1)
    out = np.full((len(segs), NHEAD + L), -7.0)
    assert lib().acf_from_scores(t.ctypes.data, gg.ctypes.data, run_off.ctypes.data, seg_run.ctypes.data, len(segs), L,
                                 out.ctypes.data) == 0
    return out


def split_runs(x, run_lens):
    e = np.cumsum(run_lens)
    return [x[int(b - l):int(b)] for l, b in zip(run_lens, e)]


def check_against_reference(label, out, g, tau, run_lens, L):
    """the documented bounds of one segment's device or mirror result against the longdouble reference"""
    ref = reference(tau, run_lens, L)
    assert out[0] == tau.size, label
    gref = scores(tau)
    fin = ~np.isnan(gref)
    assert np.all(np.isnan(g[~fin])), label
    err = np.max(np.abs(g[fin].astype(LD) - gref[fin]) / np.abs(gref[fin])) if np.any(fin) else 0.0
    assert err <= SCORE_RTOL, (label, float(err))
    if np.isnan(ref[1]) and tau.size:                                # void: everything but n
        assert np.all(np.isnan(out[1:])), label
        return float(err), 0.0
    assert out[5] == 0.0 and out[4] == float(ref[4]), (label, out[4], ref[4])
    if tau.size:
        assert abs(out[1] - float(ref[1])) <= 1e-13 * max(1.0, float(np.max(np.abs(gref)))), label
    r, rr = out[NHEAD:], ref[NHEAD:]
    assert np.array_equal(np.isnan(r), np.isnan(rr.astype(float))), (label, r, rr)
    ok = ~np.isnan(r)
    rerr = float(np.max(np.abs(r[ok].astype(LD) - rr[ok]))) if np.any(ok) else 0.0
    assert rerr <= R_TOL, (label, rerr)
    if np.isnan(float(ref[3])):
        assert np.isnan(out[3]), label
    else:
        assert abs(out[3] - float(ref[3])) <= Q_RTOL * float(ref[3]), (label, out[3], float(ref[3]))
    return float(err), rerr
