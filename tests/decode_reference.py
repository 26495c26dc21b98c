"""What the tests of stimulus decoding share: the cases of tests/decode_cases.json and their inputs, the gcc build of the host
mirror tests/csrc/decode_host.c (the rules of csrc/pglm_decode.h), and a numpy longdouble reference written from the formulas
of the feature (include/pyglm_hip.h, "Stimulus decoding"), not from the C header.

The allowance A of the bound.  A device or mirror value may differ from the longdouble reference by at most
    (n_addends + A) * 2^-53 * sum |addends|,
n_addends and sum |addends| computed here for that output; for g_u and H v the addends are the products along the whole chain
(L^T, K^T, the two parts of r or cc, and for H v K and L again).  A is what the rate, residual and curvature functions are
granted.  tests/pointwise_reference.py, tests/rate_reference.py and tests/hvp_reference.py state their grants as relative
tolerances of whole sums, not per element in units of 2^-53 of the element's absolute parts, so A is measured: the worst error
of the HOST MIRROR's ll term, residual and curvature (at the mirror's own f64 current x = c + K * L u) against this reference
over the whole table, in units of 2^-53 * (sum of the absolute values of the element's two parts).
    A_MEASURED = 104    measured 103.06 (the ll term of case n3_mid, where lam is close to 1 and log lam close to 0), rounded up;
                        the next largest figures are 28.04 (n33_rt70_d3) and 21.90 (cc of n70_two_slabs).
                        tests/test_decode_cases.py::test_allowance_measured_on_the_mirror prints the figure of every case and
                        asserts that none exceeds this record
    A_FACTOR   = 4      for the device's fused multiply-adds and its different exp / log implementation
    A          = 416

A case: N neurons, nT bins of dt = 1 ms, a stimulus of D dimensions through B raised-cosine-like temporal basis functions over
Rt taps with random weights, Tu frames of q bins, recorded spikes S (Poisson counts at 50 Hz with bins forced to 2 and 3
spikes, a spike in bin 0 of neuron 0 and in the last bin of the last neuron, 'silent': a neuron without a spike).  The offset
c = bias + coupling currents is made of dyadic numbers (bias level + k / 4, coupling basis k / 8, weights k / 64, Weff in
{0, 1/2, 1, -1}) so that every sum in it is exact in f64: the device's forward pass, the mirror and the reference hold the
same c, and the bound measures the decoding path alone.  'level' puts the currents above 12 or below -12."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.001
U = 2.0 ** -53
A_MEASURED = 104
A_FACTOR = 4
A = A_MEASURED * A_FACTOR
R_IMP, B_IMP = 8, 2
LD = np.longdouble
_lib = None


def load():
    with open(os.path.join(ROOT, 'tests', 'decode_cases.json')) as f:
        return json.load(f)


CASES = load()
BY_NAME = dict((c['name'], c) for c in CASES)
NAMES = [c['name'] for c in CASES]


def nlin_kind(nlin):
    return {'exp': 0, 'explinear': 1}[nlin]


def rho_of(c):
    return np.inf if c['rho'] is None else float(c['rho'])


def prior_of(c):
    return (float(c['mu']), float(c['sigma']), rho_of(c))


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of a case, read-only: S (nT, N) uint8; ibasis_imp (R_IMP, B_IMP), theta (N, P) with P = 1 + D B + N B_IMP (bias,
    stimulus weights, coupling weights), Weff (N, N); basis (Rt, B); c (nT, N) the offset (exact); u (Tu, D) the point; v1, v2
    (Tu, D) the two directions."""
    c = BY_NAME[name]
    N, nT, Rt, D, B, Tu = c['N'], c['nT'], c['Rt'], c['D'], c['B'], c['Tu']
    rng = np.random.RandomState(4000 + c['seed'])
    S = rng.poisson(0.05, size=(nT, N)).astype(np.uint8)
    active = np.array([n for n in range(N) if n != c.get('silent')])
    bins = rng.choice(np.arange(1, nT - 1), size=5, replace=False)
    S[bins[:4], active[rng.randint(0, active.size, size=4)]] = 2
    S[bins[4], active[rng.randint(0, active.size)]] = 3
    if 'silent' in c:
        S[:, c['silent']] = 0
    S[0, 0] = max(S[0, 0], 1) if c.get('silent') != 0 else 0
    S[nT - 1, N - 1] = max(S[nT - 1, N - 1], 1) if c.get('silent') != N - 1 else 0
    if c.get('silent') == 0:                          # (the spike in bin 0 goes to the next neuron then)
        S[0, 1] = 1
    if c.get('silent') == N - 1 and N > 1:
        S[nT - 1, N - 2] = 1
    ib_imp = rng.randint(0, 9, size=(R_IMP, B_IMP)) / 8.0
    w_imp = rng.randint(-4, 5, size=(N, N * B_IMP)) / 64.0
    Weff = rng.choice([0.0, 0.5, 1.0, -1.0], size=(N, N), p=[0.4, 0.2, 0.2, 0.2])
    bias = c['level'] + rng.randint(-2, 3, size=N) / 4.0
    # temporal basis of the stimulus: B bumps over the Rt taps; weights so that the stimulus current is of order 1
    tau = (np.arange(Rt)[:, None] + 0.5) / Rt
    basis = np.exp(-0.5 * ((tau - (np.arange(B)[None, :] + 0.5) / B) * (2.0 * B)) ** 2) * (1.0 + 0.1 * rng.rand(Rt, B))
    w_stim = rng.randn(N, D * B) * (0.6 / np.sqrt(Rt * D * B))
    theta = np.concatenate([bias[:, None], w_stim, w_imp], axis=1)
    # the offset, exact: c[t, n] = bias_n + sum_{n', b, tau} S[t - tau, n'] ib_imp[tau - 1, b] w_imp[n, n' B + b] Weff[n', n]
    W = (w_imp.reshape(N, N, B_IMP) * Weff.T[:, :, None])                       # [n, n', b]
    H = np.einsum('tb,nmb->tmn', ib_imp, W)                                    # [tau - 1, n', n]
    cc = np.tile(bias[None, :], (nT, 1))
    for k in range(R_IMP):
        cc[k + 1:] += S[:nT - 1 - k].astype(float) @ H[k]
    u = c['mu'] + 0.7 * rng.randn(Tu, D)
    v1 = rng.randn(Tu, D)
    v2 = np.sin(0.05 * np.arange(Tu)[:, None] * (1.0 + np.arange(D)[None, :])) + 0.25
    out = dict(S=S, ib_imp=ib_imp, theta=theta, Weff=Weff, basis=basis, c=cc, u=u, v1=v1, v2=v2)
    for a in out.values():
        a.setflags(write=False)
    return out


def offset_longdouble(name):
    """c of a case in longdouble, term by term (the check that make_case's f64 sums were exact)."""
    c = BY_NAME[name]
    m = make_case(name)
    N, nT = c['N'], c['nT']
    W = (m['theta'][:, 1 + c['D'] * c['B']:].reshape(N, N, B_IMP) * m['Weff'].T[:, :, None]).astype(LD)
    out = np.tile(m['theta'][None, :, 0].astype(LD), (nT, 1))
    for k in range(R_IMP):
        for b in range(B_IMP):
            out[k + 1:] += (m['S'][:nT - 1 - k].astype(LD) * LD(m['ib_imp'][k, b])) @ W[:, :, b].T
    return out


# ---- the longdouble reference ---------------------------------------------------------------------------------------------------
def interp_plan(nT, Tu, q):
    """s[t] = w0[t] u[i0[t]] + w1[t] u[i1[t]]"""
    t = np.arange(nT)
    i = t // q
    r = t % q
    clamp = i >= Tu - 1
    i0 = np.where(clamp, Tu - 1, i)
    i1 = np.where(clamp, Tu - 1, i + 1)
    w1 = np.where(clamp, LD(0), r.astype(LD) / LD(q))
    w0 = np.where(clamp, LD(1), LD(1) - r.astype(LD) / LD(q))
    return i0, i1, w0, w1


def L_apply(u, nT, q):
    i0, i1, w0, w1 = interp_plan(nT, u.shape[0], q)
    return w0[:, None] * u[i0] + w1[:, None] * u[i1]


def Lt_apply(g, Tu, q):
    i0, i1, w0, w1 = interp_plan(g.shape[0], Tu, q)
    out = np.zeros((Tu, g.shape[1]), dtype=LD)
    np.add.at(out, i0, w0[:, None] * g)
    np.add.at(out, i1, w1[:, None] * g)
    return out


def filters(basis, theta, D):
    """K (Rt, D, N)"""
    B = basis.shape[1]
    w = theta[:, 1:1 + D * B].astype(LD).reshape(-1, D, B)                      # [n, d, b]
    return np.einsum('tb,ndb->tdn', basis.astype(LD), w)


def K_apply(K, s):
    """I (nT, N) = K * s, strictly causal"""
    nT = s.shape[0]
    Rt, D, N = K.shape
    I = np.zeros((nT, N), dtype=LD)
    for tau in range(min(Rt, nT - 1)):
        for d in range(D):
            I[tau + 1:] += s[:nT - 1 - tau, d, None] * K[tau, d][None, :]
    return I


def Kt_apply(K, y):
    """g_s (nT, D) = K^T y, rows past nT zero"""
    nT = y.shape[0]
    Rt, D, N = K.shape
    g = np.zeros((nT, D), dtype=LD)
    for tau in range(min(Rt, nT - 1)):
        for d in range(D):
            g[:nT - 1 - tau, d] += y[tau + 1:] @ K[tau, d]
    return g


def _log1p_minus(z):
    """log1p(z) - z for 0 <= z <= 1 without the cancellation at small z"""
    small = z < 0.05
    zs = np.where(small, z, LD(0))
    # Horner of sum_{k >= 2} (-1)^(k+1) z^k / k = z^2 (-1/2 + z/3 - z^2/4 ...)
    acc = np.zeros_like(z)
    for k in range(40, 1, -1):
        acc = LD((-1) ** (k + 1)) / LD(k) + zs * acc
    ser = zs * zs * acc
    return np.where(small, ser, np.log1p(z) - z)


def point(x, S, nlin, dt):
    """Per element: the two parts of the ll term (S log lam, -dt lam), of r (S (log lam)', -dt lam') and of cc (S (log lam)'',
    -dt lam''), longdouble."""
    x = x.astype(LD)
    S = S.astype(LD)
    dt = LD(dt)
    if nlin == 'exp':
        lam = np.exp(x)
        return (S * x, -dt * lam), (S, -dt * lam), (np.zeros_like(x), -dt * lam)
    e = np.exp(-np.abs(x))
    lam = np.maximum(x, LD(0)) + np.log1p(e)
    sig = np.where(x >= 0, LD(1) / (LD(1) + e), e / (LD(1) + e))
    # (log lam)'' = sig / lam^2 ((1 - sig) lam - sig); for x < 0 with z = e^x: (1 - sig) lam - sig = (log1p(z) - z) / (1 + z)
    # (1 - sig is e / (1 + e) for x >= 0: no cancellation; sig (1 - sig) = e / (1 + e)^2 for both signs)
    inner = np.where(x >= 0, e / (LD(1) + e) * lam - sig, _log1p_minus(np.where(x < 0, e, LD(0))) / (LD(1) + e))
    h = sig / (lam * lam) * inner
    loglam = np.log(lam)
    return (np.where(S > 0, S * loglam, LD(0)), -dt * lam), (S * sig / lam, -dt * sig), (S * h, -dt * e / ((LD(1) + e) * (LD(1) + e)))


def prior_parts(u, mu, sigma, rho):
    """value terms (list of arrays), gradient parts (list of (Tu, D) arrays) of log p"""
    a = LD(1) / (LD(sigma) * LD(sigma))
    b = LD(0) if not np.isfinite(rho) else LD(1) / (LD(rho) * LD(rho))
    dev = u - LD(mu)
    diff = u[1:] - u[:-1]
    vals = [-LD(0.5) * a * dev * dev, -LD(0.5) * b * diff * diff]
    g1 = -a * dev
    g2 = np.zeros_like(u)
    g3 = np.zeros_like(u)
    g2[1:] = -b * diff                      # -(u_i - u_{i-1}) / rho^2
    g3[:-1] = b * diff                      # -(u_i - u_{i+1}) / rho^2
    return vals, [g1, g2, g3]


def frame_bins(nT, Tu, q):
    """the number of bins frame i collects from"""
    i0, i1, w0, w1 = interp_plan(nT, Tu, q)
    n = np.zeros(Tu)
    np.add.at(n, i0, (w0 != 0).astype(float))
    np.add.at(n, i1, ((w1 != 0) & (i1 != i0)).astype(float))
    return n


@functools.lru_cache(maxsize=None)
def reference(name):
    """The longdouble reference of a case at its point u and directions v1, v2: values, and for every output the number of
    addends and the sum of their absolute values.  Keys: F, ll, lp, g (Tu, D), hv1, hv2; '<key>_n', '<key>_abs'; x, term, r, cc
    (nT, N) and their '_abs'."""
    c = BY_NAME[name]
    m = make_case(name)
    nT, N, D, Rt, Tu, q = c['nT'], c['N'], c['D'], c['Rt'], c['Tu'], c['q']
    mu, sigma, rho = prior_of(c)
    K = filters(m['basis'], m['theta'], D)
    aK = np.abs(K)
    u = m['u'].astype(LD)
    s = L_apply(u, nT, q)
    x = m['c'].astype(LD) + K_apply(K, s)
    tp, rp, cp = point(x, m['S'], c['nlin'], DT)
    term, r, cc = tp[0] + tp[1], rp[0] + rp[1], cp[0] + cp[1]
    aterm, ar, acc = np.abs(tp[0]) + np.abs(tp[1]), np.abs(rp[0]) + np.abs(rp[1]), np.abs(cp[0]) + np.abs(cp[1])
    vals, gparts = prior_parts(u, mu, sigma, rho)
    ll = term.sum()
    lp = sum(v.sum() for v in vals)
    out = dict(x=x, term=term, r=r, cc=cc, term_abs=aterm, r_abs=ar, cc_abs=acc)
    out['ll'], out['lp'], out['F'] = ll, lp, ll + lp
    out['ll_n'], out['ll_abs'] = 2 * nT * N, aterm.sum()
    out['lp_n'], out['lp_abs'] = 2 * Tu * D, sum(np.abs(v).sum() for v in vals)
    out['F_n'], out['F_abs'] = out['ll_n'] + out['lp_n'], out['ll_abs'] + out['lp_abs']
    nb = frame_bins(nT, Tu, q)[:, None] * np.ones((1, D))
    out['g'] = Lt_apply(Kt_apply(K, r), Tu, q) + sum(gparts)
    out['g_abs'] = Lt_apply(Kt_apply(aK, ar), Tu, q) + sum(np.abs(p) for p in gparts)
    out['g_n'] = nb * (N * Rt * 2) + 3
    for key, v in (('hv1', m['v1']), ('hv2', m['v2'])):
        v = v.astype(LD)
        _, hparts = prior_parts(v, 0.0, sigma, rho)
        out[key] = Lt_apply(Kt_apply(K, cc * K_apply(K, L_apply(v, nT, q))), Tu, q) + sum(hparts)
        out[key + '_abs'] = Lt_apply(Kt_apply(aK, acc * K_apply(aK, L_apply(np.abs(v), nT, q))), Tu, q) + sum(np.abs(p) for p in hparts)
        out[key + '_n'] = nb * (N * Rt * 2) * (D * Rt * 2) + 3
    return out


def objective_longdouble(name, u):
    """F(u) alone, for the central differences"""
    c = BY_NAME[name]
    m = make_case(name)
    K = filters(m['basis'], m['theta'], c['D'])
    x = m['c'].astype(LD) + K_apply(K, L_apply(u, c['nT'], c['q']))
    tp, _, _ = point(x, m['S'], c['nlin'], DT)
    vals, _ = prior_parts(u, *prior_of(c))
    return (tp[0] + tp[1]).sum() + sum(v.sum() for v in vals)


def gradient_longdouble(name, u):
    c = BY_NAME[name]
    m = make_case(name)
    K = filters(m['basis'], m['theta'], c['D'])
    x = m['c'].astype(LD) + K_apply(K, L_apply(u, c['nT'], c['q']))
    _, rp, _ = point(x, m['S'], c['nlin'], DT)
    _, gparts = prior_parts(u, *prior_of(c))
    return Lt_apply(Kt_apply(K, rp[0] + rp[1]), c['Tu'], c['q']) + sum(gparts)


def bound(ref, key):
    """(n_addends + A) 2^-53 sum |addends| of output `key`"""
    return (np.asarray(ref[key + '_n'], dtype=LD) + A) * LD(U) * ref[key + '_abs']


def check(value, ref, key, label=''):
    """The worst ratio error / bound of output `key` (printed by the callers before they assert <= 1)."""
    err = np.abs(np.asarray(value).astype(LD) - ref[key])
    b = bound(ref, key)
    ratio = float(np.max(err / b))
    print('%s %s: max err / bound = %.4f (max err %.3e)' % (label, key, ratio, float(np.max(err))))
    return ratio


# ---- the gcc mirror ---------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def mirror_sources():
    return [os.path.join(ROOT, 'tests', 'csrc', 'decode_host.c')] + \
        [os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', h) for h in ('pglm_decode.h', 'pglm_hmc.h', 'pglm_linesearch.h')]


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, 'tests', 'csrc', 'decode_host.so')
        srcs = mirror_sources()
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, srcs[0], '-lm'])
        L = ctypes.CDLL(so)
        vp, ll, ci, cd = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double
        L.decode_eval.restype = None
        L.decode_eval.argtypes = [ll, ci, ci, cd, vp, vp, vp, ci, ci, ci, vp, ci, vp, ll, ci, cd, cd, cd, vp, vp, vp, vp, vp]
        L.decode_points.restype = None
        L.decode_points.argtypes = [ll, ci, ci, cd, vp, vp, vp, ci, ci, ci, vp, ci, vp, ll, ci, vp, vp, vp, vp]
        for fn, at in ((L.decode_interp, [vp, ll, ci, ci, ll, vp]), (L.decode_interp_t, [vp, ll, ci, ci, ll, vp]),
                       (L.decode_conv, [vp, ci, ci, ci, vp, ll, vp]), (L.decode_corr, [vp, ci, ci, ci, vp, ll, vp])):
            fn.restype = None
            fn.argtypes = at
        _lib = L
    return _lib


def _arrays(name):
    m = make_case(name)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    return m, f(m['c']), f(m['S']), f(m['basis']), f(m['theta'])


def mirror_eval(name, u, v=None):
    """(F (3,), grad, hv or None) of the gcc mirror"""
    c = BY_NAME[name]
    m, cc, S, basis, theta = _arrays(name)
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    nT, N, Rt, D = c['nT'], c['N'], c['Rt'], c['D']
    F, g = np.empty(3), np.empty_like(u)
    hv = None if v is None else np.empty_like(u)
    work = np.empty(Rt * D * N + 3 * nT * N + 2 * nT * D)
    mu, sigma, rho = prior_of(c)
    lib().decode_eval(nT, N, nlin_kind(c['nlin']), DT, _p(cc), _p(S), _p(basis), Rt, c['B'], D, _p(theta), theta.shape[1], _p(u),
                      u.shape[0], c['q'], mu, sigma, rho, _p(v), _p(F), _p(g), _p(hv), _p(work))
    return F, g, hv


def mirror_points(name):
    """(term, r, cc) (nT, N) of the gcc mirror at the case's point"""
    c = BY_NAME[name]
    m, cc, S, basis, theta = _arrays(name)
    u = np.ascontiguousarray(m['u'], dtype=np.float64)
    nT, N, Rt, D = c['nT'], c['N'], c['Rt'], c['D']
    out = [np.empty((nT, N)) for _ in range(3)]
    work = np.empty(Rt * D * N + nT * D)
    lib().decode_points(nT, N, nlin_kind(c['nlin']), DT, _p(cc), _p(S), _p(basis), Rt, c['B'], D, _p(theta), theta.shape[1], _p(u),
                        u.shape[0], c['q'], _p(out[0]), _p(out[1]), _p(out[2]), _p(work))
    return out


def write_problems(path, names=None):
    """The problem file the stand-alone program of tests/csrc/decode_host.c reads, from the case table: per case a header line
    "nT N nlin dt Rt B D P Tu q mu sigma rho" and the arrays c, S, basis, theta, u, v1 as text (repr: exact).  The sanitizer run
    of the mirror, a CPU program on its own:
        gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DDECODE_HOST_MAIN -o decode_host_main \\
            tests/csrc/decode_host.c -lm
        python -c "from tests import decode_reference as DR; DR.write_problems('decode_problems.txt')"
        ./decode_host_main decode_problems.txt"""
    with open(path, 'w') as f:
        for name in (NAMES if names is None else names):
            c = BY_NAME[name]
            m = make_case(name)
            mu, sigma, rho = prior_of(c)
            f.write("%d %d %d %r %d %d %d %d %d %d %r %r %s\n" % (c['nT'], c['N'], nlin_kind(c['nlin']), DT, c['Rt'], c['B'], c['D'],
                                                                  m['theta'].shape[1], c['Tu'], c['q'], mu, sigma,
                                                                  'inf' if np.isinf(rho) else repr(rho)))
            for a in (m['c'], m['S'].astype(float), m['basis'], m['theta'], m['u'], m['v1']):
                f.write(' '.join(repr(float(x)) for x in np.asarray(a).ravel()) + '\n')
