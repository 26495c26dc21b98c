"""What the Wald tests share: the case table tests/wald_cases.json with its generators, a numpy.longdouble reference of
the rule of csrc/pglm_wald.h, the gcc build of the host mirror tests/csrc/wald_host.c and the comparison of bits.

The reference states the MATHEMATICS of the rule in longdouble (64-bit mantissa on x86): S = W_g W_g^T as a plain longdouble
product, a longdouble Cholesky solve, T = w^T S^-1 w, lin = c^T w, var = c^T S c -- the order of a sum is below its precision.

Bounds.  T and var: err <= c P u kappa_2(S) |value|, kappa_2 of the longdouble S.  c is measured, not derived: the mirror's
largest err / (P u kappa_2 |value|) over the table is stored in the JSON as 'measured_c' and the test allows 4 x that (other
libm / compiler versions); the GPU is held to the mirror's bits, so this bound never loosens a device check.  lin is held to
B u sum |c_b w_b|."""
import ctypes
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
LD_IS_WIDER = np.finfo(LD).eps < np.finfo(np.float64).eps
U = 2.0 ** -53
NOUT = 4
MAX_B = 16

_cases = None
_table = None
_lib = None


def table():
    global _table
    if _table is None:
        with open(os.path.join(ROOT, 'tests', 'wald_cases.json')) as f:
            _table = json.load(f)
    return _table


def load():
    return table()['cases']


def make_case(c):
    """-> dict(W (M, P, ld), theta (M, P), c (B,), info (M,) int32) of a case of the table.  W: random lower triangular with
    a positive diagonal, row i scaled by 10^U(-2, 1); the strict upper triangle and the pad columns hold NaN (they must not
    be read).  'zero_w': [m, g] sets that group's weights to 0; 'equal_rows': [m, g] gives rows o and o + 1 of that group the
    same two entries 1.5, 2 (S_00 = S_10 = S_11 = 6.25 exactly: the second pivot is exactly 0); 'info_row': m has info = 3."""
    rng = np.random.default_rng(c['seed'])
    M, P, B, G, first, ld = c['M'], c['P'], c['B'], c['G'], c['first'], c['P'] + c['pad']
    W = np.full((M, P, ld), np.nan)
    low = np.tril(rng.normal(size=(M, P, P)))
    d = np.arange(P)
    low[:, d, d] = np.abs(low[:, d, d]) + 0.5
    low *= (10.0 ** rng.uniform(-2.0, 1.0, size=(M, P)))[:, :, None]
    il = np.tril_indices(P)
    for m in range(M):
        W[m][il] = low[m][il]
    theta = rng.normal(size=(M, P))
    cvec = rng.normal(size=B)
    if 'zero_w' in c:
        m, g = c['zero_w']
        theta[m, first + g * B:first + (g + 1) * B] = 0.0
    if 'equal_rows' in c:
        m, g = c['equal_rows']
        o = first + g * B
        for r in (o, o + 1):
            W[m, r, :r + 1] = 0.0
            W[m, r, 0:2] = (1.5, 2.0)
    info = np.zeros(M, dtype=np.int32)
    if c.get('info_row') is not None:
        info[c['info_row']] = 3
    return {'W': W, 'theta': theta, 'c': cvec, 'info': info}


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, 'tests', 'csrc', 'wald_host.so')
        srcs = [os.path.join(ROOT, 'tests', 'csrc', 'wald_host.c')] + \
            [os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', h) for h in ('pglm_wald.h', 'pglm_hmc.h', 'pglm_linesearch.h')]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, srcs[0], '-lm'])
        L = ctypes.CDLL(so)
        vp, ll = ctypes.c_void_p, ctypes.c_longlong
        L.wald_run.restype = None
        L.wald_run.argtypes = [vp, ll, ll, ll, vp, ll, ll, ctypes.c_int, vp, vp, vp, vp]
        _lib = L
    return _lib


def host_wald(W, theta, first, G, B, c, info=None, want_u=False):
    """the gcc mirror: -> out (M, G, 4), or (out, u (G M, P)) with want_u"""
    W = np.ascontiguousarray(W, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    M, P, ld = W.shape
    out = np.empty((M, G, NOUT))
    u = np.empty((G * M, P)) if want_u else None
    inf = None if info is None else np.ascontiguousarray(info, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    lib().wald_run(p(W), M, P, ld, p(theta), first, G, B, p(c), p(inf), p(out), p(u))
    return (out, u) if want_u else out


def same_bits(a, b):
    """a and b hold NaN at the same places and the same bits everywhere else"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- longdouble algebra -------------------------------------------------------------------------------------------------
def ld_cholesky(S):
    S = np.array(S, dtype=LD)
    n = S.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for a in range(n):
        for b in range(a + 1):
            s = S[a, b] - np.dot(L[a, :b], L[b, :b])
            L[a, b] = s / L[b, b] if b < a else np.sqrt(s)
    return L


def ld_solve_spd(S, w):
    L = ld_cholesky(S)
    n = L.shape[0]
    z = np.zeros(n, dtype=LD)
    for a in range(n):
        z[a] = (LD(w[a]) - np.dot(L[a, :a], z[:a])) / L[a, a]
    y = np.zeros(n, dtype=LD)
    for a in range(n - 1, -1, -1):
        y[a] = (z[a] - np.dot(L[a + 1:, a], y[a + 1:])) / L[a, a]
    return y


def ld_inverse_spd(A):
    n = A.shape[0]
    eye = np.eye(n)
    return np.stack([ld_solve_spd(A, eye[i]) for i in range(n)], axis=1)


def reference_group(Wm, theta_m, o, B, c):
    """longdouble T, lin, var, kappa_2(S), sum |c_b w_b| and S of one group of the row (Wm (P, >= P), lower triangle read)"""
    P = theta_m.size
    Wg = np.tril(np.where(np.isnan(Wm[:, :P]), 0.0, Wm[:, :P]))[o:o + B].astype(LD)
    S = Wg.dot(Wg.T)
    w = theta_m[o:o + B].astype(LD)
    cl = np.asarray(c, dtype=LD)
    y = ld_solve_spd(S, w)
    return {'T': np.dot(w, y), 'lin': np.dot(cl, w), 'var': np.dot(cl, S.dot(cl)),
            'kappa': float(np.linalg.cond(S.astype(np.float64))), 'abs_lin': float(np.sum(np.abs(cl * w))), 'S': S}


def ratios(out4, ref, P):
    """err_T and err_var over P u kappa |value|, and err_lin over B u sum |c w|, of one group against reference_group's dict"""
    den = P * U * ref['kappa']
    rT = float(abs(LD(out4[0]) - ref['T'])) / (den * float(abs(ref['T']))) if ref['T'] != 0 else float(abs(out4[0]))
    rV = float(abs(LD(out4[2]) - ref['var'])) / (den * float(abs(ref['var'])))
    rL = float(abs(LD(out4[1]) - ref['lin'])) / ref['abs_lin'] / U / ref['S'].shape[0]
    return rT, rV, rL


def expected_info(c, m, g):
    return 2 if c.get('equal_rows') == [m, g] else 0
