"""Float64 references of the Hessian-vector tests (test infrastructure, no GPU):

  curvature_stable   c(x, s) without the cancellation of tests/test_hvp_host.curvature (which subtracts two terms ~ 1 for
                     x << 0): the reference of tests/test_gpu_hvp_sweep.py, held to mpmath in tests/test_hvp_reference.py
  curvature_mp       the defining formula in mpmath at enough digits for its own cancellation
  curvature_branches the branch formulas of pgl_curvature (csrc/pglm_hvp.hip.h) in numpy float64 with libm's exp / log:
                     what those formulas can reach in f64, the yardstick of the device's curvature grid
  ref_hvp            F^T (c o (F v)) per neuron with curvature_stable
"""
import numpy as np

LN_1EM2 = np.log(1.0e-2)


def curvature_stable(x, s, kind, dt):
    """c = -dt lam''(x) + s (log lam)''(x), elementwise.  explinear, with e = e^-|x| and lam = log1p(e^x):
         lam'' = e / (1 + e)^2
         x >= 0: (log lam)'' = (e lam - 1) / ((1 + e)^2 lam^2),  lam = x + log1p(e)       (e lam <= log 2: no cancellation)
         x <  0: (log lam)'' = e (lam - e) / ((1 + e)^2 lam^2),  lam = log1p(e); lam - e = -e^2 / 2 + e^3 / 3 - ..  cancels:
                 for e < 0.1 by the series lam = e l(e), lam - e = -e^2 q(e) / 2  (25 terms: 0.1^25 / 25 << 2^-53 of the
                 leading term; the alternating terms decrease tenfold: no cancellation), else directly (the difference
                 keeps e / 2 >= 0.05 of its terms: 20 * 2^-53 relative).
       exp: c = -dt e^min(x, 709) (the header's clamp)."""
    x = np.asarray(x, dtype=float)
    s = np.asarray(s, dtype=float)
    if kind == 'exp':
        return -dt * np.exp(np.minimum(x, 709.0))
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        xa = np.minimum(np.abs(x), 1.7976931348623157e308)          # (x = +-inf: the limits c = 0, not 0 * inf)
        e = np.exp(-xa)
        i2 = 1.0 / ((1.0 + e) * (1.0 + e))
        lam_p = xa + np.log1p(e)
        h_pos = i2 * (e * lam_p - 1.0) / (lam_p * lam_p)
        lam_n = np.log1p(e)
        h_mid = e * i2 * (lam_n - e) / (lam_n * lam_n)
        l = np.zeros_like(e)
        q = np.zeros_like(e)
        for k in range(25, -1, -1):                       # l = sum (-e)^k / (k + 1), q = sum 2 (-e)^k / (k + 2)
            l = 1.0 / (k + 1) - e * l
            q = 2.0 / (k + 2) - e * q
        h_ser = -0.5 * e * i2 * q / (l * l)
        h = np.where(x >= 0.0, h_pos, np.where(e < 0.1, h_ser, h_mid))
        c = -dt * e * i2 + np.where(s > 0.0, s * h, 0.0)
    return np.where(np.isnan(x), x, c)


def curvature_mp(x, s, kind, dt, dps=None):
    """The defining formula at `dps` digits (default: 60 + the digits its cancellation at x << 0 eats, |x| / ln 10 twice
    over).  Returns an mpmath number; x finite."""
    import mpmath as mp
    dps = int(60 + 2 * min(abs(x), 800.0) / np.log(10.0)) if dps is None else dps
    with mp.workdps(dps):
        xm, sm, dtm = mp.mpf(float(x)), mp.mpf(float(s)), mp.mpf(float(dt))
        if kind == 'exp':
            return -dtm * mp.exp(min(xm, mp.mpf(709)))
        sig = 1 / (1 + mp.exp(-xm))
        lam = mp.log(1 + mp.exp(xm))
        return +(-dtm * sig * (1 - sig) + sm * (sig * (1 - sig) / lam - sig ** 2 / lam ** 2))


def branch(x, s, kind):
    """Which formula of pgl_curvature an element takes: 'exp', 'rate' (explinear without a spike), 'pos' (x >= 0),
    'mid' (e^-|x| >= 1e-2), 'series'."""
    if kind == 'exp':
        return 'exp'
    if not s > 0:
        return 'rate'
    if x >= 0:
        return 'pos'
    return 'series' if np.exp(-abs(x)) < 1.0e-2 else 'mid'


def curvature_branches(x, s, kind, dt):
    """pgl_curvature's own formulas, operation for operation, in numpy float64 (scalars or arrays)."""
    x = np.asarray(x, dtype=float)
    s = np.asarray(s, dtype=float)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        if kind == 'exp':
            c = -dt * np.exp(np.minimum(x, 709.0))
            return np.where(np.isnan(x), x, c)
        xc = np.minimum(x, 1.7976931348623157e308)
        e = np.exp(-np.abs(xc))
        u = 1.0 + e
        inv = 1.0 / u
        i2 = inv * inv
        c = -dt * e * i2
        lam = xc + (np.log(u) + (e - (u - 1.0)) * inv)
        rl = 1.0 / lam
        h_pos = i2 * (e * lam - 1.0) * rl * rl
        l = np.full_like(e, 0.1)
        q = np.full_like(e, 2.0 / 11.0)
        for k in range(8, -1, -1):
            l = -e * l + 1.0 / (k + 1)
            q = -e * q + 2.0 / (k + 2)
        rs = 1.0 / l
        h_ser = -0.5 * e * i2 * q * rs * rs
        lam_m = np.log(u) + (e - (u - 1.0)) * inv
        rm = 1.0 / lam_m
        h_mid = e * i2 * (lam_m - e) * rm * rm
        h = np.where(xc >= 0.0, h_pos, np.where(e < 1.0e-2, h_ser, h_mid))
        c = np.where(s > 0.0, s * h + c, c)
    return np.where(np.isnan(x), x, c)


def feature_rows(fS, fstim, Weff_col, t_lo, t_hi):
    """f_t = [1, fstim[t, :], Weff[n', n] fS[t, n', b]] over the bins [t_lo, t_hi), (bins, P)"""
    nT, N, B = fS.shape
    cols = [np.ones((t_hi - t_lo, 1))]
    if fstim is not None and fstim.shape[1] > 0:
        cols.append(fstim[t_lo:t_hi])
    cols.append((fS[t_lo:t_hi] * Weff_col[None, :, None]).reshape(t_hi - t_lo, N * B))
    return np.hstack(cols)


def ref_hvp(fS, fstim, S, Weff, theta_rows, V, neurons, kind, dt, t_lo, t_hi):
    """Row i: H_n . V[i] for n = neurons[i] at theta_rows[i], with the per-bin currents and curvatures and the first-order
    bound sum_t |f_tk| |c_t| (|f_t| . |v|) of every component.  Returns (Hv, absHv, x list, spike list)."""
    out = np.zeros((len(neurons), V.shape[1]))
    absout = np.zeros_like(out)
    xs, ss = [], []
    for i, n in enumerate(neurons):
        F = feature_rows(fS, fstim, Weff[:, n], t_lo, t_hi)
        x = F.dot(theta_rows[i])
        s = S[t_lo:t_hi, n].astype(float)
        c = curvature_stable(x, s, kind, dt)
        out[i] = F.T.dot(c * F.dot(V[i]))
        aF = np.abs(F)
        absout[i] = aF.T.dot(np.abs(c) * aF.dot(np.abs(V[i])))
        xs.append(x)
        ss.append(s)
    return out, absout, xs, ss


# ---- the curvature grid of tests/test_gpu_hvp_curvature.py -----------------------------------------------------------
GRID_S = (0, 1, 3, 255)
DBL_MIN = 2.2250738585072014e-308


def curvature_grid():
    """The biases of the grid: finite ones (in order), then +inf, -inf, NaN."""
    import mpmath as mp
    with mp.workdps(60):
        true = mp.log(mp.mpf(1) / 100)
        a = float(true)
        lo, hi = (a, np.nextafter(a, 0.0)) if mp.mpf(a) <= true else (np.nextafter(a, -np.inf), a)
    assert LN_1EM2 in (lo, hi)
    one = 30.0                                            # the first x with 1 + e^-x == 1 in f64: bisection on doubles
    top = 40.0
    assert 1.0 + np.exp(-one) != 1.0 and 1.0 + np.exp(-top) == 1.0
    while np.nextafter(one, top) < top:
        mid = 0.5 * (one + top)
        if 1.0 + np.exp(-mid) == 1.0:
            top = mid
        else:
            one = mid
    finite = [-745.0, -700.0, -40.0, -20.0, lo, hi, -1.0, -1e-300, -0.0, 0.0, 1e-300, 1.0, 12.0, top, 700.0, 709.0,
              np.nextafter(709.0, np.inf), 710.0, 1e308]
    return np.array(finite + [np.inf, -np.inf, np.nan])


def grid_cpu_error(dt):
    """Worst relative error of curvature_branches (numpy f64, libm) against mpmath over the finite grid values whose exact
    c is a normal double, per branch: {branch: error}."""
    b = curvature_grid()
    b = b[np.isfinite(b)]
    worst = {}
    for kind in ('explinear', 'exp'):
        for s in GRID_S:
            got = curvature_branches(b, np.full(len(b), float(s)), kind, dt)
            for x, g in zip(b, got):
                c = curvature_mp(x, s, kind, dt)
                if abs(c) < DBL_MIN:
                    continue
                k = branch(x, s, kind)
                worst[k] = max(worst.get(k, 0.0), float(abs((g - c) / c)))
    return worst
