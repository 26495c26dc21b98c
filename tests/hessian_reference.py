"""The case table of the dense-Hessian sweep (tests/hessian_cases.json) and its float64 reference (test infrastructure, no
GPU): tests/test_hessian_cases.py keeps the table honest on the CPU, tests/test_gpu_hessian_sweep.py runs it on the device.

Reference: H_ref = F^T (c o F) over the bins of the time range, F = tests/test_hvp_host.features on a DIRECT time-domain
convolution of the spikes (oracle.convolve_with_basis: the FFT of helpers.Problem.fS leaves ~1e-17 where the feature is
exactly 0, which an elementwise bound cannot take), c = hvp_reference.curvature_stable(F theta) with the current F theta
summed in numpy.longdouble: |c'(x) / c(x)| ~ 1 for both nonlinearities, so an absolute error of x is a relative error of
c that gamma has no term for, and an element that a single bin dominates inherits it whole (a float64 dot product over the
721 columns of the N = 144 cases moves c by up to 4.1e-14 of itself: a fifth of CURV_REL, kept out of the reference).

Bounds, per neuron:  max|H_dev - H_ref| <= 1e-9 max|H_ref|  (the project's own for second-order quantities), and per element
  |H_dev[i,j] - H_ref[i,j]| <= gamma A[i,j],   A = |F|^T (|c| o |F|),   A[i,j] == 0  =>  H_dev[i,j] == 0 exactly,
  gamma = (bins + 4) 2^-53 + CURV_REL:
    (bins + 4) 2^-53  the worst case of a float64 sum of `bins` terms in ANY order ((bins - 1) u to first order, u = 2^-53),
                      and four more roundings per term: c f_i, (c f_i) f_j, and Weff on either side of the device's sum;
    CURV_REL          the relative error tests/test_gpu_hvp_curvature.py allows the device's c against mpmath: 32 times the
                      worst error of the branch formulas in numpy float64 on its grid, 32 x 6.90e-15 (its docstring;
                      test_hessian_cases.py holds CURV_REL to that test's own limit where mpmath is importable).
  Nothing in gamma is read off k_hess's output."""
import json
import os

import numpy as np

from oracle import glm_oracle as O
from tests import helpers as H
from tests import hvp_reference as R
from tests.test_hvp_host import features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'hessian_cases.json')
FIELDS = ('name', 'N', 'B', 'R', 'Dstim', 'nT', 'kind', 'rate_hz', 'burst', 'silent', 'range', 'list', 't_lo', 't_hi',
          'seed', 'kernel', 'launches', 'hits')
TOL = 1e-9
U = 2.0 ** -53
CURV_REL = 32 * 6.90e-15
CAP = 16                       # PGL_CAP: staged events per (tile, presynaptic neuron)


def load_cases():
    with open(CASES) as f:
        cases = json.load(f)
    for c in cases:
        assert sorted(c) == sorted(FIELDS), (c.get('name'), sorted(set(c) ^ set(FIELDS)))
    return cases


def basis(B, R):
    """R taps of the first B of eight columns: the interpolated standard_glm basis (5), then the spatiotemporal one (3,
    without its 1 / dt_max)."""
    return np.ascontiguousarray(np.hstack((H.std_ibasis(R), H.st_ibasis(R) * (R * 0.001)))[:, :B])


def gamma_sum(bins):
    return (bins + 4) * U


def gamma(bins):
    return gamma_sum(bins) + CURV_REL


def neurons(c):
    """the evaluated neurons in the order of the call: a range, or a seeded non-contiguous list of c['list'] neurons"""
    if c['list']:
        ids = np.random.RandomState(700 + c['seed']).permutation(c['N'])[:c['list']]
        assert np.any(np.diff(ids) != 1)
        return ids
    return np.arange(c['range'][0], c['range'][1])


def time_range(c):
    return c['t_lo'], (c['nT'] if c['t_hi'] is None else c['t_hi'])


def problem(c):
    """helpers.Problem of the case (weighted Weff: half of it exact zeros), then
       burst:  [neurons, p]: the first `neurons` neurons spike in alternating stretches of 2 R bins, Poisson(p) counts per bin
               in the odd ones on top of the base rate (windows above AND below the staging's capacity);
       silent: the listed neurons never spike.
    The features are the direct convolution (module docstring)."""
    kw = {} if c['kind'] == 'explinear' else {'bias_mu': 1.0, 'w_scale': 0.05}
    p = H.Problem(c['N'], c['nT'], basis(c['B'], c['R']), kind=c['kind'], rate_hz=c['rate_hz'], Dstim=c['Dstim'],
                  seed=c['seed'], weighted=True, **kw)
    S = p.S.copy()
    if c['burst']:
        nb, pb = c['burst']
        rng = np.random.default_rng(1000 + c['seed'])
        on = ((np.arange(c['nT']) // (2 * c['R'])) % 2 == 1)
        extra = rng.poisson(pb, size=(c['nT'], nb)) * on[:, None]
        S[:, :nb] = np.minimum(S[:, :nb].astype(int) + extra, 10).astype(np.uint8)
    for n in c['silent']:
        S[:, n] = 0
    p.S = S
    p._fS = O.convolve_with_basis(S.astype(float), p.ibasis)
    return p


def window_counts(S, R):
    """Events per (16-bin tile, presynaptic neuron) as the handle's wlo / whi windows count them: an event (a bin with a
    spike) at s belongs to tile k when its taps s + 1 .. s + R overlap the tile's bins: 16 k - R <= s < 16 k + 15."""
    nT = S.shape[0]
    cs = np.vstack((np.zeros((1, S.shape[1]), dtype=int), np.cumsum(S > 0, axis=0)))       # events in bins < k
    tiles = np.arange((nT + 15) // 16)
    lo = np.clip(16 * tiles - R, 0, nT)
    hi = np.clip(16 * tiles + 15, 0, nT)
    return cs[hi] - cs[lo]


def ref_hessian(p, ids, t_lo=0, t_hi=None, dtype=np.float64):
    """(H_ref, A) of the listed neurons over [t_lo, t_hi), (len(ids), P, P) each; dtype = numpy.longdouble sums the same
    float64 products' factors in extended precision (c stays the float64 curvature)."""
    t_hi = p.nT if t_hi is None else t_hi
    Hr = np.empty((len(ids), p.P, p.P), dtype=dtype)
    A = np.empty((len(ids), p.P, p.P))
    for i, n in enumerate(ids):
        F = features(p, n)
        F = F[t_lo:t_hi]
        x = (F.astype(np.longdouble) @ p.theta[n].astype(np.longdouble)).astype(float)       # (see the module docstring)
        c = R.curvature_stable(x, p.S[t_lo:t_hi, n].astype(float), p.kind, p.dt)
        Fx, cx = F.astype(dtype), c.astype(dtype)
        Hr[i] = Fx.T @ (cx[:, None] * Fx)
        aF = np.abs(F)
        A[i] = aF.T @ (np.abs(c)[:, None] * aF)
    return Hr, A


def check(Hd, Hr, A, bins, label):
    """The three assertions of the module docstring on (rows, P, P) arrays, and bit-for-bit symmetry; returns (worst of
    max|dH| / max|H_ref| over the rows, worst |dH| / (gamma A) over the elements with A > 0)."""
    assert Hd.shape == Hr.shape, (label, Hd.shape, Hr.shape)
    assert np.all(np.isfinite(Hd)), "%s: %d elements not finite (never written?)" % (label, np.sum(~np.isfinite(Hd)))
    assert np.array_equal(Hd, Hd.transpose(0, 2, 1)), label + ": the two triangles differ"
    d = np.abs(Hd - Hr)
    glob = float(np.max(d.max(axis=(1, 2)) / np.abs(Hr).max(axis=(1, 2))))
    zero = A == 0.0
    bad0 = np.argwhere(zero & (Hd != 0.0))
    assert len(bad0) == 0, "%s: %d elements with A == 0 are not exactly 0, first (row, i, j) %s = %r" % (
        label, len(bad0), bad0[0].tolist(), Hd[tuple(bad0[0])])
    ratio = np.where(zero, 0.0, d / np.where(zero, 1.0, gamma(bins) * A))
    elem = float(ratio.max())
    w = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s: max|dH| / max|H_ref| %.3e, worst |dH| / (gamma A) %.3e (gamma %.3e, %d bins) at (row %d, %d, %d): H_ref %.3e, A %.3e"
          % (label, glob, elem, gamma(bins), bins, w[0], w[1], w[2], Hr[w], A[w]))
    assert elem <= 1.0, "%s: element (row %d, %d, %d): |dH| = %.3e > gamma A = %.3e (H_ref %.6e, H_dev %.6e)" % (
        label, w[0], w[1], w[2], d[w], gamma(bins) * A[w], Hr[w], Hd[w])
    assert glob <= TOL, "%s: %.3e of max|H_ref|" % (label, glob)
    return glob, elem
