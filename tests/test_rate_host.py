"""The rate-window rule of csrc/pglm_ratewin.h, built for the host with gcc (tests/csrc/ratewin_host.c), against the numpy
statement of tests/rate_reference.py: the four moment planes to the bit (the M2 step is a fused multiply-add on both sides),
the pit to 1e-13, the NaN rules, draw 0 as the initialiser, and the constants the header, the binding and the public header
state."""
import os
import re

import numpy as np

from tests import rate_reference as R

ROOT = R.ROOT


def _same(acc, ref):
    assert np.array_equal(np.isnan(acc), np.isnan(ref))
    ok = ~np.isnan(ref[0])
    for k in range(4):
        assert np.array_equal(acc[k][ok], ref[k][ok]), "plane %d differs from the numpy statement" % k
    fin = ~np.isnan(ref[4])
    assert np.all(np.abs(acc[4][fin] - ref[4][fin]) <= 1e-13 * np.abs(ref[4][fin]))


def test_constants_agree():
    L = R.lib()
    assert L.rw_planes() == R.NACC == 5 and L.rw_max_count() == R.MAX_COUNT == 1024 and L.rw_max_lam() == R.MAX_LAM == 700.0
    from theano_pyglm_amd import _lib
    assert (_lib.RW_NACC, _lib.RW_MAX_COUNT, _lib.RW_MAX_LAM) == (R.NACC, R.MAX_COUNT, R.MAX_LAM)
    src = open(os.path.join(ROOT, 'include', 'pyglm_hip.h')).read()
    assert re.search(r'#define PGL_RW_NACC 5\b', src) and re.search(r'#define PGL_RW_MAX_COUNT 1024\b', src)
    for name in ('pgl_rate_windows_count', 'pgl_rate_windows_dev', 'pgl_rate_windows'):
        assert name in _lib.SYMBOLS and re.search(r'\bint %s\(' % name, src)


def test_midp_is_the_numpy_statement():
    rng = np.random.default_rng(1)
    lam = np.concatenate((np.exp(rng.uniform(-8.0, np.log(700.0), size=300)), [0.0, 700.0, 1e-300]))
    y = np.concatenate((rng.poisson(np.minimum(lam[:300], 600.0)), [0, 1024, 2])).astype(float)
    u, ref = R.host_midp(lam, y), R.midp(lam, y)
    assert np.all(np.isfinite(u)) and np.all((u > 0.0) & (u <= 1.0))
    assert np.all(np.abs(u - ref) <= 1e-15)
    # the limits: a mean above 700 or a count above 1024 has no value; the bounds themselves have one
    assert np.isnan(R.host_midp([700.0000001, 5.0, np.inf], [3.0, 1025.0, 0.0])).all()
    assert np.isfinite(R.host_midp([700.0, 5.0], [700.0, 1024.0])).all()


def test_fold_against_the_numpy_statement():
    rng = np.random.default_rng(12)
    S = 25
    mu = np.exp(rng.uniform(-4.0, 6.0, size=(6, 5)))
    lam = mu[None] * np.exp(0.3 * rng.standard_normal((S, 6, 5)))
    y = rng.poisson(mu).astype(float)
    y[0, 0] = 0.0
    acc = R.host_fold(lam, y)
    _same(acc, R.fold_numpy(lam, y))
    assert np.all(acc[1] >= 0.0) and np.all(acc[2] <= acc[0]) and np.all(acc[0] <= acc[3])
    # draw 0 initialises: the state before it does not matter
    assert np.array_equal(R.host_fold(lam, y, garbage=False), acc)
    # folding one draw at a time is the run
    st = np.full((R.NACC, y.size), 7.0)
    yy = np.ascontiguousarray(y)
    for s in range(S):
        R.lib().rw_fold(np.ascontiguousarray(lam[s]).ctypes.data, yy.ctypes.data, y.size, s, st.ctypes.data)
    assert np.array_equal(st.reshape(acc.shape), acc)
    # equal values: M2 = 0 exactly, mean = min = max
    eq = R.host_fold(np.full((9, 3), 4.25), np.array([0.0, 4.0, 11.0]))
    assert np.all(eq[0] == 4.25) and np.all(eq[1] == 0.0) and np.all(eq[2] == 4.25) and np.all(eq[3] == 4.25)
    assert np.all(np.abs(eq[4] - R.midp(np.full(3, 4.25), [0.0, 4.0, 11.0])) <= 1e-15)


def test_nan_rules():
    rng = np.random.default_rng(4)
    lam = np.exp(rng.uniform(0.0, 3.0, size=(12, 7)))
    y = rng.poisson(lam[0]).astype(float)
    clean = R.host_fold(lam, y)
    assert np.all(np.isfinite(clean))
    # a non-finite Lam (NaN, +inf, at draw 0 and later): all five planes of that element NaN for good, nothing else moves
    bad = lam.copy()
    bad[5, 1], bad[0, 2], bad[11, 3] = np.nan, np.inf, np.nan
    acc = R.host_fold(bad, y)
    _same(acc, R.fold_numpy(bad, y))
    assert np.all(np.isnan(acc[:, 1:4])) and np.array_equal(acc[:, [0, 4, 5, 6]], clean[:, [0, 4, 5, 6]])
    # Lam > 700 in one draw, or a count above 1024: the pit of that element stays NaN, its four moment planes are the clean
    # ones; the other elements are untouched
    big = lam.copy()
    big[3, 4] = 700.5
    acc = R.host_fold(big, y)
    _same(acc, R.fold_numpy(big, y))
    assert np.isnan(acc[4, 4]) and np.all(np.isfinite(acc[:4, 4])) and acc[3, 4] == 700.5
    assert np.array_equal(np.delete(acc, 4, axis=1), np.delete(clean, 4, axis=1))
    y2 = y.copy()
    y2[6] = 1025.0
    acc = R.host_fold(lam, y2)
    assert np.isnan(acc[4, 6]) and np.array_equal(acc[:4], clean[:4]) and np.array_equal(acc[4, :6], clean[4, :6])
