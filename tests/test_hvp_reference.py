"""The float64 curvature reference of the Hessian-vector sweep (tests/hvp_reference.curvature_stable) against mpmath
over the sweep's own range of currents, the older cancelling reference of tests/test_hvp_host.py against it where that one
is well-conditioned, and what the branch formulas of pgl_curvature reach in numpy float64 on the grid of
tests/test_gpu_hvp_curvature.py.  No GPU needed."""
import numpy as np
import pytest

from tests import hvp_reference as R
from tests.test_hvp_host import curvature as curvature_old

DT = 0.001


def _sweep_currents():
    # the sweep's biases are -20 .. 20.9 (edge neurons -20, -2, 3, 12; the seeded ones 1 or 20 +- 0.3 sigma) and its
    # weights are scaled to currents within 6 of the bias: -26 .. 27, taken with a margin
    rng = np.random.default_rng(5)
    return np.concatenate((np.linspace(-30.0, 30.0, 1201), rng.uniform(-30.0, 30.0, 400), rng.uniform(-6.0, 1.0, 400),
                           [R.LN_1EM2, np.nextafter(R.LN_1EM2, 0.0), np.log(0.1), -0.0, 0.0]))


@pytest.mark.parametrize('kind', ['explinear', 'exp'])
def test_stable_curvature_is_within_1e_12_of_mpmath_per_bin(kind):
    mp = pytest.importorskip('mpmath')
    x = _sweep_currents()
    worst = 0.0
    for s in (0, 1, 2, 3, 10):
        got = R.curvature_stable(x, np.full(len(x), float(s)), kind, DT)
        for xi, g in zip(x, got):
            c = R.curvature_mp(xi, s, kind, DT, dps=80)           # (>= 40 digits left after the e^-30 cancellation)
            assert abs(c) >= R.DBL_MIN
            err = float(abs((g - c) / c))
            worst = max(worst, err)
            assert err <= 1e-12, (kind, s, xi, g, mp.nstr(c, 20), err)
    print("%s: curvature_stable against mpmath over %d currents x 5 spike counts: worst relative error %.2e"
          % (kind, len(x), worst))


def test_old_reference_agrees_where_it_is_well_conditioned():
    x = _sweep_currents()
    x = x[np.abs(x) < 3.0]
    for kind in ('explinear', 'exp'):
        for s in (0, 1, 3):
            sv = np.full(len(x), float(s))
            a, b = curvature_old(x, sv, kind, DT), R.curvature_stable(x, sv, kind, DT)
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (kind, s, float(np.max(np.abs(a - b) / np.abs(b))))
    # ... and is NOT a reference at x << 0, where it subtracts two terms ~ 1 (the reason for curvature_stable)
    a, b = curvature_old(np.array([-20.0]), np.array([1.0]), 'explinear', DT), \
        R.curvature_stable(np.array([-20.0]), np.array([1.0]), 'explinear', DT)
    assert abs(a[0] - b[0]) > 1e-10 * abs(b[0])


def test_stable_curvature_limits():
    x = np.array([np.inf, -np.inf, np.nan, 1e308, -745.0])
    for s in (0.0, 3.0):
        c = R.curvature_stable(x, np.full(5, s), 'explinear', DT)
        assert c[0] == 0.0 and c[1] == 0.0 and np.isnan(c[2]) and c[3] == 0.0 and abs(c[4]) < R.DBL_MIN
        c = R.curvature_branches(x, np.full(5, s), 'explinear', DT)
        assert c[0] == 0.0 and c[1] == 0.0 and np.isnan(c[2]) and c[3] == 0.0 and abs(c[4]) < R.DBL_MIN
    for f in (R.curvature_stable, R.curvature_branches):
        c = f(x, np.zeros(5), 'exp', DT)
        assert c[0] == c[3] == -DT * np.exp(709.0) and np.isfinite(c[0]) and c[1] == 0.0 and np.isnan(c[2])


def test_branch_formulas_in_float64_on_the_grid():
    """What pgl_curvature's formulas reach with libm in f64 on the device test's grid: the device is allowed 32 times
    this (and never more than 1e-10).  Measured here: see the print; every branch must itself stay far below 1e-10 / 32."""
    pytest.importorskip('mpmath')
    b = R.curvature_grid()
    assert len(b) == 22 and np.sum(np.isfinite(b)) == 19
    worst = R.grid_cpu_error(DT)
    print("numpy-f64 branch formulas against mpmath on the grid, worst relative error per branch: %s"
          % ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))
    assert set(worst) == {'exp', 'rate', 'pos', 'mid', 'series'}
    assert max(worst.values()) <= 1e-10 / 32.0
