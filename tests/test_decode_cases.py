"""The case table of stimulus decoding and its longdouble reference (tests/decode_reference.py): the table covers what the
issue of the feature lists, the reference is finite everywhere and its offset is exact, its gradient and Hessian-vector product
agree with central differences, L / L^T and K / K^T are adjoint pairs, H is symmetric, and the allowance A of the bound is what
was measured on the host mirror."""
import numpy as np
import pytest

from tests import decode_reference as DR

LD = np.longdouble


def test_table_covers_the_shapes():
    C = DR.CASES
    assert {1, 3, 17, 33} <= set(c['N'] for c in C) and any(c['N'] > 64 for c in C)
    assert set(c['nT'] for c in C) == {257, 1000, 3000}
    assert set(c['Rt'] for c in C) == {1, 5, 70}
    assert any(c['Rt'] > 64 for c in C) and any(4 * c['Rt'] > c['nT'] for c in C)
    assert set(c['D'] for c in C) == {1, 3} and set(c['B'] for c in C) == {1, 4}
    assert set(c['q'] for c in C) == {1, 4, 7}
    assert all(c['Tu'] * c['q'] != c['nT'] for c in C)
    assert any(c['Tu'] * c['q'] > c['nT'] for c in C) and any(c['Tu'] * c['q'] < c['nT'] for c in C)
    assert set(c['nlin'] for c in C) == {'exp', 'explinear'}
    assert any(c['rho'] is None for c in C) and any(c['rho'] is not None for c in C)
    assert any('silent' in c for c in C)


@pytest.mark.parametrize('name', DR.NAMES)
def test_spike_patterns_and_exact_offset(name):
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    S = m['S']
    assert S.max() >= 3 and (S == 2).any()
    assert S[0].any() and S[-1].any()
    if 'silent' in c:
        assert not S[:, c['silent']].any()
    assert np.array_equal(DR.offset_longdouble(name), m['c'].astype(LD))        # every f64 sum of the offset was exact


def test_currents_above_and_below_twelve():
    hi = [float(DR.reference(n)['x'].min()) for n in DR.NAMES if DR.BY_NAME[n]['level'] >= 15]
    lo = [float(DR.reference(n)['x'].max()) for n in DR.NAMES if DR.BY_NAME[n]['level'] <= -13]
    assert hi and min(hi) > 12.0
    assert lo and max(lo) < -12.0


@pytest.mark.parametrize('name', DR.NAMES)
def test_reference_is_finite_everywhere(name):
    ref = DR.reference(name)
    for key, val in ref.items():
        assert np.all(np.isfinite(np.asarray(val, dtype=LD))), key
    for key in ('F', 'g', 'hv1', 'hv2'):
        assert np.all(DR.bound(ref, key) > 0), key


def _direction(name, seed):
    c = DR.BY_NAME[name]
    return np.random.RandomState(seed).randn(c['Tu'], c['D']).astype(LD)


@pytest.mark.parametrize('name', DR.NAMES)
def test_gradient_against_central_differences(name):
    """<g, w> against (F(u + h w) - F(u - h w)) / 2h in longdouble, h = 1e-5: the truncation error is h^2 |F'''| / 6 ~ 1e-10 of
    the scale, the rounding error 2^-64 |F| / h ~ 1e-14 |F|; held to 1e-7 of sum |g| |w|."""
    ref = DR.reference(name)
    u = DR.make_case(name)['u'].astype(LD)
    w = _direction(name, 11)
    h = LD(1e-5)
    fd = (DR.objective_longdouble(name, u + h * w) - DR.objective_longdouble(name, u - h * w)) / (2 * h)
    an = (ref['g'] * w).sum()
    scale = (np.abs(ref['g']) * np.abs(w)).sum()
    print(name, 'fd', float(fd), 'analytic', float(an), 'rel', float(abs(fd - an) / scale))
    assert abs(fd - an) <= 1e-7 * scale


@pytest.mark.parametrize('name', DR.NAMES)
def test_hvp_against_central_differences_of_the_gradient(name):
    ref = DR.reference(name)
    m = DR.make_case(name)
    u = m['u'].astype(LD)
    h = LD(1e-5)
    for key, v in (('hv1', m['v1']), ('hv2', m['v2'])):
        v = v.astype(LD)
        fd = (DR.gradient_longdouble(name, u + h * v) - DR.gradient_longdouble(name, u - h * v)) / (2 * h)
        err = np.abs(fd - ref[key]).max()
        scale = ref[key + '_abs'].max()
        print(name, key, 'max err', float(err), 'scale', float(scale))
        assert err <= 1e-7 * scale


@pytest.mark.parametrize('name', DR.NAMES)
def test_adjoint_identities_and_symmetry(name):
    """<L a, b> = <a, L^T b>, <K * a, b> = <a, K^T b> and <H v, w> = <v, H w> in longdouble, to 1e-16 of the sum of the absolute
    products (longdouble carries 2^-64; the sums have up to ~1e6 terms)."""
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    nT, N, D, Tu, q = c['nT'], c['N'], c['D'], c['Tu'], c['q']
    rng = np.random.RandomState(77)
    a, b = rng.randn(Tu, D).astype(LD), rng.randn(nT, D).astype(LD)
    La, Ltb = DR.L_apply(a, nT, q), DR.Lt_apply(b, Tu, q)
    assert abs((La * b).sum() - (a * Ltb).sum()) <= 1e-16 * (np.abs(La) * np.abs(b)).sum()
    K = DR.filters(m['basis'], m['theta'], D)
    s, y = rng.randn(nT, D).astype(LD), rng.randn(nT, N).astype(LD)
    Ks, Kty = DR.K_apply(K, s), DR.Kt_apply(K, y)
    assert abs((Ks * y).sum() - (s * Kty).sum()) <= 1e-16 * (np.abs(DR.K_apply(np.abs(K), np.abs(s))) * np.abs(y)).sum()
    ref = DR.reference(name)
    v1, v2 = m['v1'].astype(LD), m['v2'].astype(LD)
    lhs, rhs = (ref['hv1'] * v2).sum(), (v1 * ref['hv2']).sum()
    assert abs(lhs - rhs) <= 1e-16 * (ref['hv1_abs'] * np.abs(v2)).sum()


def test_allowance_measured_on_the_mirror():
    """The worst error of the host mirror's ll term, residual and curvature over the whole table, at the mirror's own f64
    current, in units of 2^-53 times the element's absolute parts: A_MEASURED records it (rounded up), A = A_FACTOR A_MEASURED
    is what the bound grants the device."""
    worst = 0.0
    for name in DR.NAMES:
        ref = DR.reference(name)
        for key, val in zip(('term', 'r', 'cc'), DR.mirror_points(name)):
            scale = ref[key + '_abs']
            err = np.abs(val.astype(LD) - ref[key])
            ok = scale > 0
            assert np.all(err[~ok] == 0), (name, key)
            w = float((err[ok] / (LD(DR.U) * scale[ok])).max())
            print(name, key, 'worst error %.2f u' % w)
            worst = max(worst, w)
    print('worst of the table: %.2f u; recorded A_MEASURED = %d' % (worst, DR.A_MEASURED))
    assert worst <= DR.A_MEASURED
    assert DR.A == DR.A_FACTOR * DR.A_MEASURED and DR.A_FACTOR == 4
