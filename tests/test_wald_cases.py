"""The Wald rule of a coupling group without a GPU: the numpy statement (inference/connectivity.py: wald_groups) and the gcc
build of csrc/pglm_wald.h (tests/csrc/wald_host.c) agree bit for bit on every case of tests/wald_cases.json; both meet the
longdouble reference (tests/wald_reference.py); the Benjamini-Hochberg rule; coupling_tests' host algebra; the new symbols
and the kernels' resources."""
import os

import numpy as np
import pytest

from tests import wald_reference as WR

needs_ld = pytest.mark.skipif(not WR.LD_IS_WIDER, reason="numpy.longdouble is float64 here")
CASES = WR.load()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_numpy_statement_and_gcc_mirror_agree_bit_for_bit(case):
    from theano_pyglm_amd.inference.connectivity import wald_groups
    d = WR.make_case(case)
    a = (d['W'], d['theta'], case['first'], case['G'], case['B'], d['c'])
    out_h, u_h = WR.host_wald(*a, info=d['info'], want_u=True)
    out_n, u_n = wald_groups(*a, info=d['info'], want_u=True)
    assert WR.same_bits(out_h, out_n) and WR.same_bits(u_h, u_n)
    assert WR.same_bits(WR.host_wald(*a, info=d['info']), out_h)                 # (without u: the same statistics)
    M, G, B, first = case['M'], case['G'], case['B'], case['first']
    for m in range(M):
        if d['info'][m] != 0:
            assert np.all(np.isnan(out_h[m])) and np.all(np.isnan(u_h[m::M]))
            continue
        for g in range(G):
            want = WR.expected_info(case, m, g)
            assert out_h[m, g, 3] == want
            if want:
                assert np.all(np.isnan(out_h[m, g, :3]))
            else:
                assert np.all(np.isfinite(out_h[m, g])) and out_h[m, g, 0] >= 0.0 and out_h[m, g, 2] > 0.0
            o = first + g * B
            assert np.all(u_h[g * M + m, o + B:] == 0.0)                         # whole rows, zeros included
    # the rows without the failed one: the bits of the call with it
    keep = np.nonzero(d['info'] == 0)[0]
    if keep.size < M:
        out_k, u_k = WR.host_wald(d['W'][keep], d['theta'][keep], first, G, B, d['c'], want_u=True)
        assert WR.same_bits(out_k, out_h[keep])
        assert WR.same_bits(u_k.reshape(G, keep.size, -1), u_h.reshape(G, M, -1)[:, keep])


@pytest.mark.parametrize('case', [c for c in CASES if c['G'] > 1], ids=[c['name'] for c in CASES if c['G'] > 1])
def test_a_group_alone_or_among_others(case):
    d = WR.make_case(case)
    G, B, first, M = case['G'], case['B'], case['first'], case['M']
    out, u = WR.host_wald(d['W'], d['theta'], first, G, B, d['c'], info=d['info'], want_u=True)
    for g in sorted(set([0, G // 2, G - 1])):
        o1, u1 = WR.host_wald(d['W'], d['theta'], first + g * B, 1, B, d['c'], info=d['info'], want_u=True)
        assert WR.same_bits(o1[:, 0], out[:, g]) and WR.same_bits(u1, u[g * M:(g + 1) * M])


def _worst_ratios():
    worst = [0.0, 0.0, 0.0]
    for case in CASES:
        d = WR.make_case(case)
        out = WR.host_wald(d['W'], d['theta'], case['first'], case['G'], case['B'], d['c'], info=d['info'])
        for m in range(case['M']):
            for g in range(case['G']):
                if d['info'][m] != 0 or WR.expected_info(case, m, g):
                    continue
                ref = WR.reference_group(d['W'][m], d['theta'][m], case['first'] + g * case['B'], case['B'], d['c'])
                if case.get('zero_w') == [m, g]:
                    assert out[m, g, 0] == 0.0 and ref['T'] == 0
                    continue
                r = WR.ratios(out[m, g], ref, case['P'])
                worst = [max(a, b) for a, b in zip(worst, r)]
    return worst


@needs_ld
def test_mirror_meets_the_longdouble_bound_on_every_case():
    rT, rV, rL = _worst_ratios()
    c = WR.table()['measured_c']
    print("worst err / (P u kappa |value|): T %.3e var %.3e (measured_c %.3e);  lin: %.3f of B u sum|c w|" % (rT, rV, c, rL))
    assert 0.0 < c < 1.0                         # (a bound of the form c P u kappa with c above 1 would hold nothing)
    assert max(rT, rV) <= 4.0 * c
    assert rL <= 1.0


@needs_ld
def test_quadratic_form_against_brute_force_inverse():
    """T of every group against w_g^T inv(cov[g, g]) w_g with cov the longdouble inverse of a random SPD A, through the
    factor W = chol(cov) as the Laplace route forms it.  W is cov's factor rounded to double: S = W_g W_g^T differs from
    cov[g, g] by P u |cov|, the quadratic form by that times kappa_2: the bound is 64 P u kappa_2(cov[g, g]) relative (the
    constant of tests/test_gpu_laplace_device.py)."""
    rng = np.random.default_rng(21)
    P, B, first, G = 19, 3, 1, 6
    X = rng.normal(size=(60, P))
    A = X.T.dot(X) / 60.0 + 0.1 * np.eye(P)
    cov = WR.ld_inverse_spd(A.astype(WR.LD))
    W = np.asarray(WR.ld_cholesky(cov), dtype=np.float64)[None]
    theta = rng.normal(size=(1, P))
    c = rng.normal(size=B)
    out = WR.host_wald(W, theta, first, G, B, c)
    for g in range(G):
        o = first + g * B
        blk = cov[o:o + B, o:o + B]
        w = theta[0, o:o + B].astype(WR.LD)
        T = float(np.dot(w, WR.ld_solve_spd(blk, w)))
        kappa = np.linalg.cond(blk.astype(np.float64))
        assert abs(out[0, g, 0] - T) <= 64.0 * P * WR.U * kappa * T
        var = float(np.dot(c.astype(WR.LD), blk.dot(c.astype(WR.LD))))
        assert abs(out[0, g, 2] - var) <= 64.0 * P * WR.U * kappa * var


def test_zero_weights_and_equal_rows():
    by = dict((c['name'], c) for c in CASES)
    c = by['zero_weights']
    d = WR.make_case(c)
    out = WR.host_wald(d['W'], d['theta'], c['first'], c['G'], c['B'], d['c'])
    m, g = c['zero_w']
    assert out[m, g, 0] == 0.0 and out[m, g, 1] == 0.0 and out[m, g, 2] > 0.0 and out[m, g, 3] == 0.0
    c = by['equal_rows']
    d = WR.make_case(c)
    out, u = WR.host_wald(d['W'], d['theta'], c['first'], c['G'], c['B'], d['c'], want_u=True)
    m, g = c['equal_rows']
    assert out[m, g, 3] == 2.0 and np.all(np.isnan(out[m, g, :3]))
    others = np.ones(out.shape[:2], dtype=bool)
    others[m, g] = False
    assert np.all(np.isfinite(out[others])) and np.all(out[others][:, 3] == 0.0)
    o = c['first'] + g * c['B']
    assert np.all(np.isnan(u[g * c['M'] + m, :o + 1])) and np.all(u[g * c['M'] + m, o + c['B']:] == 0.0)


# ---- Benjamini-Hochberg -------------------------------------------------------------------------------------------------
def test_benjamini_hochberg_by_hand_and_against_scipy():
    from scipy.stats import false_discovery_control
    from theano_pyglm_amd.inference.connectivity import benjamini_hochberg
    # n = 5: p_(i) n / i = 0.005, 0.02, 0.05, 0.05, 0.5 -> running minimum from the right: the same
    p = np.array([0.04, 0.001, 0.5, 0.008, 0.03])
    q = benjamini_hochberg(p)
    assert np.allclose(q, [0.05, 0.005, 0.5, 0.02, 0.05], rtol=1e-15, atol=0.0)
    # a later smaller ratio pulls the earlier ones down: p n / i = 0.04, 0.03, 0.03 -> 0.03, 0.03, 0.03
    assert np.allclose(benjamini_hochberg([0.02, 0.01 * 4 / 3, 0.03]), [0.03, 0.03, 0.03], rtol=1e-15, atol=0.0)
    # NaNs are not members of the family
    pn = np.array([[0.04, np.nan, 0.001], [0.5, 0.008, np.nan], [np.nan, 0.03, np.nan]])
    qn = benjamini_hochberg(pn)
    assert np.array_equal(np.isnan(qn), np.isnan(pn))
    assert np.allclose(qn[~np.isnan(pn)], benjamini_hochberg(pn[~np.isnan(pn)]), rtol=0, atol=0)
    assert np.allclose(np.sort(qn[~np.isnan(pn)]), np.sort(q), rtol=1e-15, atol=0.0)
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 400):
        v = rng.uniform(size=n) ** 3
        v[rng.integers(0, n, size=n // 4)] = v[0]                                  # ties
        assert np.allclose(benjamini_hochberg(v), false_discovery_control(v, method='bh'), rtol=1e-14, atol=0.0)
    assert benjamini_hochberg(np.array([])).shape == (0,)


# ---- coupling_tests' host algebra ---------------------------------------------------------------------------------------
def test_host_algebra_p_q_z_and_the_diagonal():
    from scipy.stats import chi2
    from theano_pyglm_amd.inference.connectivity import tests_from_statistics, benjamini_hochberg
    rng = np.random.default_rng(9)
    M, N, B, n_lo = 3, 5, 4, 1
    out = np.zeros((M, N, 4))
    out[..., 0] = rng.chisquare(B, size=(M, N)) * rng.choice([1.0, 6.0], size=(M, N))
    out[..., 1] = rng.normal(size=(M, N))
    out[..., 2] = rng.uniform(0.5, 2.0, size=(M, N))
    out[2, 3] = (np.nan, np.nan, np.nan, 2.0)                                      # a group that failed
    r = tests_from_statistics(out, B, n_lo=n_lo, alpha=0.1)
    assert r['dof'] == B and r['wald'].shape == (M, N)
    ok = np.isfinite(out[..., 0])
    assert np.allclose(r['p_value'][ok], chi2.sf(out[..., 0][ok], B), rtol=1e-15, atol=0) and np.isnan(r['p_value'][2, 3])
    diag = np.zeros((M, N), dtype=bool)
    diag[np.arange(M), np.arange(M) + n_lo] = True
    fam = ok & ~diag
    assert np.array_equal(np.isfinite(r['q_value']), fam)
    assert np.array_equal(r['q_value'][fam], benjamini_hochberg(r['p_value'][fam]))
    assert np.array_equal(r['significant'], fam & (np.nan_to_num(r['q_value'], nan=1.0) <= 0.1))
    assert not r['significant'][2, 3] and r['group_info'][2, 3] == 2 and np.all(r['group_info'][ok] == 0)
    assert np.allclose(r['z'][ok], out[..., 1][ok] / np.sqrt(out[..., 2][ok]), rtol=1e-15, atol=0)
    assert np.array_equal(r['weight'][ok], out[..., 1][ok]) and np.allclose(r['weight_se'][ok] ** 2, out[..., 2][ok], rtol=1e-15)
    r2 = tests_from_statistics(out, B, n_lo=n_lo, alpha=0.1, include_self=True)
    assert np.array_equal(np.isfinite(r2['q_value']), ok)
    assert np.array_equal(r2['q_value'][ok], benjamini_hochberg(r2['p_value'][ok]))
    # a row that is not positive definite: NaN throughout, not significant, not in the family
    out[0] = np.nan
    r3 = tests_from_statistics(out, B, n_lo=n_lo)
    assert np.all(np.isnan(r3['q_value'][0])) and not np.any(r3['significant'][0]) and np.all(r3['group_info'][0] == -1)


@needs_ld
def test_one_step_points_equal_the_covariance_form():
    """theta - W (W_g^T y) against theta - cov[:, g] inv(cov[g, g]) w_g in longdouble, to P u kappa: relative to |theta| +
    |step| per entry with the constant 64 of the quadratic-form test; the group's entries are exact zeros."""
    from theano_pyglm_amd.inference.connectivity import one_step_points, wald_groups
    rng = np.random.default_rng(33)
    P, B, first, G, M = 16, 3, 1, 5, 2
    W = np.zeros((M, P, P))
    theta = rng.normal(size=(M, P))
    covs = []
    for m in range(M):
        X = rng.normal(size=(50, P))
        cov = WR.ld_inverse_spd((X.T.dot(X) / 50.0 + 0.1 * np.eye(P)).astype(WR.LD))
        covs.append(cov)
        W[m] = np.asarray(WR.ld_cholesky(cov), dtype=np.float64)
    out, u = wald_groups(W, theta, first, G, B, np.ones(B), want_u=True)
    X1 = one_step_points(theta, W, u, first, G, B)
    for g in range(G):
        o = first + g * B
        for m in range(M):
            cov = covs[m]
            blk = cov[o:o + B, o:o + B]
            step = cov[:, o:o + B].dot(WR.ld_solve_spd(blk, theta[m, o:o + B].astype(WR.LD)))
            want = theta[m].astype(WR.LD) - step
            kappa = np.linalg.cond(blk.astype(np.float64)) * np.linalg.cond(np.asarray(cov, dtype=np.float64))
            row = X1[g * M + m]
            assert np.all(row[o:o + B] == 0.0)
            rest = np.ones(P, dtype=bool)
            rest[o:o + B] = False
            scale = np.max(np.abs(theta[m])) + float(np.max(np.abs(step)))
            assert float(np.max(np.abs(row[rest] - want[rest]))) <= 64.0 * P * WR.U * kappa * scale
            assert float(np.max(np.abs(want[o:o + B]))) <= 64.0 * P * WR.U * kappa * scale      # (the exact point has them at 0)


# ---- symbols, constants, resources -------------------------------------------------------------------------------------
def test_symbols_version_constants_and_resources():
    import ctypes
    import sys
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    from theano_pyglm_amd.inference import connectivity as CN
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(WR.ROOT, 'include', 'pyglm_hip.h')).read()
    for n in ('pgl_wald_groups_dev', 'pgl_wald_groups'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and 'int %s(' % n in hdr
    assert _lib.load().pgl_version() >= 116
    assert '#define PGL_WALD_MAX_B 16' in hdr and '#define PGL_WALD_NOUT 4' in hdr
    L = WR.lib()
    assert (L.wald_max_b(), L.wald_nout(), L.wald_lanes()) == (_lib.WALD_MAX_B, _lib.WALD_NOUT, CN.LANES) == (16, 4, 64)
    assert CN.MAX_B == WR.MAX_B == 16
    for m in ('wald_groups', 'wald_groups_dev', 'wald_groups_host'):
        assert hasattr(_lib.DeviceGlm, m)
    Lp = _lib.load()
    assert Lp.pgl_wald_groups_dev(None, None, 1, 8, 8, None, 1, 1, 1, None, None, None, None) == -1
    assert Lp.pgl_wald_groups(None, None, 1, 8, 8, None, 1, 1, 1, None, None, None, None) == -1
    sys.path.insert(0, os.path.join(WR.ROOT, 'tools'))
    import kernel_resources as KR
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_wald'))
    assert sorted(built) == sorted('k_wald_groups<%d>' % b for b in range(1, 17))
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0 and r['lds'] <= 65536, (n, r)


def test_detection_counts_and_the_table_text():
    from theano_pyglm_amd.inference import connectivity as CN
    N, B = 4, 5
    out = np.zeros((N, N, 4))
    out[..., 2] = 1.0
    truth = np.zeros((N, N), dtype=bool)
    truth[0, 1] = truth[2, 3] = truth[3, 0] = True
    out[..., 0] = 2.0
    out[0, 1, 0], out[2, 3, 0], out[3, 0, 0] = 60.0, 50.0, 1.0          # two found, one missed
    out[1, 2, 0] = 55.0                                                   # one false positive
    res = CN.tests_from_statistics(out, B, alpha=0.05)
    res['pd'] = np.ones(N, dtype=bool)
    d = CN.detection_counts(res, truth)
    assert (d['n'], d['positives'], d['negatives'], d['tp'], d['fp']) == (12, 3, 9, 2, 1)
    assert d['tpr'] == 2.0 / 3.0 and d['fpr'] == 1.0 / 9.0
    # ROC of T: of the 27 (present, absent) pairs 60 beats all 9 absent, 50 beats 8 (it loses to 55), 1.0 none: (9 + 8 + 0) / 27
    assert abs(d['auc'] - 17.0 / 27.0) < 1e-15
    res['lr1'] = res['wald'] + 0.5
    res['lr1_minus_wald'] = res['lr1'] - res['wald']
    text = CN.format_table(res, 0.05, truth)
    assert "3 of 12 pairs significant" in text and "true positives 2 (rate 0.667), false positives 1 (rate 0.111)" in text
    assert "median 2.500e-01, maximum 5.000e-01 over 16 pairs" in text
    assert np.isnan(CN.detection_counts(res, np.ones((N, N), dtype=bool))['auc'])       # a complete graph has no ROC
