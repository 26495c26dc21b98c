"""The independence rule without a GPU: the gcc build of csrc/pglm_acf.h (tests/csrc/acf_host.c) against the longdouble
reference over tests/acf_cases.json and against gof.acf_scores bit for bit; the new symbols, bindings and the kernel's
resources; the dry run of the recorded kernel name; the keys the KS results gained."""
import os

import numpy as np
import pytest

from tests import acf_reference as AR

needs_ld = pytest.mark.skipif(not AR.LD_IS_WIDER, reason="numpy.longdouble is float64 here")


def test_symbols_version_and_null_handles():
    import ctypes
    import sys
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(AR.ROOT, 'include', 'pyglm_hip.h')).read()
    for n in ('pgl_rescale_acf_dev', 'pgl_rescale_acf'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and 'int %s(' % n in hdr
    assert _lib.load().pgl_version() >= 115
    assert '#define PGL_ACF_MAX_LAG 64' in hdr and '#define PGL_ACF_NHEAD 6' in hdr
    for m in ('rescale_acf', 'rescale_acf_dev', 'rescale_acf_host'):
        assert hasattr(_lib.DeviceGlm, m)
    L = _lib.load()
    assert L.pgl_rescale_acf_dev(None, None, None, None, 1, 20, None, None) == -1
    assert L.pgl_rescale_acf(None, None, None, None, 1, 20, None, None) == -1
    src = open(os.path.join(AR.ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_acf.h')).read()
    for name, v in (('MAX_LAG', _lib.ACF_MAX_LAG), ('NHEAD', _lib.ACF_NHEAD), ('PIECE', _lib.ACF_PIECE)):
        assert '#define PGL_ACF_%s %d' % (name, v) in src
    assert (AR.lib().acf_max_lag(), AR.lib().acf_nhead(), AR.lib().acf_piece()) == (AR.MAX_LAG, AR.NHEAD, AR.PIECE) == \
        (_lib.ACF_MAX_LAG, _lib.ACF_NHEAD, _lib.ACF_PIECE)
    sys.path.insert(0, os.path.join(AR.ROOT, 'tools'))
    import kernel_resources as KR
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_acf'))
    print(built)
    assert sorted(built) == ['k_acf_segment']
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0 and r['lds'] <= 65536, (n, r)


def test_dry_run_records_the_kernel():
    from theano_pyglm_amd import _lib
    assert _lib.plan_kernels(8, path=10) == ['k_acf_segment']
    assert _lib.plan_kernels(32, B=5, R=200, nT=300000) == ['k_fused6<5, 2, 1, 4, 1>']        # (the others are what they were)


@needs_ld
def test_host_mirror_meets_the_bounds_on_every_case():
    for c in AR.load():
        tau = AR.case_tau(c)
        out, g = AR.host_acf(tau, [c['runs']], c['L'])
        es, er = AR.check_against_reference(c['name'], out[0], g, tau, c['runs'], c['L'])
        print("%-14s scores %.2e relative, r %.2e absolute" % (c['name'], es, er))


def test_void_rules_and_special_values():
    by = dict((c['name'], c) for c in AR.load())
    for name in ('n0', 'n1', 'n2'):
        c = by[name]
        out, _ = AR.host_acf(AR.case_tau(c), [c['runs']], c['L'])
        assert out[0, 0] == sum(c['runs']) and out[0, 4] == 0.0 and out[0, 5] == 0.0
        assert np.all(np.isnan(out[0, AR.NHEAD:])) and np.isnan(out[0, 3])
        assert np.isnan(out[0, 1]) == (name == 'n0')
    for name in ('has_nan', 'has_negative'):
        c = by[name]
        out, g = AR.host_acf(AR.case_tau(c), [c['runs']], c['L'])
        assert out[0, 0] == sum(c['runs']) and np.all(np.isnan(out[0, 1:]))
        assert np.sum(np.isnan(g)) == (1 if name == 'has_nan' else 0)        # every score is written all the same
    c = by['const4']
    out, g = AR.host_acf(AR.case_tau(c), [c['runs']], c['L'])
    assert out[0, 2] == 0.0 and out[0, 1] == g[0] and np.isnan(out[0, 3]) and out[0, 4] == 0.0
    c = by['specials']
    tau = AR.case_tau(c)
    out, g = AR.host_acf(tau, [c['runs']], c['L'])
    assert np.all(np.isfinite(g)) and np.isfinite(out[0, 3])
    for i in (3, 9, 17, 25):
        assert 37.0 < abs(g[i]) < 38.0 and (g[i] > 0) == (tau[i] > 1.0), (i, g[i])
    assert g[17] == g[25] and g[3] == g[9]                                    # the clamp
    # max_lag >= n: the lags without a pair are NaN and left out of Q
    c = by['lag_ge_n']
    out, _ = AR.host_acf(AR.case_tau(c), [c['runs']], c['L'])
    assert out[0, 4] == 9.0 and np.all(np.isnan(out[0, AR.NHEAD + 9:])) and np.all(np.isfinite(out[0, AR.NHEAD:AR.NHEAD + 9]))


def test_mirror_equals_the_numpy_statement_bit_for_bit():
    from theano_pyglm_amd.inference import gof
    for c in AR.load():
        tau = AR.case_tau(c)
        out, g = AR.host_acf(tau, [c['runs']], c['L'])
        void = [bool(np.any(~(tau >= 0.0)))]
        mine = gof.acf_from_scores([AR.split_runs(g, c['runs'])], c['L'], void)
        assert mine.tobytes() == out.tobytes(), (c['name'], mine, out)
        again = AR.host_from_scores(tau, g, [c['runs']], c['L'])
        assert again.tobytes() == out.tobytes(), c['name']
        # numpy's scores against the mirror's: libm apart
        gn = gof.normal_scores(tau)
        ok = ~np.isnan(g)
        assert np.array_equal(np.isnan(gn), ~ok)
        assert np.all(np.abs(gn[ok] - g[ok]) <= 4e-15 * np.abs(g[ok])), c['name']
        full = gof.acf_scores([AR.split_runs(tau, c['runs'])], c['L'])
        assert full[0, 0] == out[0, 0] and np.array_equal(np.isnan(full), np.isnan(out)), c['name']


def test_bits_do_not_depend_on_the_company_or_on_max_lag():
    by = dict((c['name'], c) for c in AR.load())
    c = by['runs3_short']
    tau, segs, at = AR.crowd(c)
    assert len(segs) == 301 and sum(1 for s in segs if sum(s) == 0) >= 40
    out, g = AR.host_acf(tau, segs, c['L'])
    alone, g1 = AR.host_acf(AR.case_tau(c), [c['runs']], c['L'])
    assert out[at].tobytes() == alone[0].tobytes()
    wide, _ = AR.host_acf(AR.case_tau(c), [c['runs']], 64)
    one, _ = AR.host_acf(AR.case_tau(c), [c['runs']], 1)
    assert wide[0, AR.NHEAD] == one[0, AR.NHEAD] == alone[0, AR.NHEAD]
    assert wide[0, :3].tobytes() == one[0, :3].tobytes()


def test_ks_results_gained_a_p_value_and_nothing_else_moved():
    from theano_pyglm_amd.inference import gof

    class Fake(object):
        def compute_rescaled_intervals(self, x):
            return taus, stats
    taus = [np.zeros(0), np.array([0.7]), np.array([0.7, 0.1]), np.random.default_rng(5).exponential(size=400)]
    stats = np.array([[0.5, 1, 0, 0], [1.5, 2, 0, 0], [2.5, 3, 1, 0], [390.0, 401, 3, 0]])
    res = gof.ks_time_rescaling(Fake(), None)
    assert set(res) == {'D', 'band', 'passed', 'n_intervals', 'expected_count', 'observed_count', 'multi_spike_bins', 'alpha',
                        'D_plus', 'D_minus', 'route', 'p_value'}
    assert np.isnan(res['p_value'][0]) and np.isnan(res['p_value'][1]) and res['p_value'][3] > 0.05
    for name in ('independence_time_rescaling', 'independence_time_rescaling_draws', 'acf_scores', 'ks_pvalue',
                 'format_independence_table', 'format_independence_draws_table'):
        assert hasattr(gof, name)
