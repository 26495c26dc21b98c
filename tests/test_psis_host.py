"""PSIS-LOO without a GPU: the case table of tests/psis_reference.py reaches what it names; the float64 numpy statement of
inference/model_compare.py against the longdouble reference gives the error scale e0 recorded there; the host build of
csrc/pglm_psis.h meets the bound 100 max(e0, 1e-13), and the bound rejects three emulated defects of the numpy statement;
the reference's fit recovers the shape of exact generalized-Pareto excesses; the per-neuron algebra, the paired difference
and the table."""
import re
import os

import numpy as np
import pytest

from tests import psis_reference as R
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import model_compare as MC

IDS = [c['name'] for c in R.CASES]


def _case(name):
    return [c for c in R.CASES if c['name'] == name][0]


@pytest.mark.parametrize('c', R.CASES, ids=IDS)
def test_case_reaches_what_it_names(c):
    ll, out, lw = R.case_reference(c)
    reach = c['reach']
    n, khat = np.asarray(out[3], dtype=float), np.asarray(out[1], dtype=float)
    assert ll.shape == (c['S'], c['C'])
    if 'M' in reach:
        assert R.tail_len(c['S']) == reach['M'] == int(np.ceil(min(c['S'] / 5.0, 3.0 * np.sqrt(c['S'])))) and np.all(n == reach['M'])
    if 'fit' in reach:
        assert np.all(np.isfinite(khat)) == reach['fit'] and (reach['fit'] or np.all(khat == np.inf))
    if 'khat_above' in reach:
        assert np.all(khat > reach['khat_above'])
    if 'khat_below' in reach:
        assert np.all(khat < reach['khat_below'])
    if 'n' in reach:
        assert list(n) == reach['n'] and np.all((n >= 5) == np.isfinite(khat))
    if 'uniform' in reach:
        assert np.allclose(np.asarray(lw, dtype=float), -np.log(c['S']), atol=1e-14) and np.all(np.asarray(out[0], dtype=float) == ll[0])
    if 'tied_tail' in reach:
        # two draws of the tail with the same l: the smaller index has the lower rank, so the smaller smoothed weight
        col, w = ll[:, 0], np.asarray(lw[:, 0], dtype=float)
        tail = np.argsort(-col, kind='stable')[-int(n[0]):]
        pairs = [(a, b) for a, b in zip(tail[:-1], tail[1:]) if col[a] == col[b]]
        assert len(pairs) >= 3 and all(a < b and w[a] < w[b] for a, b in pairs)
        assert n[0] < R.tail_len(c['S'])                     # (and ties at the cutoff shortened the tail)
    if 'floor' in reach:
        x = -ll - np.max(-ll, axis=0)
        cut = np.sort(x, axis=0)[c['S'] - R.tail_len(c['S']) - 1]
        assert np.all(cut < 2.0 * float(R.LOG_DBL_MIN))      # far below the floor


def test_sizes_cross_every_threshold():
    assert [R.tail_len(S) for S in (2, 24, 25, 26, 100, 225, 226, 1024, R.MAX_DRAWS)] == [1, 5, 5, 6, 20, 45, 46, 96, 192]
    assert all(R.tail_len(S) == int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S)))) for S in range(2, 5000))
    assert all(R.lib().psis_tail(S) == R.tail_len(S) for S in list(range(2, 3000)) + [R.MAX_DRAWS, 10 ** 6, 10 ** 6 + 1])
    src = open(os.path.join(R.ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_psis.h')).read()
    pub = open(os.path.join(R.ROOT, 'include', 'pyglm_hip.h')).read()
    for text in (src, pub):
        assert int(re.search(r'#define PGL_PSIS_MAX_DRAWS (\d+)', text).group(1)) == R.MAX_DRAWS == _lib.PSIS_MAX_DRAWS >= 4096
    assert R.lib().psis_max_draws() == R.MAX_DRAWS and R.lib().psis_planes() == _lib.PSIS_NOUT == 4
    assert int(re.search(r'#define PGL_PSIS_MAX_TAIL (\d+)', src).group(1)) == R.tail_len(R.MAX_DRAWS)


def _worst(fn):
    worst = dict((q, 0.0) for q in R.QUANTITIES)
    for c in R.CASES:
        ll, out, lw = R.case_reference(c)
        o, w = fn(ll)
        e = R.errors(o, w, out, lw)
        for q in R.QUANTITIES:
            worst[q] = max(worst[q], e[q])
    return worst


def test_error_scale():
    """e0: the float64 statement against the longdouble reference over the whole table, within the recorded constants"""
    worst = _worst(lambda ll: MC.psis_loo_from_pointwise(ll, weights=True))
    print("e0 measured %s, recorded %s" % (worst, R.E0))
    for q in R.QUANTITIES:
        assert worst[q] <= R.E0[q] * 1.05, (q, worst[q])
        assert R.BOUND[q] == 100.0 * max(R.E0[q], 1e-13)


def test_host_mirror_meets_the_bound():
    worst = _worst(R.host_mirror)
    print("host mirror: worst %s, ratio to the bound %s" % (worst, dict((q, worst[q] / R.BOUND[q]) for q in R.QUANTITIES)))
    assert R.within(worst)


def test_host_mirror_non_finite_column():
    ll = R.matrix(_case('S64')).copy()
    clean, clean_lw = R.host_mirror(ll)
    for bad in (np.nan, np.inf, -np.inf):
        a = ll.copy()
        a[17, 1] = bad
        out, lw = R.host_mirror(a)
        assert np.all(np.isnan(out[:, 1])) and np.all(np.isnan(lw[:, 1]))
        assert np.array_equal(out[:, [0, 2]], clean[:, [0, 2]]) and np.array_equal(lw[:, [0, 2]], clean_lw[:, [0, 2]])
        o2 = MC.psis_loo_from_pointwise(a)
        assert np.all(np.isnan(o2[:, 1])) and np.all(np.isfinite(o2[:, [0, 2]]))


@pytest.mark.parametrize('defect', ['tail_off_by_one', 'quantiles_i_over_n', 'no_truncation'])
def test_bound_rejects_defect(defect, monkeypatch):
    if defect == 'tail_off_by_one':
        orig = MC._tail_len
        monkeypatch.setattr(MC, '_tail_len', lambda S: orig(S) + 1)
    elif defect == 'quantiles_i_over_n':
        monkeypatch.setattr(MC, '_quantiles', lambda n: np.arange(1, n + 1) / float(n))
    else:
        monkeypatch.setattr(MC, '_truncate', lambda x: x)
    caught = []
    for c in R.CASES:
        ll, out, lw = R.case_reference(c)
        with np.errstate(all='ignore'):
            o, w = MC.psis_loo_from_pointwise(ll, weights=True)
        if not R.within(R.errors(o, w, out, lw)):
            caught.append(c['name'])
    print(defect, caught)
    assert len(caught) >= 3 and 'S1000' in caught


@pytest.mark.parametrize('k', [0.1, 0.5, 0.9])
def test_reference_fit_recovers_generalized_pareto_shape(k):
    khats = []
    for seed in range(20):
        u = np.random.default_rng(1000 + seed).uniform(0.0, 1.0, 2000)
        e = np.sort(2.0 * ((1.0 - u) ** (-k) - 1.0) / k)
        khats.append(float(R.gpd_fit_ld(e)[0]))
        assert abs(MC.gpd_fit(e)[0] - khats[-1]) < 1e-9
    print(k, np.mean(khats))
    assert abs(np.mean(khats) - k) < 0.05


def _result(seed, nb=7, M=3, S=400, sd=1.0):
    rng = np.random.default_rng(seed)
    ll = -30.0 + rng.normal(0.0, 1.0, (1, nb, M)) + rng.normal(0.0, sd, (S, nb, M))
    out = MC.psis_loo_from_pointwise(ll)
    return ll, out, MC.loo_from_columns(out, MC.log_mean_exp(ll), S)


def test_loo_from_columns_algebra():
    ll, out, res = _result(3)
    nb, S = ll.shape[1], ll.shape[0]
    assert np.allclose(res['elpd_loo'], out[0].sum(axis=0), rtol=0, atol=0) and np.array_equal(res['looic'], -2.0 * res['elpd_loo'])
    assert np.allclose(res['p_loo'], (MC.log_mean_exp(ll) - out[0]).sum(axis=0), rtol=1e-15)
    assert np.allclose(res['se'], np.sqrt(nb * np.var(out[0], axis=0, ddof=1)), rtol=1e-15)
    assert np.array_equal(res['khat_max'], out[1].max(axis=0)) and np.array_equal(res['elpd_b'], out[0])
    assert np.array_equal(res['khat_b'], out[1]) and res['n_blocks'] == nb and res['n_draws'] == S
    assert res['khat_threshold'] == min(1.0 - 1.0 / np.log10(S), 0.7) and MC.khat_threshold(100) == 0.5
    forged = out.copy()
    forged[1] = 0.1
    forged[1, 2, 1] = 0.71
    forged[1, 4, 1] = np.inf
    forged[1, 0, 2] = 0.7
    assert list(MC.loo_from_columns(forged, MC.log_mean_exp(ll), 10000)['n_khat_bad']) == [0, 2, 0]      # threshold 0.7
    assert list(MC.loo_from_columns(forged, MC.log_mean_exp(ll), 100)['n_khat_bad']) == [0, 2, 1]        # threshold 0.5
    assert np.all(res['p_loo'] > 0)
    with pytest.raises(ValueError):
        MC.loo_from_columns(out, MC.log_mean_exp(ll)[1:], S)


def test_elpd_diff():
    _, _, a = _result(3)
    _, _, b = _result(4)
    d, r = MC.elpd_diff(a, b), MC.elpd_diff(b, a)
    assert np.array_equal(d['elpd_diff'], -r['elpd_diff']) and np.array_equal(d['se_diff'], r['se_diff'])
    assert np.allclose(d['elpd_diff'], a['elpd_loo'] - b['elpd_loo'], rtol=1e-12)
    assert np.allclose(d['se_diff'], np.sqrt(7 * np.var(a['elpd_b'] - b['elpd_b'], axis=0, ddof=1)), rtol=1e-15)
    z = MC.elpd_diff(a, a)
    assert np.all(z['elpd_diff'] == 0) and np.all(z['se_diff'] == 0)
    _, _, short = _result(5, nb=6)
    with pytest.raises(ValueError, match="blocks"):
        MC.elpd_diff(a, short)
    lla, _, _ = _result(3)
    llb, _, _ = _result(4)
    w = MC.elpd_diff(MC.waic_from_pointwise(lla), MC.waic_from_pointwise(llb))       # WAIC results carry elpd_b too
    assert np.allclose(w['elpd_diff'], MC.waic_from_pointwise(lla)['elpd_waic'] - MC.waic_from_pointwise(llb)['elpd_waic'], rtol=1e-12)


def test_format_table_prints_the_loo_table():
    _, _, res = _result(3)
    res.update(route='device', block_bins=512, n_lo=4)
    text = MC.format_table(res)
    print(text)
    lines = text.split("\n")
    assert lines[0] == "PSIS-LOO (400 draws, 7 blocks of 512 bins, device)"
    for word in ('elpd_loo', 'p_loo', 'looic', 'se', 'max khat', 'khat>0.62'):
        assert word in lines[1]
    assert len(lines) == 2 + 3 + 1 and lines[2].split()[0] == '4' and float(lines[2].split()[1]) == round(res['elpd_loo'][0], 3)
    assert lines[-1].startswith("total elpd_loo %.3f" % res['elpd_loo'].sum()) and "of 21 blocks above the khat threshold" in lines[-1]
    ll, _, _ = _result(3)
    wa = MC.waic_from_pointwise(ll)
    assert '--loo' in MC.format_table(wa).split("\n")[-1] and 'not implemented' not in MC.format_table(wa)
    assert 'PSIS-LOO' in MC.__doc__ and 'not implemented' not in MC.__doc__


def test_loo_agrees_with_waic_at_small_posterior_variance():
    ll, _, res = _result(11, nb=12, M=4, S=500, sd=0.05)
    wa = MC.waic_from_pointwise(ll)
    assert np.all(np.abs(res['elpd_loo'] - wa['elpd_waic']) < np.minimum(res['se'], wa['se']))
    assert np.all(res['n_khat_bad'] == 0) and np.all(wa['n_high_var'] == 0)


def test_argument_checks():
    with pytest.raises(ValueError):
        MC.psis_loo_from_pointwise(np.zeros((1, 3)))
    with pytest.raises(ValueError):
        MC.psis_loo_from_pointwise(np.zeros(5))
    for s in ('pgl_psis_loo_dev', 'pgl_psis_loo'):
        assert s in _lib.SYMBOLS
    assert _lib.ABI_VERSION >= 110
