"""The rule of the filter bands (csrc/pglm_filters.h) without a GPU: the numpy statement (inference/filters.py:
filter_bands_numpy) against the longdouble reference over tests/filter_cases.json -- order statistics equal, moments within
the measured bounds -- the coverage theorem of the simultaneous band, and excl_zero on constructed groups."""
import numpy as np
import pytest

from tests import filter_reference as FR
from theano_pyglm_amd.inference import filters as F

CASES = FR.load()
_results = {}


def _statement(c):
    if c['name'] not in _results:
        _results[c['name']] = F.filter_bands_numpy(*FR.args(c))
    return _results[c['name']]


def _groups(c):
    return [(m, g) for m in range(c['M']) for g in range(c['G'])]


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_statement_against_longdouble(c):
    d = FR.make_case(c)
    out, grp = _statement(c)
    S, R = c['n'] * c['C'], c['R']
    worst = [0.0, 0.0]
    for m, g in _groups(c):
        o, gr = out[m, g], grp[m, g]
        if FR.bad_group(c, m, g):
            assert np.all(np.isnan(o)) and np.all(np.isnan(gr[:7])) and gr[7] == 1.0
            continue
        assert gr[7] == 0.0
        w = FR.pooled_group(c, m, g)
        h = F.curves(w, np.concatenate([d['basis'], d['c'][None]], axis=0))
        fin = np.all(np.isfinite(h), axis=0)
        assert np.array_equal(np.isnan(o[:, 0]), ~fin[:R])
        # order statistics: equal
        qs, k = FR.order_statistics(h, c['level'])
        got = np.concatenate([o[:, 2:5], gr[None, 3:6]], axis=0)
        for j in range(3):
            assert FR.same_bits(got[fin, j], qs[j][fin]), (m, g, j)
        assert gr[6] == np.sum(h[:, R] > 0.0) / S
        r, dd = FR.ratios_d(h[:, :R], o)
        assert gr[0] == np.partition(dd, k - 1)[k - 1] + 0.0
        if not c.get('wide'):
            e = FR.error_ratios(o, gr, w, d['basis'], d['c'])
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    if not c.get('wide'):
        print(c['name'], "measured", worst, "stored", c['measured'])
        assert worst[0] <= max(4.0 * c['measured'][0], 4.0) and worst[1] <= max(4.0 * c['measured'][1], 4.0)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_coverage_theorem(c):
    """What the rule proves (pglm_filters.h, step 3): with r_s[tau] the rounded ratio |h_s - mean| / sd and k = ceil(level S),
    at least k draws have r_s[tau] <= c_sim at every lag with sd > 0 at once -- a share >= level -- and c_sim is at least the
    k-th smallest r_s[tau] of each such lag (never narrower than the symmetric pointwise band)."""
    d = FR.make_case(c)
    out, grp = _statement(c)
    S = c['n'] * c['C']
    for m, g in _groups(c):
        if FR.bad_group(c, m, g):
            continue
        h = F.curves(FR.pooled_group(c, m, g), d['basis'])
        r, _ = FR.ratios_d(h, out[m, g])
        k = F.band_rank(c['level'], S)
        with np.errstate(invalid='ignore'):
            inside = np.all(~(r > grp[m, g, 0]), axis=1)              # (a lag without sd > 0 or a NaN ratio does not count)
        assert inside.sum() >= k and k >= c['level'] * S and inside.sum() / S >= c['level']
        live = out[m, g][:, 1] > 0.0
        if np.any(live):
            with np.errstate(invalid='ignore'):
                kth = np.sort(np.where(np.isnan(r[:, live]), 0.0, r[:, live]), axis=0)[k - 1]
            assert np.all(grp[m, g, 0] >= kth)


def test_edge_cases_of_the_table():
    by = dict((c['name'], c) for c in CASES)
    out, grp = _statement(by['s257_const'])                          # a constant group: sd = 0 at every lag, c_sim = 0
    assert np.all(out[0, 1, :, 1] == 0.0) and grp[0, 1, 0] == 0.0 and not np.signbit(grp[0, 1, 0])
    assert np.all(out[0, 1, :, 0] == out[0, 1, :, 3]) and np.all(grp[0, [0, 2], 0] > 0.0)
    out, grp = _statement(by['s256_c4_zero_lag'])                    # a zero basis row: that lag is 0 +- 0 and does not enter d
    assert np.all(out[0, :, 3, :] == 0.0) and np.all(grp[0, :, 0] > 0.0)
    out, grp = _statement(by['s2'])                                  # ceil(level S) = S at S = 2 for level > 1/2
    assert F.band_rank(0.999, 2) == 2 and F.band_rank(0.5, 2) == 1 and F.band_rank(0.95, 1000) == 950
    c = by['s1000_c4_nan_inf']                                       # info = 1 for the two groups only
    out, grp = _statement(c)
    assert sorted(map(tuple, np.argwhere(grp[..., 7] == 1.0))) == [(1, 2), (2, 0)]
    assert np.isnan(out).sum() == 2 * c['R'] * 5
    c = by['s65_ties']                                               # duplicated draws: the quantiles are draws or between them
    out, grp = _statement(c)
    assert np.all(out[..., 2] <= out[..., 3]) and np.all(out[..., 3] <= out[..., 4])


def test_excl_zero_on_constructed_groups():
    rng = np.random.default_rng(3)
    S, B, R = 400, 3, 20
    basis = np.abs(rng.normal(size=(R, B)))
    x = np.zeros((S, 1, 1 + 2 * B))
    x[:, 0, 1:1 + B] = 5.0 + 0.1 * rng.normal(size=(S, B))           # far from 0
    x[:, 0, 1 + B:] = 0.1 * rng.normal(size=(S, B))                  # centred at 0
    out, grp = F.filter_bands_numpy(x, 1, 1, 2, basis, 0.001 * basis.sum(axis=0), 0.95)
    d = F.bands_dict(out, grp, np.arange(R))
    assert d['excl_zero'].tolist() == [[True, False]]
    assert d['p_pos'][0, 0] == 1.0 and 0.3 < d['p_pos'][0, 1] < 0.7
    assert np.all(d['c_sim'] > 1.5) and np.all(d['c_sim'] < 6.0) and d['info'].tolist() == [[0, 0]]
    with pytest.raises(ValueError):
        F.filter_bands_numpy(x, 1, 1, 2, basis, 0.001 * basis.sum(axis=0), 1.0)
    with pytest.raises(ValueError):
        F.filter_bands_numpy(x[:1], 1, 1, 2, basis, 0.001 * basis.sum(axis=0), 0.95)
