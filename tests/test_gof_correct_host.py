"""The discrete-time correction and the KS rule without a GPU: the gcc build of csrc/pglm_gof.h (tests/csrc/gof_host.c)
against the longdouble references over both tables of tests/ks_cases.json; the header's uniforms against the integer
restatement; the statistical claim on the reference alone (data simulated from a known rate with lam dt = 0.2 .. 0.5: the
corrected D inside the band, the uncorrected one beyond three bands); the unchanged defaults of ks_time_rescaling; the new
symbols, bindings and keyword arguments."""
import inspect
import os

import numpy as np
import pytest

from tests import gof_reference as GR
from tests import rescale_reference as RR

T = GR.load()
SEED = 5
LD = np.longdouble
LD_IS_WIDER = np.finfo(LD).eps < np.finfo(np.float64).eps


@pytest.mark.skipif(not LD_IS_WIDER, reason="numpy.longdouble is float64 here")
def test_host_mirror_meets_the_bounds_on_both_tables():
    for c in T['corr']:
        for t_lo, t_hi, _ in GR.corr_ranges(c):
            for draw in (0, 1):
                ref = GR.corr_reference(c, t_lo, t_hi, SEED, draw)
                tau, off = GR.host_corr(c, t_lo, t_hi, SEED, draw)
                assert np.array_equal(off, RR.offsets(ref[0]))
                r = GR.corr_ratio(tau, off, ref)
                print("%-12s [%4d, %4d) draw %d: host mirror %.2e of the bound" % (c['name'], t_lo, t_hi, draw, r))
                assert r <= 1.0, (c['name'], t_lo, draw)
    for c in T['ks']:
        tau = GR.ks_tau(c)
        ks, zs = GR.host_ks(tau, np.array([0, tau.size]))
        _check(c['name'], tau, ks[0], zs)
    tau, off = GR.multi()
    ks, zs = GR.host_ks(tau, off)
    for m in range(off.size - 1):
        _check("segment %d" % m, tau[off[m]:off[m + 1]], ks[m], zs[off[m]:off[m + 1]])
    for m in (1, 4, 8, 10, 299):                                  # a segment alone: the same bits
        one, z1 = GR.host_ks(tau[off[m]:off[m + 1]], np.array([0, off[m + 1] - off[m]]))
        assert one[0].tobytes() == ks[m].tobytes() and z1.tobytes() == zs[off[m]:off[m + 1]].tobytes()


def _check(label, tau, ks, z):
    ref = GR.ks_reference(tau)
    assert ks[3] == tau.size, label
    if np.isnan(ref[0]):
        assert np.all(np.isnan(ks[:3])), label
        return
    assert np.all(np.diff(z) >= 0.0), label
    zn = np.sort(-np.expm1(-tau))
    assert np.all(np.abs(z - zn) <= 2.0 * np.spacing(zn)), label
    assert tuple(ks[:3]) == GR.ks_from_sorted(z), label           # numpy's arithmetic, bit for bit
    assert np.max(np.abs(ks[:3] - ref[:3])) <= GR.KS_TOL, label


def test_uniforms_of_the_header_equal_the_integer_restatement():
    rng = np.random.default_rng(77)
    keys = [(0, 0, 0, 0), (2 ** 64 - 1, 0, 0, 0), (5, 1, 7, 2 ** 31), (1, 2 ** 40, 127, 600000)]
    keys += [tuple(int(v) for v in (rng.integers(0, 2 ** 63), rng.integers(0, 5000), rng.integers(0, 1024), rng.integers(0, 10 ** 6)))
             for _ in range(996)]
    assert len(keys) == 1000
    us = []
    for k in keys:
        u = GR.lib().gof_uniform(*k)
        assert u == GR.uniform(*k) and 0.0 < u <= 1.0, k
        us.append(u)
    assert abs(np.mean(us) - 0.5) < 0.05 and len(set(us)) == 1000
    # the event term: in (0, q], its limits, against longdouble.  The argument of log1p is -(u - u e^-q), rounded at 2^-53
    # absolute, and the logarithm's slope there is 1 / (1 - u + u e^-q): for q >> 1 the term loses digits as u -> 1
    for q in (1e-8, 0.3, 30.0):
        for u in (2.0 ** -53, 0.25, 0.5, 1.0 - 2.0 ** -20, 1.0):
            e = GR.lib().gof_event_term(q, u)
            ref = float(-np.log1p(LD(u) * np.expm1(-LD(q))))
            slope = 1.0 / (1.0 - u + u * np.exp(-q))
            assert 0.0 < e <= q and abs(e - ref) <= 1e-14 * ref + 2.0 ** -52 * slope, (q, u, e, ref)
    assert GR.lib().gof_event_term(0.3, 1.0) == pytest.approx(0.3, rel=1e-15)
    assert GR.lib().gof_tile() == GR.TILE and GR.lib().gof_nout() == 4


STAT_NT = 40000
STAT_SEEDS = (11, 12, 13, 14, 15)


def _simulated(seed):
    """one neuron, a known rate with lam dt in [0.2, 0.5], Bernoulli bins with p = 1 - exp(-q): (q, event bins)"""
    rng = np.random.default_rng(seed)
    t = np.arange(STAT_NT)
    q = 0.35 + 0.15 * np.sin(2 * np.pi * t / 997.0 + rng.uniform(0, 6.28))
    ev = np.flatnonzero(rng.random(STAT_NT) < -np.expm1(-q))
    return q, ev


@pytest.mark.skipif(not LD_IS_WIDER, reason="numpy.longdouble is float64 here")
@pytest.mark.parametrize('seed', STAT_SEEDS)
def test_correction_removes_the_bias_of_binned_time_rescaling(seed):
    """Reference arithmetic only.  Over these five seeds at 40 000 bins (about 11 600 intervals, band 0.0126) the corrected D is
    0.005 .. 0.012 and the uncorrected one 0.21."""
    from theano_pyglm_amd.inference import gof
    q, ev = _simulated(seed)
    assert q.min() >= 0.2 and q.max() <= 0.5
    cum = np.cumsum(q.astype(LD))
    plain = np.asarray(cum[ev[1:]] - cum[ev[:-1]], dtype=float)
    u = np.array([GR.uniform(seed, 0, 0, j) for j in range(1, ev.size)], dtype=LD)
    corr = np.asarray(cum[ev[1:] - 1] - cum[ev[:-1]] - np.log1p(u * np.expm1(-q[ev[1:]].astype(LD))), dtype=float)
    band = gof.ks_band(plain.size)
    d_plain, d_corr = GR.ks_reference(plain)[0], GR.ks_reference(corr)[0]
    print("seed %d: %d intervals, band %.4f, corrected D %.4f, uncorrected D %.4f" % (seed, plain.size, band, d_corr, d_plain))
    assert d_corr <= band
    assert d_plain >= 3.0 * band


class _FakePopulation(object):
    """compute_rescaled_intervals as the parent's Population has it: one positional argument"""

    def __init__(self, taus, stats):
        self.taus, self.stats = taus, stats

    def compute_rescaled_intervals(self, x):
        return self.taus, self.stats


def test_defaults_of_ks_time_rescaling_are_what_they_were():
    from theano_pyglm_amd.inference import gof
    taus = [np.zeros(0), np.array([0.7]), np.array([0.7, 0.1]), np.random.default_rng(5).exponential(size=400)]   # test_gof_host's
    stats = np.array([[0.5, 1, 0, 0], [1.5, 2, 0, 0], [2.5, 3, 1, 0], [390.0, 401, 3, 0]])
    res = gof.ks_time_rescaling(_FakePopulation(taus, stats), None)
    D, band, passed, cnt = gof.ks_from_intervals(taus)
    old = {'D': D, 'band': band, 'passed': passed, 'n_intervals': cnt, 'expected_count': stats[:, 0],
           'observed_count': np.array([1, 2, 3, 401]), 'multi_spike_bins': np.array([0, 0, 1, 3])}
    for k, v in old.items():
        assert np.array_equal(res[k], v, equal_nan=True) and res[k].dtype == np.asarray(v).dtype, k
    assert res['alpha'] == 0.05 and res['route'] == 'host'
    assert np.array_equal(res['D'], np.fmax(res['D_plus'], res['D_minus']), equal_nan=True)
    assert "3 of 4" not in gof.format_table(res) and "of 4 neurons inside the band" in gof.format_table(res)
    sig = inspect.signature(gof.ks_time_rescaling)
    assert list(sig.parameters)[:6] == ['population', 'x', 'alpha', 'correct', 'seed', 'device']
    assert [sig.parameters[k].default for k in ('alpha', 'correct', 'seed', 'device')] == [0.05, False, 0, False]
    sig = inspect.signature(gof.ks_time_rescaling_draws)
    assert list(sig.parameters) == ['population', 'x', 'samples', 'alpha', 'correct', 'seed', 'n_lo']
    assert [sig.parameters[k].default for k in ('alpha', 'correct', 'seed', 'n_lo')] == [0.05, True, 0, 0]
    from theano_pyglm_amd.population import Population
    sig = inspect.signature(Population.compute_rescaled_intervals)
    assert [(k, sig.parameters[k].default) for k in ('correct', 'seed', 'draw')] == [('correct', False), ('seed', 0), ('draw', 0)]


def test_new_symbols_bindings_and_kernels():
    import ctypes
    import sys
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(GR.ROOT, 'include', 'pyglm_hip.h')).read()
    for n in ('pgl_rescale_corr_dev', 'pgl_rescale_corr', 'pgl_ks_uniform_dev', 'pgl_ks_uniform'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and 'int %s(' % n in hdr
    assert _lib.load().pgl_version() >= 114
    for m in ('rescale_corr_dev', 'rescale_corr', 'ks_uniform', 'ks_uniform_dev', 'ks_uniform_host'):
        assert hasattr(_lib.DeviceGlm, m)
    L = _lib.load()
    assert L.pgl_rescale_corr_dev(None, None, None, 0, 0, None, None, None) == -1
    assert L.pgl_rescale_corr(None, None, None, 0, 0, None, None) == -1
    assert L.pgl_ks_uniform_dev(None, None, None, 1, None, None) == -1
    assert L.pgl_ks_uniform(None, None, None, 1, None, None) == -1
    sys.path.insert(0, os.path.join(GR.ROOT, 'tools'))
    import kernel_resources as KR
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items()
                 if KR.short(n).startswith(('k_rcorr', 'k_ks_')))
    print(built)
    assert sorted(built) == ['k_ks_segment', 'k_rcorr_chunk<0>', 'k_rcorr_chunk<1>', 'k_rcorr_finish']
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0, (n, r)
    src = open(os.path.join(GR.ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_gof.h')).read()
    assert '#define PGL_KS_TILE %d' % _lib.KS_TILE in src and _lib.KS_TILE == GR.TILE and _lib.KS_NOUT == 4
