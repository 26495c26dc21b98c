"""Host side of the time-rescaling goodness of fit: the C ABI's symbols, the KS statistic of inference/gof.py against scipy,
the resources of the k_rescale_* kernels in the built code object, and the dry run of their launch sequence.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESCALE_KERNELS = ['k_rescale_chunk<0>', 'k_rescale_chunk<1>', 'k_rescale_scan', 'k_rescale_finish']


def test_rescale_symbols_and_version():
    import ctypes
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'pyglm_hip.h')) as f:
        hdr = f.read()
    for n in ('pgl_rescale_count', 'pgl_rescale_dev', 'pgl_rescale'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
        assert 'int %s(' % n in hdr
    assert _lib.load().pgl_version() >= 105                  # (104: the version before the rescaling entry points)
    for m in ('rescale_count', 'rescale_dev', 'rescale'):
        assert hasattr(_lib.DeviceGlm, m)
    from theano_pyglm_amd.population import Population
    assert hasattr(Population, 'compute_rescaled_intervals')
    # the chunk length the GPU tests place their edge events by
    with open(os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_binwalk.hip.h')) as f:
        m = re.search(r'#define PGL_RS_CHUNK (\d+)', f.read())
    assert int(m.group(1)) == _lib.RESCALE_CHUNK and _lib.RESCALE_CHUNK % 16 == 0


def test_rescale_null_handle_is_an_argument_error():
    from theano_pyglm_amd import _lib
    lib = _lib.load()
    off = np.zeros(3, dtype=np.int64)
    assert lib.pgl_rescale_count(None, off.ctypes.data) == -1
    assert lib.pgl_rescale_dev(None, None, None, None, None, None) == -1
    assert lib.pgl_rescale(None, None, None, None, None) == -1


@pytest.mark.parametrize('n', [2, 3, 7, 100, 1001, 20000])
def test_ks_statistic_equals_scipy(n):
    from scipy import stats
    from theano_pyglm_amd.inference import gof
    rng = np.random.default_rng(1000 + n)
    for z in (rng.random(n), -np.expm1(-rng.exponential(size=n)), -np.expm1(-1.7 * rng.exponential(size=n)),
              np.full(n, 0.25)):
        assert abs(gof.ks_uniform(z) - stats.kstest(z, 'uniform').statistic) <= 1e-14


def test_ks_of_zero_one_and_two_intervals():
    from scipy import stats
    from theano_pyglm_amd.inference import gof
    taus = [np.zeros(0), np.array([0.7]), np.array([0.7, 0.1]), np.random.default_rng(5).exponential(size=400)]
    D, band, passed, cnt = gof.ks_from_intervals(taus)
    assert list(cnt) == [0, 1, 2, 400]
    assert np.isnan(D[0]) and np.isnan(D[1]) and not passed[0] and not passed[1]
    for i in (2, 3):
        z = -np.expm1(-taus[i])
        assert abs(D[i] - stats.kstest(z, 'uniform').statistic) <= 1e-14
        assert band[i] == 1.36 / np.sqrt(cnt[i])
        assert passed[i] == (D[i] <= band[i])
    assert passed[3]                                         # Exp(1) draws (seeded): inside the 95 % band
    # a model whose rate is off by a factor 2 fails at this sample size
    assert not gof.ks_from_intervals([2.0 * taus[3]])[2][0]
    assert np.isnan(gof.ks_uniform([]))
    assert abs(gof.ks_band(100, 0.05) - 0.136) <= 1e-15
    assert abs(gof.ks_band(100, 0.01) - np.sqrt(-0.5 * np.log(0.005)) / 10.0) <= 1e-15


def test_rescale_kernels_are_built_without_scratch():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    from theano_pyglm_amd import _lib
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_rescale'))
    print(built)
    assert sorted(built) == sorted(RESCALE_KERNELS)
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0, (n, r)


def test_dry_run_with_the_rescale_family():
    """Path 6 of the dry run: the forward launches of path 2, then the three rescaling launches; the other paths are what
    they were."""
    from theano_pyglm_amd import _lib
    for N, Ds, stim in ((8, 0, 0), (20, 2, 0), (128, 0, 0), (144, 0, 0), (64, 3 + 1024, 2)):
        fwd = _lib.plan_kernels(N, B=5 if stim == 0 else 3, R=200 if stim == 0 else 300, Dstim=Ds, nT=5000, stim=stim, path=2)
        got = _lib.plan_kernels(N, B=5 if stim == 0 else 3, R=200 if stim == 0 else 300, Dstim=Ds, nT=5000, stim=stim, path=6)
        assert fwd and got[:len(fwd)] == fwd
        assert got[len(fwd):] == ['k_rescale_chunk<0>', 'k_rescale_scan', 'k_rescale_finish']
    assert _lib.plan_kernels(32, B=5, R=200, nT=300000) == ['k_fused6<5, 2, 1, 4, 1>']
