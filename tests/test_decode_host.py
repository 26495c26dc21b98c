"""Host side of stimulus decoding: the numpy statement of inference/decode.py, the gcc mirror of csrc/pglm_decode.h and the
library's own plain-C entry point pgl_decode_host, each against the longdouble reference within the derived bound
(tests/decode_reference.py); the pieces of the mirror (L, L^T, K *, K^T) against each other; the new symbols and ABI 119."""
import os
import re

import numpy as np
import pytest

from tests import decode_reference as DR
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import decode as DEC

LD = np.longdouble


def _check_all(name, F, g, hv1, hv2, label):
    ref = DR.reference(name)
    ratios = [DR.check(F[0], ref, 'F', label + ' ' + name), DR.check(F[1], ref, 'll', label + ' ' + name),
              DR.check(F[2], ref, 'lp', label + ' ' + name), DR.check(g, ref, 'g', label + ' ' + name),
              DR.check(hv1, ref, 'hv1', label + ' ' + name), DR.check(hv2, ref, 'hv2', label + ' ' + name)]
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize('name', DR.NAMES)
def test_mirror_within_the_bound(name):
    m = DR.make_case(name)
    F, g, hv1 = DR.mirror_eval(name, m['u'], m['v1'])
    _, _, hv2 = DR.mirror_eval(name, m['u'], m['v2'])
    _check_all(name, F, g, hv1, hv2, 'mirror')


@pytest.mark.parametrize('name', DR.NAMES)
def test_numpy_statement_within_the_bound(name):
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    prob = DEC.DecodeProblem(m['c'], m['S'], m['basis'], m['theta'][:, 1:1 + c['D'] * c['B']], c['D'], c['nlin'], DR.DT, c['q'],
                             *DR.prior_of(c))
    F, g = prob.eval(m['u'])
    _check_all(name, F, g, prob.hvp(m['v1']), prob.hvp(m['v2']), 'numpy')


@pytest.mark.parametrize('name', ['n1_rt1_exp', 'n3_q4_high', 'n17_rt70_low', 'n3_mid', 'n70_two_slabs'])
def test_library_host_entry_equals_the_mirror(name):
    """pgl_decode_host compiles the same header with the host compiler of the library: the same rule, within the bound of the
    reference as well (bit equality is not asked: two compilers may contract multiply-adds differently)."""
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    F, g, hv1 = _lib.decode_host(m['c'], m['S'], m['basis'], c['D'], m['theta'], c['nlin'], DR.DT, m['u'], c['q'], DR.prior_of(c),
                                 v=m['v1'])
    _, _, hv2 = _lib.decode_host(m['c'], m['S'], m['basis'], c['D'], m['theta'], c['nlin'], DR.DT, m['u'], c['q'], DR.prior_of(c),
                                 v=m['v2'])
    _check_all(name, F, g, hv1, hv2, 'pgl_decode_host')


@pytest.mark.parametrize('name', ['n3_q4_high', 'n17_rt70_low', 'n1_frames_past'])
def test_mirror_pieces_are_adjoint(name):
    """<L a, b> = <a, L^T b> and <K * a, b> = <a, K^T b> for the mirror's four operators, to the f64 rounding of the sums."""
    c = DR.BY_NAME[name]
    m = DR.make_case(name)
    L = DR.lib()
    nT, N, D, Tu, q, Rt = c['nT'], c['N'], c['D'], c['Tu'], c['q'], c['Rt']
    rng = np.random.RandomState(5)
    a, b = rng.randn(Tu, D), rng.randn(nT, D)
    La, Ltb = np.empty((nT, D)), np.empty((Tu, D))
    L.decode_interp(DR._p(a), Tu, D, q, nT, DR._p(La))
    L.decode_interp_t(DR._p(b), nT, D, q, Tu, DR._p(Ltb))
    assert abs(np.sum(La * b) - np.sum(a * Ltb)) <= 4 * nT * D * DR.U * np.sum(np.abs(La) * np.abs(b))
    K = np.ascontiguousarray(DR.filters(m['basis'], m['theta'], D).astype(np.float64))
    s, y = rng.randn(nT, D), rng.randn(nT, N)
    Ks, Kty = np.empty((nT, N)), np.empty((nT, D))
    L.decode_conv(DR._p(K), Rt, D, N, DR._p(s), nT, DR._p(Ks))
    L.decode_corr(DR._p(K), Rt, D, N, DR._p(y), nT, DR._p(Kty))
    scale = float((np.abs(DR.K_apply(np.abs(K).astype(LD), np.abs(s).astype(LD))) * np.abs(y)).sum())
    assert abs(np.sum(Ks * y) - np.sum(s * Kty)) <= 4 * (Rt * D + nT * N) * DR.U * scale


def test_numpy_statement_turns_down_what_is_not_served():
    m = DR.make_case('n3_mid')
    with pytest.raises(ValueError, match="integer"):
        DEC.frames_per_bin(0.0025, 0.001)
    with pytest.raises(ValueError, match="nonlinearity"):
        DEC.DecodeProblem(m['c'], m['S'], m['basis'], m['theta'][:, 1:13], 3, 'relu', DR.DT, 4, 0.0, 1.0, np.inf)
    assert DEC.frames_per_bin(0.004, 0.001) == 4


def test_symbols_and_abi():
    names = ('pgl_decode_prepare_dev', 'pgl_decode_eval_dev', 'pgl_decode_hvp_dev', 'pgl_decode_prepare', 'pgl_decode_eval', 'pgl_decode_hvp',
             'pgl_decode_host')
    header = open(os.path.join(DR.ROOT, 'include', 'pyglm_hip.h')).read()
    assert int(re.search(r'#define PGL_ABI_VERSION (\d+)', header).group(1)) == 119
    assert _lib.ABI_VERSION == 119
    for n in names:
        assert n in _lib.SYMBOLS and re.search(r'\bint %s\(' % n, header), n
    assert 'pgl_decode_prior' in header and 'PGL_OPT_DECODE_CUT 89' in header and _lib.OPT_DECODE_CUT == 89
    for m in ('decode_prepare', 'decode_prepare_dev', 'decode_eval', 'decode_eval_dev', 'decode_hvp', 'decode_hvp_dev'):
        assert hasattr(_lib.DeviceGlm, m), m
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n


def test_dry_run_records_the_decoding_launches():
    ev = _lib.plan_kernels(8, B=2, R=10, Dstim=4, nT=2000, path=11)
    for k in ('k_dec_filters', 'k_dec_offset', 'k_dec_interp', 'k_dec_forward<0, 0>', 'k_dec_sum', 'k_dec_backward', 'k_dec_interp_t'):
        assert k in ev, (k, ev)
    assert ev.index('k_dec_filters') < ev.index('k_dec_offset') < ev.index('k_dec_interp') < ev.index('k_dec_sum')
    assert _lib.plan_kernels(8, B=2, R=10, Dstim=4, nT=2000, path=12) == ['k_dec_interp', 'k_dec_forward<0, 1>', 'k_dec_backward',
                                                                          'k_dec_interp_t']
    with pytest.raises(_lib.PglError, match="'basis' stimulus"):
        _lib.plan_kernels(8, B=2, R=10, Dstim=0, nT=2000, path=11)
    with pytest.raises(_lib.PglError, match="separable"):
        _lib.plan_kernels(8, B=2, R=10, Dstim=4, nT=2000, stim=1, path=11)


def test_population_checks_the_stimulus_columns():
    """The host forms move Tu * D doubles: an array whose columns are not the model's stimulus dimensions is turned down before
    anything reaches the library (a vector is one dimension)."""
    from theano_pyglm_amd.population import Population
    assert Population._stimulus_array(np.zeros(7), 1, 'stim').shape == (7, 1)
    assert Population._stimulus_array(np.zeros((7, 2)), 2, 'stim').shape == (7, 2)
    with pytest.raises(ValueError, match=r"stim must be \(Tu, D\) with D = 2 stimulus dimensions, got \(7, 1\)"):
        Population._stimulus_array(np.zeros(7), 2, 'stim')
    with pytest.raises(ValueError, match=r"v must be \(Tu, D\) with D = 2 stimulus dimensions, got \(7, 3\)"):
        Population._stimulus_array(np.zeros((7, 3)), 2, 'v')


def test_sanitizer_program_runs_over_the_table(tmp_path):
    """The stand-alone program of tests/csrc/decode_host.c (DECODE_HOST_MAIN) over the problem file DR.write_problems writes from
    the case table: built plain here; DR.write_problems' docstring has the -fsanitize=address,undefined line.  Its F of every
    case is the mirror's."""
    import subprocess
    path = str(tmp_path / 'decode_problems.txt')
    exe = str(tmp_path / 'decode_host_main')
    names = [n for n in DR.NAMES if DR.BY_NAME[n]['nT'] * DR.BY_NAME[n]['N'] <= 40000]      # (the quick ones; the run by hand takes all)
    DR.write_problems(path, names)
    subprocess.check_call(['gcc', '-O2', '-DDECODE_HOST_MAIN', '-o', exe, DR.mirror_sources()[0], '-lm'])
    out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names) >= 6
    for line, name in zip(out, names):
        F = float(re.search(r'F = (\S+)', line).group(1))
        assert F == DR.mirror_eval(name, DR.make_case(name)['u'])[0][0], (name, line)
