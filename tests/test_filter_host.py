"""The gcc build of the rule of the filter bands (tests/csrc/filters_host.c over csrc/pglm_filters.h) against the numpy
statement, bit for bit; a group alone; pooled chains; average_states against the reference's average / std arithmetic on
samples_to_states dicts; the driver's layouts; synth_map's flag; the new symbols and the kernels' resources."""
import os

import numpy as np
import pytest

from tests import filter_reference as FR
from theano_pyglm_amd.inference import filters as F

CASES = FR.load()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_gcc_mirror_and_numpy_statement_agree_bit_for_bit(c):
    a = FR.args(c)
    out, grp = F.filter_bands_numpy(*a)
    hout, hgrp = FR.host_bands(*a)
    assert FR.same_bits(hgrp, grp) and FR.same_bits(hout, out)


def test_a_group_alone_equals_itself_among_others():
    c = [c for c in CASES if c['name'] == 's63'][0]
    x, nc, first, G, basis, cc, level = FR.args(c)
    out, grp = FR.host_bands(x, nc, first, G, basis, cc, level)
    for m, g in ((0, 0), (1, 3), (2, 4)):
        for fn in (FR.host_bands, F.filter_bands_numpy):
            o1, g1 = fn(np.ascontiguousarray(x[:, m:m + 1]), nc, first + g * c['B'], 1, basis, cc, level)
            assert FR.same_bits(o1[0, 0], out[m, g]) and FR.same_bits(g1[0, 0], grp[m, g])


def test_four_chains_equal_one_chain_in_pooled_order():
    c = [c for c in CASES if c['name'] == 's256_c4_zero_lag'][0]
    x, nc, first, G, basis, cc, level = FR.args(c)
    n, M = c['n'], c['M']
    one = x.reshape(n, nc, M, -1).transpose(1, 0, 2, 3).reshape(nc * n, M, -1)         # s = chain n + draw
    for fn in (FR.host_bands, F.filter_bands_numpy):
        a, b = fn(x, nc, first, G, basis, cc, level), fn(np.ascontiguousarray(one), 1, first, G, basis, cc, level)
        assert FR.same_bits(a[0], b[0]) and FR.same_bits(a[1], b[1])


def _population(basis_stim):
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    model = make_model('standard_glm', N=2, dt=0.001)
    if basis_stim:
        model['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': model['bkgd']['basis']}
    return Population(model)


@pytest.mark.parametrize('basis_stim', [False, True], ids=['no_stimulus', 'basis_stimulus'])
def test_average_states_against_the_list_of_dicts_arithmetic(basis_stim):
    """average_list_of_dicts / std_list_of_dicts of the reference over the per-draw states: the mean of the entries, and
    sqrt(mean((v - avg)^2)) -- the POPULATION sd, denominator S.  average_states(ddof=0) states that one (the bands' sd,
    denominator S - 1, times sqrt((S - 1) / S)); ddof=1 gives the bands' own.  Both to rounding: the sums run in another
    order."""
    from theano_pyglm_amd.inference.batched_hmc import samples_to_states
    popn = _population(basis_stim)
    rng = np.random.RandomState(5)
    x = popn.sample(rng)
    S, N, P = 12, popn.N, popn.glm.P
    samples = 0.3 * rng.standard_normal((S, N, P))
    states = []
    for i in range(S):
        glms = samples_to_states(popn, x, samples, i)
        states.append([popn.glm.get_state(g) for g in glms])
    s_mean, s_std = F.average_states(popn, x, samples, device=False)
    _, s_std1 = F.average_states(popn, x, samples, ddof=1, device=False)
    keys = [('imp', 'impulse')] + ([('bkgd', 'stim_response')] if basis_stim else [])
    for n in range(N):
        for a, b in keys:
            vals = np.array([st[n][a][b] for st in states])
            avg = vals.sum(axis=0) / S
            std = np.sqrt(((vals - avg) ** 2).sum(axis=0) / S)
            assert s_mean['glms'][n][a][b].shape == avg.shape
            assert np.allclose(s_mean['glms'][n][a][b], avg, rtol=1e-12, atol=1e-15)
            assert np.allclose(s_std['glms'][n][a][b], std, rtol=1e-12, atol=1e-15)
            assert np.allclose(s_std1['glms'][n][a][b], vals.std(axis=0, ddof=1), rtol=1e-12, atol=1e-15)
        assert ('stim_response' in s_mean['glms'][n]['bkgd']) == basis_stim
        assert np.array_equal(s_mean['glms'][n]['imp']['basis'], popn.glm.imp_model.ibasis)


def test_driver_layouts_and_keys_on_the_host_route():
    popn = _population(True)
    rng = np.random.RandomState(6)
    N, P = popn.N, popn.glm.P
    chains = rng.standard_normal((2, 9, N, P))
    res = F.filter_bands(popn, chains, level=0.9, device=False)
    R, Rs = popn.glm.imp_model.ibasis.shape[0], popn.glm.bkgd_model.ibasis.shape[0]
    assert res['route'] == 'host' and res['level'] == 0.9
    assert res['impulse']['q_hi'].shape == (N, N, R) and res['stim']['mean'].shape == (N, 2, Rs) and res['lags'].shape == (R,)
    for k in ('c_sim', 'weight_mean', 'weight_sd', 'weight_q_lo', 'weight_median', 'weight_q_hi', 'p_pos', 'info', 'excl_zero'):
        assert res[k].shape == (N, N) and res['stim'][k].shape == (N, 2), k
    pooled = chains.reshape(18, N, P)                                                 # one chain in pooled order
    one = F.filter_bands(popn, {'samples': pooled}, level=0.9, device=False)
    assert FR.same_bits(one['impulse']['sd'], res['impulse']['sd']) and FR.same_bits(one['stim']['c_sim'], res['stim']['c_sim'])
    # the layout theta_row gives: stimulus weight b of dimension d at 1 + d B_stim + b, impulse weight b of neuron j behind them
    Bs, B = popn.glm.bkgd_model.B, popn.glm.imp_model.ibasis.shape[1]
    w = pooled[:, 1, 1 + Bs:1 + 2 * Bs]
    assert np.allclose(res['stim']['mean'][1, 1], popn.glm.bkgd_model.ibasis.dot(w.mean(axis=0)), rtol=1e-10, atol=1e-14)
    w = pooled[:, 0, 1 + 2 * Bs + B:1 + 2 * Bs + 2 * B]
    assert np.allclose(res['impulse']['mean'][0, 1], popn.glm.imp_model.ibasis.dot(w.mean(axis=0)), rtol=1e-10, atol=1e-14)
    assert 'stim' not in F.filter_bands(popn, chains, stim=False, device=False)
    assert 'stim' not in F.filter_bands(_population(False), rng.standard_normal((9, N, 1 + N * B)), device=False)
    with pytest.raises(ValueError):
        F.filter_bands(popn, chains[:, :, :, :-1], device=False)
    with pytest.raises(ValueError):
        F.filter_bands(popn, chains[0, :1], device=False)
    text = F.band_table(res, truth=np.eye(N, dtype=bool))
    assert text.startswith("filter bands (level 0.9, host)") and len(text.splitlines()) == N + 2


def test_unserved_packing_raises_the_samplers_error():
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model('spatiotemporal_glm', N=2, dt=0.001))
    with pytest.raises(ValueError, match="lock-step HMC"):
        F.filter_bands(popn, np.zeros((9, 2, 5)), device=False)


def test_synth_map_flag_parsing():
    from theano_pyglm_amd.harness.synth_map import parser
    p = parser()
    assert p.parse_args(['-d', 'x']).filters is None
    assert p.parse_args(['-d', 'x', '--hmc', '64', '--filters']).filters == 0.95
    a = p.parse_args(['-d', 'x', '--nuts', '64', '--filters', '0.9'])
    assert a.filters == 0.9 and a.nuts == 64


def test_symbols_constants_and_kernel_resources():
    """(No GPU needed: the library's exports and the code object's metadata.)"""
    import ctypes
    import sys
    import __graft_entry__ as ge
    from theano_pyglm_amd import _lib
    ge.build_hip()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(FR.ROOT, 'include', 'pyglm_hip.h')).read()
    for n in ('pgl_filter_bands_dev', 'pgl_filter_bands'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS and 'int %s(' % n in hdr
    assert _lib.load().pgl_version() >= 117
    assert (_lib.FILT_MAX_B, _lib.FILT_MAX_DRAWS, F.PIECE) == (FR.lib().filters_max_b(), FR.lib().filters_max_draws(),
                                                               FR.lib().filters_piece())
    assert len(_lib.FILT_LAG_COLS) == 5 and len(_lib.FILT_GRP_COLS) == 8
    sys.path.insert(0, os.path.join(FR.ROOT, 'tools'))
    import reachable_kernels as RK
    built = dict((n, r) for n, r in RK.built_fused().items() if n.startswith('k_filter_bands<'))
    assert len(built) == 16
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['lds'] <= 512, (n, r)
