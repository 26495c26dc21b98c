"""The committed case table of the Hessian-vector sweep (tests/hvp_cases.json, written by
`python tools/reachable_kernels.py --emit-hvp-cases`) names every kernel instantiation that pgl_hvp_prepare_* /
pgl_hvp_apply_dev can reach -- a dry run of both (paths 3 / 4 of pgl_plan_kernels) over the shape grid, with and without
the forcing options -- holds exactly one case per reachable (prepare sequence, apply sequence) and per form of call of
every k_hvp5 column pair, and each case still dispatches to the sequences recorded for it.  No GPU needed: a change of
the launch_hvp5 switch or of hvp_select, or a case deleted from the table, fails here with the names concerned.
tests/test_gpu_hvp_sweep.py runs every case against a float64 reference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rk():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import reachable_kernels as RK
    return RK


def test_hvp_dry_run_paths():
    RK = _rk()
    from theano_pyglm_amd import _lib
    import pytest
    assert _lib.load().pgl_version() >= 103
    kw = dict(B=5, R=200, nT=4800)
    assert _lib.plan_kernels(128, path=3, **kw) == ['k_hvp5<18, 22, 1>']
    assert _lib.plan_kernels(128, path=4, **kw) == ['k_hvp5<18, 22, 0>', 'k_fused5<18, 22, 2, 0, 0, 0>']
    # the 3-phase path: one forward-only launch per column slice | the same, then one backward-only launch per slice
    prep, app = _lib.plan_kernels(32, path=3, **kw), _lib.plan_kernels(32, path=4, **kw)
    assert len(prep) == 1 and prep[0].startswith('k_fused2<') and app == prep * 2
    prep, app = _lib.plan_kernels(144, path=3, **kw), _lib.plan_kernels(144, path=4, **kw)
    assert len(prep) == 2 and all(n.startswith('k_fused2<') for n in prep) and app == prep * 2
    assert _lib.plan_kernels(32, path=3, opt_f32=1, **kw)[0].endswith('float>')
    for path in (3, 4):                          # a separable stimulus: unsupported, as the call itself
        with pytest.raises(_lib.PglError, match="separable"):
            _lib.plan_kernels(64, B=3, R=300, Dstim=3 + 24, nT=4800, stim=2, path=path)
    # every arm of the launch_hvp5 switch, both forms
    pairs = set(RK.hvp_pair([n]) for n in RK.hvp_reachable_both()[1] if n.startswith('k_hvp5<'))
    assert pairs == {'3, 3', '5, 5', '7, 7', '9, 11', '12, 14', '14, 18', '18, 22'}, pairs
    for p in pairs:
        assert all('k_hvp5<%s, %d>' % (p, f) in RK.hvp_reachable_both()[1] for f in (0, 1)), p


def test_hvp_case_table_names_every_reachable_instantiation():
    RK = _rk()
    cases = RK.load_cases(RK.HVP_CASES)
    named = set(n for c in cases for n in c['prepare'] + c['apply'])
    auto, reach, seqs = RK.hvp_reachable_both()
    assert set(auto) <= set(reach)
    missing, stale = sorted(set(reach) - named), sorted(named - set(reach))
    assert not missing and not stale, (
        "tests/hvp_cases.json is out of date (python tools/reachable_kernels.py --emit-hvp-cases): "
        "reachable instantiations without a case: %s; named in the table but no longer reachable: %s" % (missing, stale))
    # exactly one case per role: a base case per (prepare, apply) sequence pair, one per form and k_hvp5 pair, one short
    have, want = sorted(RK.hvp_case_role(c) for c in cases), RK.hvp_roles(seqs)
    assert have == want, ("tests/hvp_cases.json is out of date: roles without a case: %s; cases without a role (or twice): %s"
                          % (sorted(set(want) - set(have)), sorted(r for r in have if r not in want or have.count(r) > 1)))


def test_hvp_case_table_matches_the_dry_run():
    RK = _rk()
    cases = RK.load_cases(RK.HVP_CASES)
    assert len(cases) >= 7 * (1 + len(RK.HVP_FORMS)) + 1
    bad = []
    for c in cases:
        assert sorted(k for k in c if k not in ('prepare', 'apply', 'role')) == sorted(RK.HVP_FIELDS), c
        assert c['nT'] % 16 != 0 and c['n_lo'] + c['count'] <= c['N'], c        # a ragged last time tile
        assert 0 <= c['t_lo'] < c['t_hi'] <= c['nT'] and c['t_lo'] % 16 == 0, c
        assert not c['list'] or c['n_lo'] == 0, c
        pair = RK.hvp_pair(c['apply'])
        tiles = (c['t_hi'] + 15) // 16 - c['t_lo'] // 16
        tpc = -(-tiles // min(RK.DRY_CUS, tiles))           # make_plan: tiles per chunk, one chunk per workgroup
        per_wg = [min(tpc, tiles - i * tpc) for i in range(-(-tiles // tpc))]
        if c['role'] == 'ring':                  # every workgroup walks >= 3 tiles; ragged sub-range at the last neuron
            assert pair and min(per_wg) >= 3 and c['n_lo'] > 0 and c['count'] % 16 and c['n_lo'] + c['count'] == c['N'], c
        elif c['role'] in RK.HVP_FORMS:
            assert pair and max(per_wg) <= 1, c
        if c['role'] == 'list':
            assert c['list'] == 1 and 4 <= c['count'] <= c['N'] - 3, c
        if c['role'] == 'trange':
            assert c['t_lo'] > 0 and c['t_hi'] % 16 != 0, c
        if c['role'] == 'dstim':
            assert c['Dstim'] > 0 and c['count'] >= 65 and c['opt_kernel'] == 0 and c['opt_f32'] == 0, c
        if c['role'] == 'short':
            assert pair and c['nT'] < 16, c
        try:
            names = RK.hvp_names(c)
        except Exception as e:               # (no plan any more: reported with the case)
            names = ('%s: %s' % (type(e).__name__, e),)
        if names != (c['prepare'], c['apply']):
            bad.append((dict((k, c[k]) for k in RK.HVP_FIELDS), c['prepare'], c['apply'], names))
    assert not bad, "cases whose dry run changed (case, recorded prepare, apply, now): %s" % bad
