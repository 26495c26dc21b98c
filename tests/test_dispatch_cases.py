"""The committed case table of the dispatch sweep (tests/dispatch_cases.json, written by
`python tools/reachable_kernels.py --emit-cases`) names every fused kernel instantiation the dispatcher can reach, and
each case still dispatches to the launch sequence recorded for it.  No GPU needed (pgl_plan_kernels is a dry run): a new
instantiation, or a dispatch change, without a case in the table fails here with the names concerned.
tests/test_gpu_dispatch_sweep.py runs every case against the oracle."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rk():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import reachable_kernels as RK
    return RK


def test_case_table_names_every_reachable_instantiation():
    RK = _rk()
    cases = RK.load_cases()
    named = set(n for c in cases for n in c['names'])
    reach = set(RK.reachable_both()[1])
    missing, stale = sorted(reach - named), sorted(named - reach)
    assert not missing and not stale, (
        "tests/dispatch_cases.json is out of date (python tools/reachable_kernels.py --emit-cases): "
        "reachable instantiations without a case: %s; named in the table but no longer reachable: %s" % (missing, stale))


def test_case_table_matches_the_dry_run():
    RK = _rk()
    cases = RK.load_cases()
    assert len(cases) >= 100
    bad = []
    for c in cases:
        assert sorted(k for k in c if k != 'names') == sorted(RK.FIELDS), c
        # a ragged last time tile; the Gibbs forward launches cover the whole population
        assert c['nT'] % 16 != 0 and c['n_lo'] + c['count'] <= c['N'], c
        assert c['path'] != 2 or (c['n_lo'] == 0 and c['count'] == c['N']), c
        try:
            names = RK.case_names(c)
        except Exception as e:               # (no plan any more: reported with the case)
            names = ['%s: %s' % (type(e).__name__, e)]
        if names != c['names']:
            bad.append((dict((k, c[k]) for k in RK.FIELDS), c['names'], names))
    assert not bad, "cases whose dry run changed (case, recorded, now): %s" % bad
