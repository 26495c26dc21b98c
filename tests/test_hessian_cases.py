"""The case table of the dense-Hessian sweep (tests/hessian_cases.json) reaches what it claims, and the sweep's reference
stays inside its own bound.  No GPU needed: the dry run of the dispatch (pgl_plan_kernels, path 3 = pgl_hvp_prepare_*,
path 5 = the k_hess launches of pgl_hess_dev after it), the shapes, and the spike arrays of the cases.

Per case every tag of its `hits` is checked against the shape / the dry run / the spikes; over the table: both k_hess
instantiations, a case with a second launch (r0 > 0), the four K edges of the 64-column blocking, both sides of the
staging's cnt <= 16.  Chunk counts depend on the CU count a device-less handle assumes and are not asserted here.
tests/test_gpu_hessian_sweep.py runs every case on the device."""
import numpy as np
import pytest

from tests import hessian_reference as HR

CB = 64                                   # PGL_HESS_CB
NEEDED = {'block-of-64-neurons', 'straddle-every-offset', 'ragged-last-block', 'K=64k', 'K=64k+1', 'Kimp=64k-with-stimulus',
          'Dstim>64', 'staging-overflow', 'staged', 'silent-neuron', 'rows', 'slab', 'partial-range-off-16', 'time-range',
          'list', 'two-launches', 'exp', 'ragged-post-tile'}


def _lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    return _lib


def _dry(c, path):
    ids = HR.neurons(c)
    n_lo = 0 if c['list'] else int(ids[0])         # a list is prepared as rows [0, count) of the call
    return _lib().plan_kernels(c['N'], B=c['B'], R=c['R'], Dstim=c['Dstim'], nT=c['nT'], n_lo=n_lo, count=len(ids), path=path)


def _windows(c):
    """event counts of the (tile, presynaptic neuron) windows the case's time range walks"""
    p = HR.problem(c)
    t_lo, t_hi = HR.time_range(c)
    return p, HR.window_counts(p.S, c['R'])[t_lo // 16:(t_hi + 15) // 16]


def _holds(tag, c):
    N, B, D = c['N'], c['B'], c['Dstim']
    Kimp, K = N * B, N * B + D + 1
    count = len(HR.neurons(c))
    t_lo, t_hi = HR.time_range(c)
    if tag == 'block-of-64-neurons':
        return B == 1 and Kimp > CB
    if tag == 'straddle-every-offset':        # the first neuron of every later block starts at another column of the block
        offs = [(-(CB * i)) % B for i in range(1, (Kimp + CB - 1) // CB)]
        return B == 7 and len(offs) >= 2 and len(set(offs)) == len(offs) and 0 not in offs
    if tag == 'ragged-last-block':
        return K % CB > 1
    if tag == 'K=64k':
        return K % CB == 0
    if tag == 'K=64k+1':
        return K % CB == 1 and K > CB
    if tag == 'Kimp=64k-with-stimulus':
        return Kimp % CB == 0 and D > 0
    if tag == 'Dstim>64':                     # and a block without an impulse column that is not the constant's alone
        return D > CB and any(CB * i >= Kimp and CB * i < Kimp + D for i in range((K + CB - 1) // CB))
    if tag in ('staging-overflow', 'staged'):
        w = _windows(c)[1]
        return bool(np.any(w > HR.CAP)) if tag == 'staging-overflow' else bool(np.any((w > 0) & (w <= HR.CAP)))
    if tag == 'silent-neuron':
        p, w = _windows(c)
        return len(c['silent']) > 0 and all(not p.S[:, n].any() and not w[:, n].any() for n in c['silent'])
    if tag == 'rows':
        return c['kernel'] == 'k_hess<0>'
    if tag == 'slab':
        return c['kernel'] == 'k_hess<1>'
    if tag == 'partial-range-off-16':
        return count % 16 != 0 and count < N and (c['list'] > 0 or c['range'][0] % 16 != 0)
    if tag == 'time-range':                   # t_lo on the 16 grid and on no coarser one, t_hi inside a tile
        return t_lo > 0 and t_lo % 16 == 0 and (t_lo // 16) % 2 == 1 and t_hi % 16 != 0 and t_hi < c['nT']
    if tag == 'list':
        return c['list'] > 0
    if tag == 'two-launches':
        return c['launches'] >= 2
    if tag == 'exp':
        return c['kind'] == 'exp'
    if tag == 'ragged-post-tile':
        return count % 16 != 0
    raise AssertionError("unknown tag %r" % tag)


def test_case_table_is_well_formed():
    cases = HR.load_cases()
    assert len(set(c['name'] for c in cases)) == len(cases)
    for c in cases:
        assert (c['range'] is None) != (c['list'] == 0), c['name']
        ids = HR.neurons(c)
        assert 0 <= ids.min() and ids.max() < c['N'] and len(set(ids.tolist())) == len(ids), c['name']
        t_lo, t_hi = HR.time_range(c)
        assert 0 <= t_lo < t_hi <= c['nT'] and t_lo % 16 == 0, c['name']
        assert 200 <= c['nT'] <= 4000, c['name']                   # a few hundred to a few thousand bins
        assert c['B'] <= 8 and c['kind'] in ('explinear', 'exp'), c['name']
        assert all(0 <= n < c['N'] for n in c['silent']), c['name']


def test_every_case_hits_what_it_claims():
    cases = HR.load_cases()
    bad = [(c['name'], t) for c in cases for t in c['hits'] if not _holds(t, c)]
    assert not bad, "claimed but not reached: %s" % bad
    reached = set(t for c in cases for t in c['hits'])
    assert NEEDED <= reached, "no case for: %s" % sorted(NEEDED - reached)
    # the shapes the table must hold
    shapes = set((c['N'], c['B'], c['Dstim']) for c in cases)
    assert {(70, 1, 0), (21, 3, 0), (32, 2, 0), (32, 2, 5), (8, 3, 70)} <= shapes
    assert {1, 2, 3, 7} <= set(c['B'] for c in cases) and {37, 100, 300} <= set(c['R'] for c in cases)
    for kind in ('explinear', 'exp'):
        assert any(c['kind'] == kind and {'staging-overflow', 'staged', 'silent-neuron'} <= set(c['hits']) for c in cases), kind
    assert any(c['kind'] == 'exp' and 'slab' in c['hits'] for c in cases)
    for form in ('list', 'partial-range-off-16'):
        assert any({'rows', 'time-range', form} <= set(c['hits']) and c['N'] * c['B'] + c['Dstim'] + 1 > 640 for c in cases), form


def test_case_table_matches_the_dry_run():
    cases = HR.load_cases()
    bad, seen = [], set()
    for c in cases:
        prep, hess = _dry(c, 3), _dry(c, 5)
        seen.update(hess)
        if hess != [c['kernel']] * c['launches']:
            bad.append((c['name'], hess))
        if (c['kernel'] == 'k_hess<1>') != (len(prep) == 1 and prep[0].startswith('k_hvp5<')):
            bad.append((c['name'], prep))
    assert not bad, "cases whose dry run differs from the table: %s" % bad
    assert seen == {'k_hess<0>', 'k_hess<1>'}, seen


def test_two_launch_case_by_the_plans_arithmetic():
    """hess_plan (csrc/pglm_plan.h): 32 KiB of partials per (row, block pair, chunk) within 512 MiB, rounded down to whole
    groups of eight rows: the rows of the first launch, and r0 of the second."""
    c = [c for c in HR.load_cases() if c['launches'] >= 2]
    assert c
    c = c[0]
    K = c['N'] * c['B'] + c['Dstim'] + 1
    ncb = (K + CB - 1) // CB
    rows = ((512 << 20) // (ncb * (ncb + 1) // 2 * 32768)) & ~7
    count = len(HR.neurons(c))
    assert 8 <= rows < count and -(-count // rows) == c['launches'], (rows, count)
    assert (rows, count - rows) == (64, 8)            # r0 = 64, and a last launch of one group
    assert count * K * K * 8 < 1 << 30                # the output stays under 1 GiB


def test_overflow_cases_have_windows_on_both_sides_of_the_staging():
    for c in HR.load_cases():
        if 'staging-overflow' not in c['hits']:
            continue
        p, w = _windows(c)
        over = np.any(w > HR.CAP, axis=0)
        print("%s: windows with > %d events %d, with 1..%d events %d, empty %d; largest %d; neurons that overflow: %s"
              % (c['name'], HR.CAP, np.sum(w > HR.CAP), HR.CAP, np.sum((w > 0) & (w <= HR.CAP)), np.sum(w == 0), w.max(),
                 np.nonzero(over)[0].tolist()))
        assert over.any() and not over.all()                                     # quiet neurons in the same population
        assert np.all(np.any((w > 0) & (w <= HR.CAP), axis=0)[over])             # a bursting neuron is staged in other tiles
        # a tile whose 64-column block mixes both kinds (k_hess stages per block and tile)
        assert np.any(np.any(w > HR.CAP, axis=1) & np.any((w > 0) & (w <= HR.CAP), axis=1))


@pytest.mark.parametrize('name', ['kimp64-dstim5', 'overflow-explinear-zeros'])
def test_reference_meets_its_own_bound(name):
    """H_ref summed in numpy.longdouble against the float64 matrix product, for three neurons: within the summation part
    of gamma (the curvature is the same float64 array in both), exact zeros where A == 0."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is float64 on this platform")
    c = [c for c in HR.load_cases() if c['name'] == name][0]
    p = HR.problem(c)
    t_lo, t_hi = HR.time_range(c)
    ids = HR.neurons(c)[[0, len(HR.neurons(c)) // 2, -1]]
    H64, A = HR.ref_hessian(p, ids, t_lo, t_hi)
    Hld, _ = HR.ref_hessian(p, ids, t_lo, t_hi, dtype=np.longdouble)
    d = np.abs(H64.astype(np.longdouble) - Hld).astype(float)
    g = HR.gamma_sum(t_hi - t_lo)
    zero = A == 0.0
    assert zero.any() and np.all(H64[zero] == 0.0) and np.all(Hld[zero] == 0.0)
    ratio = (d[~zero] / (g * A[~zero])).max()
    print("%s: float64 against longdouble: worst |dH| / (gamma_sum A) %.3e (gamma_sum %.3e; gamma %.3e)"
          % (name, ratio, g, HR.gamma(t_hi - t_lo)))
    assert ratio <= 1.0
    assert np.max(d.max(axis=(1, 2)) / np.abs(H64).max(axis=(1, 2))) <= HR.TOL
    # the silent neuron's rows and columns, and those of a zero in Weff, are among the exact zeros
    for i, n in enumerate(ids):
        for m in list(c['silent']) + np.nonzero(p.Weff[:, n] == 0.0)[0].tolist():
            cols = slice(1 + c['Dstim'] + m * c['B'], 1 + c['Dstim'] + (m + 1) * c['B'])
            assert np.all(zero[i, cols, :]) and np.all(zero[i, :, cols])


def test_curvature_term_of_gamma_is_the_curvature_tests_limit():
    """CURV_REL is no wider than what tests/test_gpu_hvp_curvature.py asserts of the device's c: min(32 x the worst error
    of the branch formulas in numpy float64 on its grid, 1e-10)."""
    pytest.importorskip('mpmath')
    from tests import hvp_reference as R
    limit = min(32.0 * max(R.grid_cpu_error(0.001).values()), 1e-10)
    print("curvature limit %.3e, CURV_REL %.3e" % (limit, HR.CURV_REL))
    assert HR.CURV_REL <= limit * 1.01
