"""The collapsed-Gibbs column kernels over tests/gibbs_cases.json against the longdouble reference of tests/gibbs_reference.py
(tests/test_gibbs_cases.py proves on the CPU that every case reaches the edge it is named after).  Per case: every output entry
compared (none left out), the NaN pattern exactly the reference's, worst quotient against the bound
1e-10 |ll| + 1e-12 A + E at most 1, two calls bit-identical, the regime-split and the all-f64 kernel each held to the reference,
the recorded launches those geometry() states."""
import numpy as np
import pytest

from tests import gibbs_reference as GR

pytestmark = pytest.mark.gpu

CASES = GR.load_cases()
LL_CASES = [c for c in CASES if c['update'] is None and c['form'] == 'cols']
UPD_CASES = [c for c in CASES if c['update'] is not None]


def _call(c):
    t_lo, t_hi = GR.case_range(c)
    return c['cols'], c['pre'], GR.case_weights(c), t_lo, t_hi


def _device(c):
    from theano_pyglm_amd import _lib
    p = GR.problem(c)
    d = p.device()
    if c['t'] is not None:
        d.set_time_range(*c['t'])
    d.gibbs_prepare_all(p.theta, p.Weff)
    return p, d, _lib


def _ll(d, _lib, p, c, kern, cols=None, pre=None, ws=None):
    """one recorded pgl_gibbs_ll_cols call: (ll, names of the launches)"""
    cols = c['cols'] if cols is None else cols
    pre = c['pre'] if pre is None else pre
    ws = GR.case_weights(c) if ws is None else ws
    d.set_option(_lib.OPT_GIBBS_KERNEL, kern)
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)                       # (clears the record)
    got = d.gibbs_ll_cols(cols, pre, p.Weff[pre, cols], ws)
    return got, d.last_kernels()


def _same_geometry(d, g):
    """what the host chose for the last recorded call (pgl_gibbs_last_geometry) is what geometry() states"""
    dev = d.gibbs_last_geometry()
    keys = ('CP', 'nsplit', 'ygroups', 'nloop', 'nblk', 'sblk', 'same_pre') if g['path'] == 'regime' else \
           ('CP', 'ygroups', 'nblk', 'gtb', 'rows')
    assert dev['path'] == (0 if g['path'] == 'regime' else 1)
    assert dict((k, dev[k]) for k in keys) == dict((k, int(g[k])) for k in keys), (dev, g)
    return dev


def _check(c, got, ref, tag):
    assert got.shape == ref[0].shape
    assert np.array_equal(np.isnan(got), ref[3]), tag               # the NaN pattern is the reference's, exactly
    assert np.all(np.isfinite(got) | ref[3]), tag                   # ... so no entry is left out of the comparison
    r = GR.ratio(got, ref)
    print('gibbs sweep %-24s %-8s ratio %.3g' % (c['name'], tag, r))
    assert r <= 1.0, (c['name'], tag, r)
    return r


@pytest.mark.parametrize('c', LL_CASES, ids=lambda c: c['name'])
def test_ll_cols_case(c):
    p, d, _lib = _device(c)
    call = _call(c)
    try:
        d.set_option(99, GR.dbg_word(c['nloop']))
        for kern in ((0,) if p.kind == 'exp' else (0, 1)):
            g = GR.case_geometry(c, kern)
            ref = GR.reference(c, *call, opt_gibbs=kern)
            got, names = _ll(d, _lib, p, c, kern)
            assert names == g['kernels'], (names, g)
            _same_geometry(d, g)                                    # the forced nloop, nsplit, sblk, same_pre ... really ran
            again, names2 = _ll(d, _lib, p, c, kern)
            assert names2 == g['kernels']
            assert got.tobytes() == again.tobytes()                 # fixed summation order: identical bits
            _check(c, got, ref, g['path'])
    finally:
        d.set_option(99, 0)
        d.set_option(_lib.OPT_GIBBS_KERNEL, 0)
        d.close()


def test_forced_loop_values_on_one_handle():
    """the forced nloop values one after the other on ONE handle (the partial buffers are reused between the layouts); the
    device reports the loop it ran.  The older 4-bit field of the debug option still forces 1 .. 15; 16 << 8 is its same_pre
    switch and forces nothing."""
    from theano_pyglm_amd import _lib
    c = [c for c in CASES if c['name'] == 'nloop_3'][0]
    p, d, _ = _device(c)
    call = _call(c)
    ref = GR.reference(c, *call)
    t_lo, t_hi = GR.case_range(c)
    mx = GR.max_events(c, c['cols'], t_lo, t_hi)
    try:
        for word in [GR.dbg_word(n) for n in (16, 1, 8, 2, 3, 0)] + [15 << 8, 16 << 8]:
            g = GR.geometry(len(c['cols']), len(c['w']), c['pre'], t_hi - t_lo, mx, p.kind, 0, R=GR.taps(p), opt_dbg=word)
            d.set_option(99, word)
            got, _names = _ll(d, _lib, p, c, 0)
            dev = _same_geometry(d, g)
            assert dev['nloop'] == (GR.dbg_nloop(word) or 1) and dev['nblk'] == -(-8 // dev['nloop'])
            _check(c, got, ref, 'dbg=%#x' % word)
    finally:
        d.set_option(99, 0)
        d.close()


def test_pair_entry_point_23_weights():
    """pgl_gibbs_prepare + pgl_gibbs_ll (two launches for 23 weights) against the same reference; its kernels
    (k_ll_current, all f64) are not those of pgl_gibbs_ll_cols, so E = 0 and there is no bit-for-bit statement to make
    between the two entry points; the one-column pgl_gibbs_ll_cols calls on the same weights are held to the reference too"""
    from theano_pyglm_amd import _lib
    c = [c for c in CASES if c['form'] == 'pair'][0]
    p, d, _ = _device(c)
    cols, pre, ws, t_lo, t_hi = _call(c)
    try:
        for kern in (0, 1):
            d.set_option(_lib.OPT_GIBBS_KERNEL, kern)
            one = d.gibbs_ll_cols(cols, pre, p.Weff[pre, cols], ws)          # 16 + 7 weights
            _check(c, one, GR.reference(c, cols, pre, ws, t_lo, t_hi, opt_gibbs=kern), 'cols/%d' % kern)
        ref = GR.reference(c, cols, pre, ws, t_lo, t_hi, opt_gibbs=1)
        d.gibbs_prepare(cols[0], p.theta[cols[0]], p.Weff[:, cols[0]])
        got = d.gibbs_ll(pre[0], p.Weff[pre[0], cols[0]], ws[0])[None, :]
        assert np.array_equal(got, d.gibbs_ll(pre[0], p.Weff[pre[0], cols[0]], ws[0])[None, :])
        _check(c, got, ref, 'pair')
    finally:
        d.set_option(_lib.OPT_GIBBS_KERNEL, 0)
        d.close()


def test_time_range_off_the_tile_grid_is_refused():
    c = [c for c in CASES if c['name'] == 'subrange_off_grid'][0]
    p = GR.problem(c)
    d = p.device()
    try:
        with pytest.raises(Exception, match='multiple of 16'):
            d.set_time_range(323, 1001)
    finally:
        d.close()


@pytest.mark.parametrize('c', UPD_CASES, ids=lambda c: c['name'])
def test_update_cols_case(c):
    p, d, _lib = _device(c)
    cols, pre, ws, t_lo, t_hi = _call(c)
    delta = np.asarray(c['update']['delta'])
    nrows = t_hi - t_lo
    others = [n for n in range(p.N) if n not in cols]
    try:
        before = np.stack([d.gibbs_currents(n, nrows) for n in range(p.N)], axis=1)
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d.gibbs_update_cols(cols, pre, delta)
        assert d.last_kernels() == ['k_gibbs_update_cols']
        after = np.stack([d.gibbs_currents(n, nrows) for n in range(p.N)], axis=1)
        # the columns not listed keep their bits
        assert after[:, others].tobytes() == before[:, others].tobytes()
        # the update alone, at its bound: against the device's own currents before it
        full = np.zeros((p.nT, len(cols)))
        full[t_lo:t_hi] = before[:, cols]
        x, bd = GR.updated_currents(c, cols, pre, delta, base=full)
        err = np.abs(after[:, cols] - x[t_lo:t_hi]).astype(float)
        assert np.all(np.isfinite(after))
        assert np.all(err <= bd[t_lo:t_hi]), float(np.max(err - bd[t_lo:t_hi]))
        # against the longdouble GX: the same bound plus the forward pass's allowance
        xl, bdl = GR.updated_currents(c, cols, pre, delta)
        fwd = GR.forward_bound(c, cols)
        errl = np.abs(after[:, cols] - xl[t_lo:t_hi]).astype(float)
        with np.errstate(all='ignore'):
            q = np.where(bdl[t_lo:t_hi] > 0, errl / bdl[t_lo:t_hi], np.where(errl > 0, np.inf, 0.0))
        print('gibbs update %-20s worst |x_dev - x_ref| / (1e-13 (|x| + |delta| T)) = %.3g, with the forward term %.3g'
              % (c['name'], float(np.max(q)), float(np.max(errl / np.maximum(bdl + fwd, 1e-300)[t_lo:t_hi]))))
        assert np.all(errl <= (bdl + fwd)[t_lo:t_hi])
        # a zero delta leaves the column's bits alone
        for i in np.flatnonzero(delta == 0.0):
            assert after[:, cols[i]].tobytes() == before[:, cols[i]].tobytes()
        # ll on the updated state == ll of a freshly prepared handle with the new weights, both within the ll bound
        W2 = p.Weff.copy()
        W2[pre, cols] += delta
        c2 = dict(c)
        c2['problem'] = dict(c['problem'])
        c2['problem']['edits'] = list(c['problem']['edits']) + [{'aw': [int(j), int(n)], 'value': float(W2[j, n])} for n, j in zip(cols, pre)]
        p2 = GR.problem(c2)
        d2 = p2.device()
        try:
            if c['t'] is not None:
                d2.set_time_range(*c['t'])
            d2.gibbs_prepare_all(p2.theta, p2.Weff)
            for kern in (0, 1):
                ref = GR.reference(c2, cols, pre, ws, t_lo, t_hi, opt_gibbs=kern)
                d.set_option(_lib.OPT_GIBBS_KERNEL, kern)
                d2.set_option(_lib.OPT_GIBBS_KERNEL, kern)
                _check(c, d.gibbs_ll_cols(cols, pre, p2.Weff[pre, cols], ws), ref, 'updated/%d' % kern)
                _check(c, d2.gibbs_ll_cols(cols, pre, p2.Weff[pre, cols], ws), ref, 'fresh/%d' % kern)
        finally:
            d2.close()
    finally:
        d.set_option(_lib.OPT_GIBBS_KERNEL, 0)
        d.close()


def test_update_refuses_duplicate_columns():
    c = UPD_CASES[1]
    p, d, _lib = _device(c)
    try:
        before = d.gibbs_currents(2, p.nT)
        with pytest.raises(Exception, match='duplicate'):
            d.gibbs_update_cols([2, 5, 2], [1, 3, 4], [0.5, 0.5, 0.5])
        assert d.gibbs_currents(2, p.nT).tobytes() == before.tobytes()
    finally:
        d.close()
