"""Single values of the curvature c(x, s) of pgl_curvature, observed through a Hessian-vector product.

Weff = 0 and no stimulus: the current of neuron n is its bias b_n in every bin.  Every bin of a column holds the same
spike count s, nT = 16 (a power of two: one time tile), v = the unit bias vector: (H v)[n][0] = nT c(b_n, s).  +-inf and
NaN enter through the bias.  Two paths: the rows layout of k_hvp_curv (the 3-phase path: 22 neurons on the automatic
dispatch) and its slab layout (PGL_OPT_KERNEL = 4: k_hvp5 on the same 66 feature columns).

Exact expectations (csrc/pglm_hvp.hip.h): NaN -> NaN; explinear at +-inf -> 0; exp at x >= 709 -> -dt e^709, finite and
the same bits for 709, its successor, 710, 1e308 and +inf; exp at -inf -> +-0.  Finite c whose exact value is a normal
double: relative error against mpmath at most 32 times the worst error the same branch formulas make in numpy float64
(libm) on this grid, and never more than 1e-10; an exact value below the normal range (c at -745, the rate term at
x >= 709) has no relative accuracy to ask for: |c| <= DBL_MIN and the sign of the limit.

Measured: numpy float64 against mpmath on this grid 6.90e-15 (the 'mid' branch beside ln 1e-2, where lam - e keeps 1/200
of its terms; exp 9.95e-17, pos 3.29e-16, rate 2.19e-16, series 2.50e-16): the device's limit is 2.2e-13.
Device (MI355X) against mpmath, worst per branch: rows layout exp 4.34e-16, mid 7.32e-15, pos 6.63e-16, rate 4.34e-16,
series 3.64e-16 (these include the sum over the 16 bins); slab layout exp 1.15e-16, mid 6.90e-15, pos 3.29e-16,
rate 2.19e-16, series 2.50e-16.  First run of this grid: c(+-inf) and c(1e308) of explinear and c(-inf) of exp were NaN
on both layouts (pgl_exp's range reduction subtracts inf from inf); pgl_curvature now clamps the exponential's argument."""
import numpy as np
import pytest

from tests import helpers as H
from tests import hvp_reference as R

pytestmark = pytest.mark.gpu

NT, B, DT = 16, 3, 0.001


def _products(kind, s, bias, opt_kernel):
    from theano_pyglm_amd import _lib
    N = len(bias)
    d = _lib.DeviceGlm(N, NT, B, 200, kind, DT, 0)
    try:
        d.set_spikes(np.full((NT, N), s, dtype=np.uint8))
        d.set_basis(np.ascontiguousarray(H.std_ibasis(200)[:, :B]))
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d.set_option(_lib.OPT_KERNEL, opt_kernel)
        theta = np.zeros((N, d.P))
        theta[:, 0] = bias
        V = np.zeros((N, d.P))
        V[:, 0] = 1.0
        hv = d.hvp(theta, V, np.zeros((N, N)))
        return hv[:, 0] / NT, d.last_kernels()
    finally:
        d.close()


def test_curvature_grid_on_both_layouts():
    pytest.importorskip('mpmath')
    bias = R.curvature_grid()
    N = len(bias)
    fin = np.isfinite(bias)
    cpu = R.grid_cpu_error(DT)
    limit = min(32.0 * max(cpu.values()), 1e-10)
    print("\nnumpy-f64 branch formulas against mpmath: %s; device limit %.2e"
          % (', '.join('%s %.2e' % kv for kv in sorted(cpu.items())), limit))
    failed, worst = [], {}
    for layout, ok in (('rows', 0), ('slab', 4)):
        for kind in ('explinear', 'exp'):
            for s in R.GRID_S:
                c, names = _products(kind, s, bias, ok)
                assert names[0].startswith('k_hvp5<' if ok else 'k_fused2<'), (layout, names)
                tag = "%s %s s=%d" % (layout, kind, s)
                ipos, ineg, inan = N - 3, N - 2, N - 1
                if not np.isnan(c[inan]):
                    failed.append("%s: c(NaN) = %r" % (tag, c[inan]))
                if kind == 'explinear':
                    if c[ipos] != 0.0 or c[ineg] != 0.0:
                        failed.append("%s: c(+inf) = %r, c(-inf) = %r, expected 0" % (tag, c[ipos], c[ineg]))
                else:
                    top = [i for i in range(N) if bias[i] >= 709.0]
                    assert len(top) == 5
                    if not (np.isfinite(c[top[0]]) and all(c[i] == c[top[0]] for i in top)):
                        failed.append("%s: c at x >= 709 not one finite value: %r" % (tag, c[top]))
                    if c[ineg] != 0.0:
                        failed.append("%s: c(-inf) = %r, expected +-0" % (tag, c[ineg]))
                for i in np.nonzero(fin)[0]:
                    exact = R.curvature_mp(bias[i], s, kind, DT)
                    if abs(exact) < R.DBL_MIN:
                        if not (abs(c[i]) <= R.DBL_MIN and c[i] <= 0.0):
                            failed.append("%s: c(%r) = %r, exact %.3e is below the normal range" % (tag, bias[i], c[i], float(exact)))
                        continue
                    err = float(abs((c[i] - exact) / exact))
                    k = layout + ' ' + R.branch(bias[i], s, kind)
                    worst[k] = max(worst.get(k, 0.0), err)
                    if not err <= limit:
                        failed.append("%s: c(%r) = %r, exact %.17g: relative error %.2e > %.2e"
                                      % (tag, bias[i], c[i], float(exact), err, limit))
    print("device against mpmath, worst relative error per layout and branch: %s"
          % ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))
    assert not failed, "%d values failed:\n%s" % (len(failed), "\n".join(failed))
    assert len(worst) == 10
