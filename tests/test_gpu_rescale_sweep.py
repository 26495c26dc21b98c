"""k_rescale_chunk / k_rescale_scan / k_rescale_finish over the shapes where their own geometry can break:
tests/rescale_cases.json, one case per edge -- a single short chunk, whole chunks with events on their edges, last chunks
that are no multiple of the 8-row unroll with events right behind t_hi, 64 / 66 / 129 / 111 chunks (per = 1, 2, 3 of the
64-segment scan, with and without empty segments) holding isolated neurons whose consecutive events lie one, two, three and
nchunks - 1 chunks apart and a dense neuron of > 1024 events, N = 1 / 16 / 17 / 40 (xs = 48) / 70, and, at N = 16 where every
lane of a wave holds a neuron, currents wholly inside each series of pgl_lambda_only (both signs), mixed, and exp with
biases from -20 to 8.  tests/test_rescale_cases.py proves on the CPU that each case reaches what it names and that the
bound below rejects four emulated defects of the decomposition.

Per (case, range): pgl_rescale_dev over NaN-filled outputs, twice (identical bits); offsets = pgl_rescale_count = the
reference's; event and multi-spike counts exact; |tau_dev - tau_ref| <= 1e-10 tau_ref + 1e-12 Lambda_ref and |Lambda_dev -
Lambda_ref| <= (1e-10 + 1e-12) Lambda_ref against tests/rescale_reference.reference (longdouble rate and cumsum on the
oracle's features) -- the bound of tests/test_gpu_gof.py; no NaN left.

Worst ratio per case on the MI355X: docs/NOTEBOOK.md, "Rescaling and simulation sweep"."""
import numpy as np
import pytest

from tests import rescale_reference as RR
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

CASES = RR.load_cases()


def _run_twice(d, p, off):
    import torch
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W = t(p.theta), t(p.Weff)
    d_off = torch.tensor(off, dtype=torch.int64, device='cuda')
    outs = []
    for _ in range(2):
        d_tau = torch.full((max(int(off[-1]), 1),), float('nan'), dtype=torch.float64, device='cuda')
        d_st = torch.full((p.N, 4), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        d.rescale_dev(d_th.data_ptr(), d_W.data_ptr(), d_tau.data_ptr(), d_off.data_ptr(), d_st.data_ptr())
        d.sync()
        outs.append((d_tau.cpu().numpy()[:int(off[-1])].copy(), d_st.cpu().numpy().copy()))
    return outs


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_rescale_case(c):
    p = RR.problem(c)
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        for t_lo, t_hi, hits in RR.ranges(c):
            label = "%s [%d, %d)" % (c['name'], t_lo, t_hi)
            taus_ref, stats_ref = ref = RR.reference(c, t_lo, t_hi)
            d.set_time_range(t_lo, t_hi)
            off = d.rescale_count()
            assert np.array_equal(off, RR.offsets(taus_ref)), label
            (tau, st), (tau2, st2) = _run_twice(d, p, off)
            names = d.last_kernels()
            assert names[-3:] == ['k_rescale_chunk<%d>' % (c['kind'] == 'explinear'), 'k_rescale_scan', 'k_rescale_finish'], names
            assert tau.tobytes() == tau2.tobytes() and st.tobytes() == st2.tobytes(), label + ": two calls differ"
            assert np.all(np.isfinite(tau)) and np.all(np.isfinite(st)), label + ": an output was never written"
            assert np.array_equal(st[:, 1], stats_ref[:, 1]), label + ": event counts"
            assert np.array_equal(st[:, 2], stats_ref[:, 2]), label + ": multi-spike bins"
            assert np.all(st[:, 3] == 0.0)
            rt, rl = RR.ratios(tau, off, st[:, 0], ref)
            print("%s: worst |dtau| / (1e-10 tau + 1e-12 Lambda) = %.3e, worst |dLambda| / (1.01e-10 Lambda) = %.3e  (%d intervals)"
                  % (label, rt, rl, int(off[-1])))
            assert rt <= 1.0, label
            assert rl <= 1.0, label
            if 'events-behind-t_hi' in hits:           # the same intervals as on a recording that ends at t_hi
                S = p.S[:t_hi]
                for n in range(p.N):
                    assert st[n, 1] == np.count_nonzero(S[t_lo:, n])
    finally:
        d.close()
