"""
What the lock-step drivers (batched_bfgs, batched_newton_cg, batched_prox, batched_hmc, batched_nuts, batched_ais) share:
the stream their launches run on and the evaluation of all rows of a neuron range.
"""
import contextlib

# the drivers' stream: one per device, kept between calls (a fresh stream costs its first wait ~6 ms: the hardware queue
# behind it is created on first use)
_STREAMS = {}


@contextlib.contextmanager
def session(population):
    """with session(population) as (torch, dev, stream, handles): the device handles of every data sequence, switched to the
    drivers' stream (pgl_set_stream) behind whatever the caller queued, with that stream current for torch.  On the way
    out -- also on the error path: kernels still queued read the driver's state and the handles' scratch, and must finish
    before the caching allocator reuses the tensors -- the stream is drained and the handles go back to their own streams."""
    import torch
    dev = torch.device('cuda', population.device)
    handles = []
    for data in population.data_sequences:
        population.set_data(data)
        handles.append(population._handle(data))
    stream = _STREAMS.get(dev.index)
    if stream is None:
        stream = _STREAMS[dev.index] = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for h in handles:
        h.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            yield torch, dev, stream, handles
    finally:
        try:
            stream.synchronize()
        except Exception:
            pass
        for h in handles:
            h.set_stream(None)


class RangeEvaluator(object):
    """ll and its gradient of the rows [n_lo, n_hi) at X (M, P): one pgl_ll_grad_dev per data sequence into that sequence's
    [ll | grad] buffer, summed into the first.  evaluator(X) -> (ll (M,), grad (M, P)), views of the first buffer, valid
    until the next call; .count: the calls so far.
    n_chains = C > 1: X is (C M, P), chain-major (row c M + m: chain c of neuron n_lo + m), the buffers hold C M rows and a
    call is C pgl_ll_grad_dev per data sequence, one per chain block; .count still counts calls."""

    def __init__(self, torch, dev, handles, Weff, M, P, n_lo, n_hi, n_chains=1):
        self.handles, self.Weff, self.M, self.n_lo, self.n_hi = handles, Weff, M, n_lo, n_hi
        self.P, self.C, self.R = P, int(n_chains), M * int(n_chains)
        self.bufs = [torch.empty(self.R * (1 + P), dtype=torch.float64, device=dev) for _ in handles]
        self.count = 0

    def __call__(self, X):
        M, R, P, tot = self.M, self.R, self.P, None
        for h, buf in zip(self.handles, self.bufs):
            if self.C == 1:
                h.ll_grad_dev(X.data_ptr(), self.Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), self.n_lo, self.n_hi)
            else:
                xp, lp, gp = X.data_ptr(), buf.data_ptr(), buf[R:].data_ptr()
                for c in range(self.C):
                    h.ll_grad_dev(xp + 8 * c * M * P, self.Weff.data_ptr(), lp + 8 * c * M, gp + 8 * c * M * P, self.n_lo,
                                  self.n_hi)
            tot = buf if tot is None else tot.add_(buf)
        self.count += 1
        return tot[:R], tot[R:]
