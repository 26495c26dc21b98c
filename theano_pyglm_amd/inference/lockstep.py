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
    until the next call; .count: the calls so far."""

    def __init__(self, torch, dev, handles, Weff, M, P, n_lo, n_hi):
        self.handles, self.Weff, self.M, self.n_lo, self.n_hi = handles, Weff, M, n_lo, n_hi
        self.bufs = [torch.empty(M * (1 + P), dtype=torch.float64, device=dev) for _ in handles]
        self.count = 0

    def __call__(self, X):
        M, tot = self.M, None
        for h, buf in zip(self.handles, self.bufs):
            h.ll_grad_dev(X.data_ptr(), self.Weff.data_ptr(), buf.data_ptr(), buf[M:].data_ptr(), self.n_lo, self.n_hi)
            tot = buf if tot is None else tot.add_(buf)
        self.count += 1
        return tot[:M], tot[M:]
