"""
What the lock-step drivers share.
All of them (batched_bfgs, batched_newton_cg, batched_newton, batched_prox, batched_hmc, batched_nuts, batched_ais,
batched_smc): session, the stream their launches run on, and RangeEvaluator, the evaluation of all rows of a neuron range.
The optimisers on theta rows (batched_newton_cg, batched_newton; batched_prox for the flags): what they serve (supported,
_check), the pinned phase flags and list staging (_host_buffers, send_list), the evaluation of a row list
(RangeEvaluator.eval_list), the wait for a launch's flags (wait) and the line-search phase of an outer iteration
(search_phase).  batched_bfgs keeps its own staging: its flags are a ring, its loop a pipeline.  batched_hmc and
batched_ais keep their wait: it drains the stream and is counted.
"""
import contextlib

import numpy as np

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
    eval_list(Xt, idx32, L) -> (ll (L,), grad (L, P)): the same for the L listed neurons idx32 (device int32) at Xt (L, P),
    one pgl_ll_grad_list_dev per data sequence, in the front of the same buffers; .list_count, .list_rows: its calls and rows.
    n_chains = C > 1: X is (C M, P), chain-major (row c M + m: chain c of neuron n_lo + m), the buffers hold C M rows and a
    call is C pgl_ll_grad_dev per data sequence, one per chain block; .count still counts calls."""

    def __init__(self, torch, dev, handles, Weff, M, P, n_lo, n_hi, n_chains=1):
        self.handles, self.Weff, self.M, self.n_lo, self.n_hi = handles, Weff, M, n_lo, n_hi
        self.P, self.C, self.R = P, int(n_chains), M * int(n_chains)
        self.bufs = [torch.empty(self.R * (1 + P), dtype=torch.float64, device=dev) for _ in handles]
        self.count = 0
        self.list_count = self.list_rows = 0

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

    def eval_list(self, Xt, idx32, L):
        P, tot = self.P, None
        for h, full in zip(self.handles, self.bufs):
            buf = full[:L * (1 + P)]
            h.ll_grad_list_dev(idx32.data_ptr(), L, Xt.data_ptr(), self.Weff.data_ptr(), buf.data_ptr(), buf[L:].data_ptr())
            tot = buf if tot is None else tot.add_(buf)
        self.list_count += 1
        self.list_rows += L
        return tot[:L], tot[L:]


# ---- the optimisers whose per-neuron vector is the device's theta row (Newton-CG, dense Newton) ----------------------
def supported(population):
    return population.glm.hvp_packing() is None


def _check(population):
    bad = population.glm.hvp_packing()
    if bad is not None:
        raise ValueError("lock-step Newton-CG: Hessian-vector products are not implemented for the %s packing" % bad)
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("lock-step Newton-CG does not run on a time-sharded population (set_time_shard): "
                         "products and evaluations are not all-reduced")


_HOST_BUFFERS = {}


def _host_buffers(torch, device_index, M):
    """Pinned phase flags and list staging of a fit, kept between fits: {(device, M): (flags, staging)}."""
    key = (int(device_index), int(M))
    hb = _HOST_BUFFERS.get(key)
    if hb is None:
        if len(_HOST_BUFFERS) > 16:
            _HOST_BUFFERS.clear()
        hb = (torch.zeros(M, dtype=torch.float64).pin_memory(), torch.empty(3 * M, dtype=torch.int32).pin_memory())
        _HOST_BUFFERS[key] = hb
    return hb


def send_list(stage, lists, rows, n_lo, M):
    """A row list travels as ONE copy of [its rows | its neurons] (int32) from the pinned staging; returns its length."""
    L = int(rows.size)
    sg = stage.numpy()
    sg[:L] = rows
    sg[M:M + L] = rows + n_lo
    lists.copy_(stage, non_blocking=True)
    return L


def wait(stream, event):
    """Until everything queued on the stream so far has run: the row kernels' pinned flags are then current."""
    event.record(stream)
    event.synchronize()


def search_phase(fl, searching, M, n_lo, stage, lists, Xts, evaluate, trial, step, stream, event):
    """The line-search phase of an outer iteration: the rows whose flag fl[r] is `searching`, one evaluation per trial
    step, until none searches.  A new list is sent and its trial points computed, trial(L, Xt); later ones come from the
    step kernel, which writes the next launch's points itself: step(L, Xt, ft, gt, Xt_next) behind
    evaluate(Xt, neurons, L) -> (ft, gt).  Xts: two (M, P) buffers that alternate.  Returns the trial launches."""
    rows = np.nonzero(fl == searching)[0].astype(np.int32)
    launch = 0
    listed = None
    while rows.size:
        L = int(rows.size)
        cur, nxt = Xts[launch & 1], Xts[(launch + 1) & 1]
        if listed is None or listed.size != L:
            send_list(stage, lists, rows, n_lo, M)           # (the trial points of a new list are recomputed)
            listed = rows
            trial(L, cur)
        ft, gt = evaluate(cur, lists[M:M + L], L)
        step(L, cur, ft, gt, nxt)
        wait(stream, event)
        launch += 1
        rows = listed[fl[listed] == searching]
    return launch
