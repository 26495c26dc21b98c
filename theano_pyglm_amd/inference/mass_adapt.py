"""
Host side of the warm-up mass adaptation and of several chains per neuron of the lock-step samplers (batched_hmc,
batched_nuts): the window schedule, the seeds of the chains, the jitter of their starting points and split-R-hat.  The
device side -- the Welford estimate, the shrinkage and the restart of the step-size adaptation -- is csrc/pglm_adapt.h.
"""
import numpy as np

_MASK = (1 << 64) - 1
_G = 0x9e3779b97f4a7c15
JITTER_T = _MASK                                              # the 'transition' whose key the start jitter is drawn from


def adapt_windows(n_warmup):
    """The windows [(start, end), ...] of transitions t (start <= t < end) over which the diagonal mass is estimated, for a
    warm-up of n_warmup transitions: Stan's schedule.  n < 20: none.  n >= 150: init = 75, term = 50, base = 25; else init
    = floor(0.15 n), term = floor(0.10 n), base = n - init - term.  Windows start at init, have sizes base, 2 base, 4 base,
    ... and tile [init, n - term): a window is stretched to n - term unless its doubled successor would end before
    n - term (Stan's rule, next boundary >= n - term: 300 gives (75, 100), (100, 250))."""
    n = int(n_warmup)
    if n < 20:
        return []
    if n >= 150:
        init, term, base = 75, 50, 25
    else:
        init, term = int(0.15 * n), int(0.10 * n)
        base = n - init - term
    last = n - term
    out, start, size = [], init, base
    while start < last:
        end = start + size
        if end + 2 * size >= last:
            end = last
        out.append((start, end))
        start, size = end, 2 * size
    return out


def schedule_ints(windows):
    """The kernels' form of a schedule (csrc/pglm_adapt.h): [n_win, start of window 0, end of window 0, end of window 1, ...]."""
    return np.array([len(windows), windows[0][0] if windows else 0] + [e for _, e in windows], dtype=np.int32)


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _MASK
    return z ^ (z >> 31)


def chain_seed(seed, c):
    """The seed chain c of a run with `seed` runs on (pgl_chain_seed of csrc/pglm_adapt.h): the seed itself for c = 0, else
    mix(mix(seed + G) ^ (G c)) in 64-bit arithmetic, mix and G the generator's (pgl_hmc_mix, include/pyglm_hip.h)."""
    seed, c = int(seed) & _MASK, int(c)
    if c < 0:
        raise ValueError("chain index must not be negative")
    if c == 0:
        return seed
    return _mix(_mix((seed + _G) & _MASK) ^ ((_G * c) & _MASK))


def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def start_jitter(seed, neuron, P):
    """P standard normals for the start of the row of `neuron` in a chain with `seed`: the generator of the chains
    (pgl_hmc_key / pgl_hmc_normal, include/pyglm_hip.h) under the key of (seed, neuron, t = 2^64 - 1), a transition no chain
    reaches, so the draws are used nowhere else.  Computed on the host (numpy's log and cos)."""
    key = _mix((_mix((_mix((int(seed) + _G) & _MASK) + _G * (int(neuron) + 1)) & _MASK) + _G * (JITTER_T + 1)) & _MASK)
    with np.errstate(over='ignore'):
        k = np.arange(1, 2 * int(P) + 1, dtype=np.uint64)
        z = _mix_np(np.uint64(key) + np.uint64(_G) * (k + np.uint64(1)))
    u = ((z >> np.uint64(11)).astype(float) + 0.5) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u[0::2])) * np.cos(6.283185307179586 * u[1::2])


def rhat(samples):
    """Split-R-hat of samples (n_chains, n_draws, ...) -> array shaped like one draw.  The PLAIN (not rank-normalised)
    split-R-hat of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021), "Rank-normalization, folding, and localization: an
    improved R-hat for assessing convergence of MCMC", eqs. 1-4: every chain is split into halves (the middle draw of an odd
    number is dropped), W = the mean within-half variance (n - 1), B / n = the variance of the half means (m - 1), R-hat =
    sqrt(((n - 1) / n W + B / n) / W).  A parameter that is constant in every half gives NaN."""
    s = np.asarray(samples, dtype=float)
    if s.ndim < 2 or s.shape[1] < 4:
        raise ValueError("rhat: samples (n_chains, n_draws >= 4, ...)")
    h = s.shape[1] // 2
    halves = np.concatenate([s[:, :h], s[:, s.shape[1] - h:]], axis=0)         # (2 C, h, ...)
    W = halves.var(axis=1, ddof=1).mean(axis=0)
    Bn = halves.mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt(((h - 1.0) / h * W + Bn) / W)
