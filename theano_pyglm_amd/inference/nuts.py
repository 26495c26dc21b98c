"""
The No-U-Turn transition, stated readably: multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017) in the whitened
momentum r = W^T p, K = 1/2 sum r^2, the inverse mass matrix being W W^T -- the rules that include/pyglm_hip.h fixes for
the device chain (csrc/pglm_nuts.h, inference/batched_nuts.py).  The leaves of the running subtree are kept in a LIST and
every U-turn test sums its block of the list: nothing here is shared with the O(max_depth) state machine, which is tested
against this statement (tests/test_nuts_host.py).  numpy only.
"""
import numpy as np

STOP_SUB, STOP_TREE, STOP_DEPTH, STOP_DIVERGENT = 1, 2, 3, 4
DIVERGE = 1000.0


def random_draws(rng, P, max_depth):
    """The draws one transition consumes: (z (P,), u_dir (max_depth,), u_merge (max_depth,), u_leaf (2^max_depth - 1,))."""
    return (rng.standard_normal(P), rng.uniform(size=max_depth), rng.uniform(size=max_depth),
            rng.uniform(size=2 ** max_depth - 1))


def _uturn(rs):
    rho = np.sum(rs, axis=0)
    return not (rho.dot(rs[0]) > 0.0 and rho.dot(rs[-1]) > 0.0)


def nuts_transition(q0, U0, g0, target, step, max_depth, z, u_dir, u_merge, u_leaf, W=None):
    """One transition from q0 (U0, g0 = U and grad U there).  target(q) -> (U, grad U).  W: the (P, P) lower-triangular
    factor of the inverse mass matrix (its strict upper triangle is ignored) or None.  z: the momentum r; u_dir[d],
    u_merge[d]: the uniforms of doubling d; u_leaf[2^d - 1 + i]: of leaf i of doubling d.
    -> dict: 'q', 'U', 'g' the next point; 'depth' doublings begun; 'n_leaf' leapfrog steps; 'stop' (STOP_*); 'sel' the
    leaf number 2^d - 1 + i of the next point (-1: q0 stays); 'alpha' the acceptance statistic; 'divergent'."""
    P = q0.size
    Wm = np.eye(P) if W is None else np.tril(np.asarray(W, dtype=float))
    h0 = Wm.T.dot(g0)
    H0 = U0 + 0.5 * z.dot(z)
    left = right = (q0, z, h0)
    rho = z.copy()
    lw_tree = 0.0
    cand, sel = (q0, U0, g0), -1
    sum_acc, n_leaf, depth, stop = 0.0, 0, 0, 0
    while not stop:
        d = depth
        depth += 1
        v = 1.0 if u_dir[d] < 0.5 else -1.0
        q, r, h = right if v > 0 else left
        leaves, sub, sel_sub, lw_sub = [], None, -1, -np.inf
        for i in range(2 ** d):
            r = r - 0.5 * v * step * h
            q = q + v * step * Wm.dot(r)
            U, g = target(q)
            h = Wm.T.dot(g)
            r = r - 0.5 * v * step * h
            with np.errstate(all='ignore'):
                dH = U + 0.5 * r.dot(r) - H0
            n_leaf += 1
            if not np.isfinite(dH) or dH > DIVERGE:
                stop = STOP_DIVERGENT
                break
            sum_acc += min(1.0, np.exp(-dH))
            lw_sub = np.logaddexp(lw_sub, -dH)
            if i == 0 or np.log(u_leaf[2 ** d - 1 + i]) < -dH - lw_sub:
                sub, sel_sub = (q, U, g), 2 ** d - 1 + i
            leaves.append(r)
            k = 1
            while (i + 1) % 2 ** k == 0:                      # every aligned block of 2^k leaves that ends here
                if _uturn(leaves[i + 1 - 2 ** k:i + 1]):
                    stop = STOP_SUB
                k += 1
            if stop:
                break
        if stop:
            break
        if np.log(u_merge[d]) < lw_sub - lw_tree:
            cand, sel = sub, sel_sub
        lw_tree = np.logaddexp(lw_tree, lw_sub)
        rho = rho + np.sum(leaves, axis=0)
        if v > 0:
            right = (q, r, h)
        else:
            left = (q, r, h)
        if not (rho.dot(left[1]) > 0.0 and rho.dot(right[1]) > 0.0):
            stop = STOP_TREE
        elif depth >= max_depth:
            stop = STOP_DEPTH
    return {'q': cand[0], 'U': cand[1], 'g': cand[2], 'depth': depth, 'n_leaf': n_leaf, 'stop': stop, 'sel': sel,
            'alpha': sum_acc / n_leaf, 'divergent': stop == STOP_DIVERGENT}


def dual_averaging_steps(step0, alphas, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, lo=1e-4, hi=10.0):
    """Step sizes of Hoffman & Gelman's algorithm 5 from the acceptance statistics alphas (n_warmup,) of the warm-up
    transitions: -> (n_warmup,) the step after each, the last one being the frozen exp(log eps bar)."""
    mu, hbar, lebar, out = np.log(10.0 * step0), 0.0, 0.0, []
    n = len(alphas)
    for m in range(1, n + 1):
        hbar = (1.0 - 1.0 / (m + t0)) * hbar + (delta - alphas[m - 1]) / (m + t0)
        le = mu - np.sqrt(m) / gamma * hbar
        eta = m ** -kappa
        lebar = eta * le + (1.0 - eta) * lebar
        out.append(min(max(np.exp(lebar if m == n else le), lo), hi))
    return np.array(out)
