"""The case table of the collapsed-Gibbs column sweep (tests/gibbs_cases.json), its longdouble reference, a Python statement of
the host launch arithmetic and a float64 numpy mirror of the regime-split decomposition with switchable defects (test
infrastructure, numpy only, no GPU): tests/test_gibbs_cases.py keeps the table honest on the CPU,
tests/test_gpu_gibbs_sweep.py runs it on the device.

Reference, independent of the device: features from the oracle (a direct time-domain convolution of the spikes), every
current in numpy.longdouble,
    ic[t]  = sum_b fS[t, n_pre, b] beta[n_post][n_pre][b]                       (the impulse current of the pair)
    x_k[t] = bias + x_total[t] - aw ic[t] + w_k ic[t]
    ll_k   = sum_t -dt lam_k + S log lam_k,   A_k = sum_t dt lam_k + S |log lam_k|
with the rate of tests/pointwise_reference.py's longdouble nonlinearity and the reference model's NaN rule: a bin whose
float64 rate is 0 makes the whole ll_k NaN (log(lam) * S is NaN there even for S = 0).

Bound: |ll_dev - ll_ref| <= 1e-10 |ll_ref| + 1e-12 A + E.  The first two terms are the project's rate-parity bound
(tests/test_gpu_pointwise.py, tests/test_gpu_gof.py).  E is what docs/NOTEBOOK.md section 4.1d grants the single-precision
log1p term of k_gibbs_rate_cols and nothing more: E = dt sum_t e_t with e_t = 6e-12 where x >= 12, 4e-5 exp(x) where
x <= -12, 0 in the band; E = 0 for the exp nonlinearity and for PGL_OPT_GIBBS_KERNEL = 1 (all-f64 kernel).

A case (one launch):
  name, problem {N, nT, kind, seed, rate_hz, w_scale, bias (number | list, resized to N | null), weff (number | null),
  edits [...]}, t (null | [t_lo, t_hi]), cols, pre, w (list of K numbers: the candidate weights of column 0; column c gets
  w (1 + c / 64) + c / 1024 -- every entry of a call distinct), nloop (forced sub-block loop, 0 = the host's choice), form
  ("cols" | "pair": pgl_gibbs_prepare + pgl_gibbs_ll), hits {...}: what tests/test_gibbs_cases.py proves the case reaches.
  Edits of the problem, in order: {"clear": n} no spike of neuron n; {"set": n, "bins": [...], "count": c};
  {"every": n, "t": [a, b], "step": s, "count": c}; {"beta": [post, pre], "values": [B numbers]} the pair's basis weights;
  {"aw": [pre, post], "value": v} one entry of Weff.
An update case has "update": {"delta": [...]}: pgl_gibbs_update_cols over (cols, pre) with these deltas."""
import functools
import json
import os

import numpy as np

from oracle import glm_oracle as O
from tests import helpers as H
from tests import pointwise_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'gibbs_cases.json')
REL, ABS_A = PR.REL, PR.ABS_A
E_POS, E_NEG, X_FAST = 6e-12, 4e-5, 12.0
X_NAN, X_FLUSH = -745.2, -744.3        # no case may put an x inside (X_NAN, X_FLUSH): the all-f64 kernel flushes there
UPD = 1e-13
GRB, GNL, GECAP_R, GECAP, KMAX = 256, 16, 20, 24, 16     # PGL_GRB, PGL_GNL, PGL_GECAP_R, PGL_GECAP, PGL_KMAX
GQ, SPT_N = 256, 196                                     # PGL_GQ, PGL_SPT_N
NUM_CU, WG_PER_CU = 256, 4             # MI355X; occupancy of k_gibbs_rate_cols at <= 40 KB of LDS
DEFECTS = ('f32_from_8', 'drop_ragged', 'drop_last_lag', 'drop_21st', 'swap_1_8', 'spikes_from_256', 'no_aw')


def load_cases():
    with open(CASES) as f:
        cases = json.load(f)
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def case_weights(c):
    """(ncols, K) candidate weights: every entry of a call distinct"""
    w = np.asarray(c['w'], dtype=float)
    ci = np.arange(len(c['cols']), dtype=float)[:, None]
    return w[None, :] * (1.0 + ci / 64.0) + ci / 1024.0


def case_range(c):
    return (0, c['problem']['nT']) if c['t'] is None else tuple(c['t'])


@functools.lru_cache(maxsize=None)
def _problem(key):
    s = json.loads(key)
    kw = {} if s.get('w_scale') is None else {'w_scale': s['w_scale']}
    p = H.Problem(s['N'], s['nT'], H.std_ibasis(), kind=s['kind'], rate_hz=s['rate_hz'], seed=s['seed'], weighted=True, **kw)
    B = p.B
    if s.get('bias') is not None:
        p.theta[:, 0] = np.resize(np.asarray(s['bias'], dtype=float), s['N'])
    if s.get('weff') is not None:
        p.Weff = np.full((s['N'], s['N']), float(s['weff']))
    for e in s.get('edits', []):
        if 'clear' in e:
            p.S[:, e['clear']] = 0
        elif 'set' in e:
            p.S[np.asarray(e['bins'], dtype=int), e['set']] = e['count']
        elif 'every' in e:
            p.S[e['t'][0]:e['t'][1]:e['step'], e['every']] = e['count']
        elif 'beta' in e:
            post, pre = e['beta']
            p.theta[post, 1 + pre * B:1 + (pre + 1) * B] = e['values']
        elif 'aw' in e:
            p.Weff[e['aw'][0], e['aw'][1]] = e['value']
        else:
            raise ValueError(e)
    p._fS = O.convolve_with_basis(p.S.astype(float), p.ibasis)
    for a in (p.S, p.theta, p.Weff):
        a.setflags(write=False)
    return p


def problem(c):
    """helpers.Problem of the case with its edits of spikes, biases and weights (built once, shared, read-only)"""
    return _problem(json.dumps(c['problem'], sort_keys=True))


def taps(p):
    """taps the kernels use: R minus the trailing all-zero basis rows (Rk of pgl_set_basis)"""
    return int(np.flatnonzero(np.abs(p.ibasis).sum(axis=1))[-1]) + 1


@functools.lru_cache(maxsize=None)
def _xtot(key):
    """(x_total without the bias (nT, N) in longdouble, the same in float64 by a float64 product)"""
    p = _problem(key)
    N, B = p.N, p.B
    w = p.theta[:, 1:].reshape(N, N, B)
    Wm = (p.Weff.T[:, :, None] * w).reshape(N, N * B).T
    F = p.fS.reshape(p.nT, N * B)
    xl = F.astype(np.longdouble).dot(Wm.astype(np.longdouble))
    x64 = F.dot(Wm)
    xl.setflags(write=False)
    x64.setflags(write=False)
    return xl, x64


@functools.lru_cache(maxsize=None)
def _abs_features(key):
    """sum over the events of count |phi_b[d]| (nT, N, B): the basis changes sign, the terms of ic are bounded by this"""
    p = _problem(key)
    return O.convolve_with_basis(p.S.astype(float), np.abs(p.ibasis))


def _key(c):
    return json.dumps(c['problem'], sort_keys=True)


def pair_current(c, post, pre, dtype=np.longdouble):
    p = problem(c)
    beta = p.theta[post, 1 + pre * p.B:1 + (pre + 1) * p.B]
    return p.fS[:, pre, :].astype(dtype).dot(beta.astype(dtype))


def currents(c, cols, pre, ws, t_lo, t_hi):
    """x (ncols, nrows, K) in longdouble"""
    p = problem(c)
    xl = _xtot(_key(c))[0]
    out = np.empty((len(cols), t_hi - t_lo, ws.shape[1]), dtype=np.longdouble)
    for i, (n, j) in enumerate(zip(cols, pre)):
        ic = pair_current(c, n, j)[t_lo:t_hi]
        x0 = np.longdouble(p.theta[n, 0]) + xl[t_lo:t_hi, n] - np.longdouble(p.Weff[j, n]) * ic
        out[i] = x0[:, None] + ws[i].astype(np.longdouble)[None, :] * ic[:, None]
    return out


def reference(c, cols, pre, ws, t_lo, t_hi, opt_gibbs=0):
    """(ll, A, E, nanmask), each (ncols, K): ll and A in longdouble, E the section-4.1d allowance of the regime-split path
    (zeros for exp and for opt_gibbs = 1), nanmask where some bin's float64 rate is 0"""
    p = problem(c)
    x = currents(c, cols, pre, ws, t_lo, t_hi)
    lam = PR.RR.rate_longdouble(x, p.kind)
    S = p.S[t_lo:t_hi][:, list(cols)].T[:, :, None].astype(np.longdouble)
    with np.errstate(divide='ignore', invalid='ignore'):
        loglam = x if p.kind == 'exp' else np.log(lam)
        spike = np.where(S > 0, S * np.where(S > 0, loglam, 0), 0)
    dt = np.longdouble(p.dt)
    ll = np.sum(-dt * lam + spike, axis=1)
    A = np.sum(dt * lam + np.abs(spike), axis=1)
    nanmask = np.any(lam.astype(np.float64) == 0.0, axis=1)
    E = np.zeros(ll.shape)
    if p.kind == 'explinear' and opt_gibbs != 1:
        e = np.where(x >= X_FAST, E_POS, np.where(x <= -X_FAST, E_NEG * np.exp(np.minimum(x, 0)), 0.0))
        E = np.asarray(p.dt * np.sum(e, axis=1), dtype=np.float64)
    return ll, A, E, nanmask


def bound(ref):
    ll, A, E, _ = ref
    return np.asarray(REL * np.abs(ll) + ABS_A * A + E, dtype=np.longdouble)


def ratio(dev, ref):
    """worst |ll_dev - ll_ref| / (1e-10 |ll_ref| + 1e-12 A + E) over EVERY entry: where the reference is NaN the device must be
    NaN (quotient 0) and nowhere else; a value that is not finite otherwise, or a shape that differs, is infinitely far"""
    ll, A, E, nanmask = ref
    dev = np.asarray(dev)
    if dev.shape != ll.shape:
        return np.inf
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.abs(dev.astype(np.longdouble) - ll) / bound(ref)
    d = np.where(np.isfinite(d) & np.isfinite(dev), d, np.inf)
    d = np.where(nanmask, np.where(np.isnan(dev), 0.0, np.inf), d)
    return float(np.max(d))


def updated_currents(c, cols, pre, delta, base=None):
    """(x (nT, ncols) in longdouble, bound (nT, ncols)): GX[:, n_post] + delta ic after pgl_gibbs_update_cols, as
    pgl_gibbs_currents returns it (no bias).  base: the currents before the update (nT, ncols) when the update alone is to be
    judged (the device's own, read back by pgl_gibbs_currents); None = the longdouble GX.

    Bound 1e-13 (|x| + |delta| sum |terms of ic|) per bin.  k_gibbs_update_cols builds ic[t] from the E events of the bin's
    window by B fused multiply-adds per event (h = sum_b phi_b[d] beta_b) and one more into the running sum, then one
    into GX: (B + 1) E + 1 roundings of u = 1.1e-16, each relative to a partial sum that is at most T = sum over the events
    and b of |count phi_b[d] beta_b|, so |ic_dev - ic| <= ((B + 1) E + 1) u T.  With B = 5 and E <= 40 events inside the
    179 taps (220 Hz) that is 2.7e-14 T; the final multiply-add rounds the result once more (u |x|).  1e-13 covers both
    with a factor of three to spare.
    The bound has no term for the rounding of GX itself: the forward pass sums N B E products whose signs mix (every
    basis function has negative lobes), so a bin where x nearly cancels carries an error of u sum |terms of x| >> 1e-13 |x|
    whatever computes it (a float64 numpy product misses 1e-13 |x| by up to 6.7x on the update cases of
    tests/gibbs_cases.json, the device by up to 9.9x).  Against the longdouble
    GX the comparison therefore adds forward_bound(); against base = the device's own currents before the update it does not."""
    p = problem(c)
    xl = _xtot(_key(c))[0]
    x = np.empty((p.nT, len(cols)), dtype=np.longdouble)
    bd = np.empty((p.nT, len(cols)))
    for i, (n, j) in enumerate(zip(cols, pre)):
        beta = p.theta[n, 1 + j * p.B:1 + (j + 1) * p.B]
        ic = pair_current(c, n, j)
        terms = _abs_features(_key(c))[:, j, :].dot(np.abs(beta))
        b0 = xl[:, n] if base is None else np.asarray(base[:, i], dtype=np.longdouble)
        x[:, i] = b0 + np.longdouble(delta[i]) * ic
        bd[:, i] = UPD * (np.abs(x[:, i]).astype(float) + abs(delta[i]) * terms)
    return x, bd


def forward_bound(c, cols):
    """1e-13 sum |terms of GX[:, n]| (nT, ncols): the allowance of the forward pass (N B E <= 17 * 5 * 40 multiply-adds of
    u = 1.1e-16 in some order at N = 17, 8 000 at N = 40: 3.7e-13 resp. 8.8e-13 in the worst case, 6e-15 resp. 1e-14 as a
    random walk)"""
    p = problem(c)
    N, B = p.N, p.B
    w = np.abs(p.theta[:, 1:].reshape(N, N, B))
    Wm = (np.abs(p.Weff.T)[:, :, None] * w).reshape(N, N * B).T
    return UPD * _abs_features(_key(c)).reshape(p.nT, N * B).dot(Wm)[:, list(cols)]


# ---- the host arithmetic of pgl_gibbs_ll_cols ---------------------------------------------------------------------------------
def dbg_word(nloop):
    """value of the debug option (99) that forces `nloop` sub-blocks per workgroup: bits 16..20"""
    return int(nloop) << 16


def dbg_nloop(opt_dbg):
    """forced sub-block loop the host reads out of the debug option (0 = none): bits 16..20 when set, else the older 4-bit
    field in bits 8..11 -- 16 << 8 is bit 12, the same_pre switch, and forces nothing"""
    return ((opt_dbg >> 16) & 0x1f) or ((opt_dbg >> 8) & 0xf)


def geometry(ncols, K, n_pre, nrows, max_ev, nlin, opt_gibbs=0, forced_nloop=0, R=179, slots=WG_PER_CU * NUM_CU, opt_dbg=None,
             num_cu=NUM_CU, B=5):
    """What pgl_gibbs_ll_cols launches for ncols columns, K weights, the presynaptic list n_pre, nrows = t_hi - t_lo bins and
    max_ev = the largest number of post-synaptic events of a listed column inside the range.  forced_nloop: the decoded
    forced loop; opt_dbg: the raw debug option instead (decoded as the host does, its bit 0x1000 switches same_pre off).

    An independent statement of the rule of theano_pyglm_amd/csrc/pglm_gibbs_plan.h: pgl_gibbs_dbg (the debug word),
    pgl_gibbs_path, pgl_gibbs_plan_shape (CP, nsplit, ygroups, nsub, same_pre, hs_region, fs_stride, sblk, the LDS bytes; all of
    the all-f64 path: CP = min(ncols, 256 / K), gtb, rows, nblk), pgl_gibbs_plan_loop (nloop, nblk, grid from `slots`) and TS of
    k_gibbs_ll_cols.  tests/test_gibbs_plan_host.py compiles the header with gcc and compares every field with this function on
    the CPU; the sweep compares what the device reports (pgl_gibbs_last_geometry).  The LDS bytes are stated here from the
    kernels' own carve-up of the block (pgl_gibbs_rate_body, k_gibbs_ll_cols in pglm_gibbs.hip.h), region by region.
    `slots` stands for gibbs_rate_wg_per_cu(lds) * numCU, which the host takes from an occupancy query at the launch's LDS size;
    the default is the 4 * 256 of an MI355X at <= 40 KB.  It only enters the unforced nloop = nsub * ygroups / (6 * slots),
    which is below 1 for every launch under 6 144 sub-block units (the case table's largest has 24)."""
    same_pre_on = True
    if opt_dbg is not None:
        forced_nloop = dbg_nloop(opt_dbg)
        same_pre_on = not (opt_dbg & 0x1000)
    n_pre = list(n_pre)
    if nlin == 'explinear' and opt_gibbs != 1 and R + GRB + 32 < 65535:
        CP = min(ncols, 8)
        nsplit = 1 if CP >= 3 else 2 if CP == 2 else 4
        yg = -(-ncols // CP)
        nsub = -(-nrows // GRB)
        same_pre = same_pre_on and ncols >= 2 and all(j == n_pre[0] for j in n_pre)
        nloop = max(1, min(8, nsub * yg // (6 * slots)))
        if forced_nloop:
            nloop = min(GNL, forced_nloop)
        nblk = -(-nsub // nloop)
        sblk = max(1, -(-max_ev // 256))
        kernels = ['k_gibbs_cols_setup'] + (['k_gibbs_pre_features'] if same_pre else []) + ['k_gibbs_rate_cols',
                                                                                               'k_gibbs_reduce_cols2']
        # first region: HS [CP][R], or with the shared train FS [B][GRB + 2] and BT [CP][8] if that is larger
        hs_region = max(CP * R, B * (GRB + 2) + CP * 8) if same_pre else CP * R
        doubles = hs_region + CP * (GRB + 2) + CP * KMAX + 4 * GQ + SPT_N + CP        # X0, Wl, Qx, TB, WM
        lds = 8 * doubles + 8 * CP * GECAP_R + 4 * CP * GNL + 2 * CP * GNL + 16      # evS (int2), WL (int), WN (short), slack
        return dict(path='regime', kernels=kernels, CP=CP, nsplit=nsplit, ygroups=yg, nsub=nsub, nloop=nloop, nblk=nblk, sblk=sblk,
                    same_pre=same_pre, grid=nblk * yg + sblk * ncols, hs_region=hs_region,
                    fs_stride=-(-nrows // 64) * 64 if same_pre else 0, lds=lds)
    CP = max(1, min(ncols, 256 // max(1, K)))
    yg = -(-ncols // CP)
    gtb = 32
    while gtb * CP < 256:
        gtb += 32
    rows = -(-(nrows * yg) // (4 * num_cu))
    rows = max(gtb, min(rows, 384))
    rows = -(-rows // gtb) * gtb
    TS = max(1, 256 // (CP * K))
    lds = 8 * (B * R + 3 * gtb * CP) + 8 * CP * GECAP + 4 * CP                       # phiS, X0 / IC / SS, evS (int2), ecnt (int)
    return dict(path='f64', kernels=['k_gibbs_ll_cols', 'k_gibbs_reduce_cols'], CP=CP, ygroups=yg, gtb=gtb, rows=rows, TS=TS,
                nblk=-(-nrows // rows), same_pre=False, lds=lds)


def update_geometry(ncols, nrows, R=179, B=5):
    """What pgl_gibbs_update_cols launches (pgl_gibbs_plan_update): a thread is a column, blocks of 1024 bins, the basis in LDS"""
    CP = min(ncols, 256)
    return dict(CP=CP, ygroups=-(-ncols // CP), rows=1024, nblk=-(-nrows // 1024), lds=8 * B * R)


def events(p, n, t_lo=None, t_hi=None):
    """(bins, counts) of neuron n, inside [t_lo, t_hi) when given"""
    s = np.flatnonzero(p.S[:, n])
    if t_lo is not None:
        s = s[(s >= t_lo) & (s < t_hi)]
    return s, p.S[s, n].astype(float)


def window(p, n, tb0, tb1, R):
    """events of neuron n a block [tb0, tb1) stages: first tile's wlo to last tile's whi (upload_windows, pglm_capi.hip)"""
    s, cnt = events(p, n)
    m = (s >= 16 * (tb0 >> 4) - R) & (s < 16 * ((tb1 - 1) >> 4) + 15)
    return s[m], cnt[m]


def max_events(c, cols, t_lo, t_hi):
    p = problem(c)
    return max(len(events(p, n, t_lo, t_hi)[0]) for n in cols)


def case_geometry(c, opt_gibbs=0):
    p = problem(c)
    t_lo, t_hi = case_range(c)
    return geometry(len(c['cols']), len(c['w']), c['pre'], t_hi - t_lo, max_events(c, c['cols'], t_lo, t_hi), p.kind,
                    opt_gibbs, c.get('nloop', 0), taps(p))


def window_counts(c, block):
    """largest number of presynaptic events a block of `block` bins from t_lo stages, over the columns and blocks"""
    p = problem(c)
    t_lo, t_hi = case_range(c)
    R = taps(p)
    return max(len(window(p, j, tb0, min(tb0 + block, t_hi), R)[0]) for j in c['pre'] for tb0 in range(t_lo, t_hi, block))


# ---- float64 mirror of the regime-split decomposition, with switchable defects ---------------------------------------------
def _ic_from(s, cnt, t, hs, R):
    """sum over the events (s, cnt) of cnt * hs[t - s - 1] for 0 <= t - s - 1 < R, in event order (float64)"""
    a = np.zeros(len(t))
    for sj, cj in zip(s, cnt):
        d = t - sj - 1
        m = (d >= 0) & (d < R)
        a[m] += cj * hs[d[m]]
    return a


def _softplus_tail64(x):
    return np.log1p(np.exp(-np.abs(x)))


def mirror(c, cols, pre, ws, t_lo, t_hi, nloop=0, defect=None):
    """ll (ncols, K) in float64 by the decomposition of k_gibbs_rate_cols + spike workgroups + k_gibbs_reduce_cols2: per
    256-bin sub-block the pair current from the events of its window, x0 = (bias + GX) - aw ic, per item (column, time
    split) the careful test |x0| + max|w| |ic| < 699, softplus = max(x, 0) [f64] + log1p(exp(-|x|)) [np.float32 e - e^2/2
    per lane where the float32 |x| >= 12, float64 elsewhere], partials per workgroup of nloop sub-blocks; the spike terms
    from the post-synaptic event list in chunks of 256; ll = -dt sum(part) + sum(partS).  `defect`: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    p = problem(c)
    R = taps(p)
    Reff = R - 1 if defect == 'drop_last_lag' else R
    thr = np.float32(8.0 if defect == 'f32_from_8' else 12.0)
    g = geometry(len(cols), ws.shape[1], pre, t_hi - t_lo, max_events(c, cols, t_lo, t_hi), p.kind, 0, nloop, R)
    GX = _xtot(_key(c))[1]
    phi = p.ibasis[:R]
    K = ws.shape[1]
    nseg = (GRB // 64) // g['nsplit']
    out = np.empty((len(cols), K))
    for i, (n, j) in enumerate(zip(cols, pre)):
        beta = p.theta[n, 1 + j * p.B:1 + (j + 1) * p.B]
        hs = phi.dot(beta)
        aw = 0.0 if defect == 'no_aw' else p.Weff[j, n]
        wmax = np.max(np.abs(ws[i]))
        part = np.zeros((g['nblk'], K))
        for sb in range(g['nsub']):
            tb0 = t_lo + sb * GRB
            tb1 = min(tb0 + GRB, t_hi)
            nb = tb1 - tb0
            if defect == 'drop_ragged' and nb < GRB:
                continue
            t = np.arange(tb0, tb1)
            s, cnt = window(p, j, tb0, tb1, R)
            if defect == 'drop_21st' and len(s) > GECAP_R and not g['same_pre']:
                s, cnt = np.delete(s, GECAP_R), np.delete(cnt, GECAP_R)
            ic = np.zeros(GRB)
            ic[:nb] = _ic_from(s, cnt, t, hs, Reff)
            x0 = np.full(GRB, -600.0)
            x0[:nb] = (p.theta[n, 0] + GX[t, n]) - aw * ic[:nb]
            for sp in range(g['nsplit']):
                sl = slice(sp * nseg * 64, (sp + 1) * nseg * 64)
                x0i, ici = x0[sl], ic[sl]
                careful = bool(np.any(~(wmax * np.abs(ici) + np.abs(x0i) < 699.0)))
                for k in range(K):
                    x = ws[i, k] * ici + x0i
                    acc = np.sum(np.maximum(x, 0.0))
                    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
                        if careful:
                            lam = np.maximum(x, 0.0) + _softplus_tail64(x)
                            tail = np.where(x >= 700.0, 0.0, np.where(lam == 0.0, np.nan, lam - np.maximum(x, 0.0)))
                            acc += np.sum(tail)
                        else:
                            af = np.abs(x).astype(np.float32)
                            fast = af >= thr
                            e = np.where(fast, np.exp2(af * np.float32(-1.44269504088896340736)), np.float32(0)).astype(np.float32)
                            e = np.where(e < np.float32(2.0 ** -126), np.float32(0), e).reshape(nseg, 64)
                            a1 = np.zeros(64, dtype=np.float32)
                            a2 = np.zeros(64, dtype=np.float32)
                            for sg in range(nseg):
                                a1 = a1 + e[sg]
                                a2 = (e[sg].astype(np.float64) ** 2 + a2.astype(np.float64)).astype(np.float32)
                            lane = (a1.astype(np.float64) - 0.5 * a2.astype(np.float64)).astype(np.float32)
                            acc += np.sum(_softplus_tail64(x[~fast])) + np.sum(lane.astype(np.float64))
                    part[sb // g['nloop'], k] += acc
        # spike terms: the events of n_post inside the range, 256 per workgroup
        s, cnt = events(p, n, t_lo, t_hi)
        if defect == 'spikes_from_256':
            s, cnt = s[:256], cnt[:256]
        partS = np.zeros((max(1, -(-len(s) // 256)), K))
        if len(s):
            sj, cj = events(p, j)
            ic = _ic_from(sj, cj, s, hs, Reff)
            x0 = (p.theta[n, 0] + GX[s, n]) - aw * ic
            for k in range(K):
                x = ws[i, k] * ic + x0
                a = np.abs(x)
                with np.errstate(all='ignore'):
                    e = np.exp(-a)
                    lam = np.maximum(x, 0.0) + np.where(a < 12.0, np.log1p(e), e * (1.0 - e * (0.5 - e / 3.0)))
                    term = cnt * np.log(lam)
                partS[:, k] = np.add.reduceat(term, np.arange(0, len(s), 256))
        out[i] = -p.dt * np.sum(part, axis=0) + np.sum(partS, axis=0)
    if defect == 'swap_1_8' and K > 8:
        out[:, [1, 8]] = out[:, [8, 1]]
    return out


def mirror_f64(c, cols, pre, ws, t_lo, t_hi):
    """ll (ncols, K) in float64 by the decomposition of k_gibbs_ll_cols + k_gibbs_reduce_cols: one term per bin,
    v = -dt lam (NaN where lam == 0) + S log lam, summed per block of `rows` bins, then over the blocks"""
    p = problem(c)
    g = geometry(len(cols), ws.shape[1], pre, t_hi - t_lo, 0, p.kind, 1, 0, taps(p))
    x = currents(c, cols, pre, ws, t_lo, t_hi).astype(np.float64)
    with np.errstate(all='ignore'):
        lam = np.exp(x) if p.kind == 'exp' else np.maximum(x, 0.0) + _softplus_tail64(x)
        loglam = x if p.kind == 'exp' else np.log(lam)
        S = p.S[t_lo:t_hi][:, list(cols)].T[:, :, None].astype(float)
        v = np.where(lam == 0.0, np.nan, -p.dt * lam) + np.where(S > 0, S * loglam, 0.0)
    blocks = np.add.reduceat(v, np.arange(0, t_hi - t_lo, g['rows']), axis=1)
    return np.sum(blocks, axis=1)
