"""Case tables, numpy.longdouble references, derived bounds and numpy mirrors of the blocking of the stimulus-preparation
kernels (theano_pyglm_amd/csrc/pglm_stim.hip.h).  Test infrastructure, numpy only, no GPU: tests/test_stim_cases.py keeps
the tables honest on the CPU, tests/test_gpu_stim_sweep.py runs them on the device.

GEMM (pgl_gemm_dev: k_gemm_nt, k_gemm_mfma<1>, <4>, k_gemm_kc<4,1,8>, <1,0,16>)
  reference  C = A B^T accumulated in longdouble.
  bound      |C - Cref|_ij <= (K + 8) 2^-53 (|A||B|)_ij: any summation order of K products, with or without FMAs, costs at most
             (K - 1 + 1) u per term to first order; + 8 covers the seven additions of the eight waves' partial tiles and the
             second-order terms (K <= 1088).  The form tests/test_gpu_bfgs_rows.py uses.
  inputs     mixed signs; the entries of A's k-chunk j (eight consecutive k: the finest unit any of the kernels hands out)
             have their own scale 10^(-3 + 6 frac_j), frac_j spread over [0, 1] in a seeded order, B is of order one.  A row
             of A is zero (its row of C must be exactly 0).  Gaps of padded operands hold NaN.

Features (pgl_set_stimulus -> pgl_get_stim_features: k_stim_project, k_stim_conv)
  reference  np.interp's rule on knots dt_stim f and positions dt t, both formed in longdouble from the double dt_stim and dt,
             the projection and the strictly causal convolution in longdouble.
  bound      u = 2^-53.  A value v interpolated between the frames f0, f1 of knot i0 carries (a) the rounding of the slope
             form, <= 4 u (|f0| + |f1|), and (b) the rounding of the position: x = fl(dt t), x0 = fl(dt_stim i0), x1 likewise
             are each off by u (i0 + 1) dt_stim at most, the difference x1 - x0 by twice that, so the weight (x - x0) / (x1 - x0)
             is off by 4 u (i0 + 2) and v by 4 u (i0 + 2) |f1 - f0| (the largest |f1 - f0| of the knot's interval and its two
             neighbours: at a knot the device may take the other interval).  The D FMAs of the projection and the Rt FMAs of
             the convolution add (D + Rt) u of the absolute sum.  Together
                 |F - Fref| <= u [ (Rt + D + 6) conv(|bt|, |bx|^T (|f0| + |f1|)) + 4 conv(|bt|, |bx|^T (i0 + 2) max|f1 - f0|) ].

STA (pgl_sta: k_sta, k_sta_finish; k_sta_weights + k_gemm_kc<1,0,16>; option 94 = 7 forces the former)
  reference  the dense lag form of oracle.sta in longdouble.
  bound      the same two terms per event (t, c) and lag l, through the sum over the neuron's E events and, in the frame-rate
             form, the Tstim <= 25 terms of the GEMM:  (dt / dt_stim) / count times
                 u [ (E + 48) sum c (|f0| + |f1|) + 4 sum c (i0 + 2) max|f1 - f0| ],   48 >= 25 + 8 (GEMM) + 4 (slope) + scale, division.

Singular pairs (pgl_leading_singular_pairs)
  matrices   U diag(s) V^T from seeded orthogonal factors: s is known, s2 / s1 <= 0.98.
  reference  LAPACK's leading pair refined by the alternating iteration in longdouble until stationary.
  bound      not derivable to a constant: e0 = the error of np.linalg.svd against the refined pair (computed where the test
             runs), the device may take 8 e0, with the floors 16 big u / (1 - s2 / s1) (vectors) and 16 big u (sigma, relative).
"""
import functools

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
NAN = float('nan')
SENTINEL = -7.25e77                    # what C holds before a GEMM; everything outside the result keeps it

# ----------------------------------------------------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------------------------------------------------
KERNELS = ('nt', 'mfma1', 'mfma4', 'kc418', 'kc1016')            # index = PGL_GEMM_*
NT_OF = {'mfma1': 1, 'mfma4': 4, 'kc418': 4, 'kc1016': 1}
NB_OF = {'kc418': 8, 'kc1016': 16}
NWG = 8
M_TAILS = (1, 15, 16, 17, 33)
K_MFMA = (1, 7, 8, 31, 32, 33, 224, 256, 257, 545)
K_MFMA4 = (1, 8, 33, 257, 545)
K_KC = (2, 6, 8, 10, 12, 62, 64, 66, 72, 576, 1088)              # (12: the one K with K % 8 = 4)
FAULTS = ('ktail', 'drop_wave', 'double_chunk', 'clamp_write')


def _gemm_cases():
    out = []

    def add(kernel, M, N, K, pat='rm', batch=1, pad=0):
        out.append(dict(name='%s-M%d-N%d-K%d-%s-b%d%s' % (kernel, M, N, K, pat, batch, '-pad%d' % pad if pad else ''),
                        kernel=kernel, M=M, N=N, K=K, pat=pat, batch=batch, pad=pad, seed=len(out)))
    for M in M_TAILS:
        for N in (1, 15, 16, 17):
            for K in K_MFMA:
                add('mfma1', M, N, K)
        for N in (1, 48, 63, 64, 65, 80):
            for K in K_MFMA4:
                add('mfma4', M, N, K)
    for kernel in ('mfma1', 'mfma4'):
        N = 17 if kernel == 'mfma1' else 65
        for batch in (1, 3):
            for K in (33, 257):
                add(kernel, 17, N, K, 'tr', batch, pad=3)              # A[m + k lda]: the Gram matrix of a tall batch
                add(kernel, 33, 1, K, 'bvec', batch, pad=3)            # sbn = 0, N = 1, C[m]: y = A x
                add(kernel, 33, 1, K, 'trbvec', batch, pad=3)          # the same on A^T
                add(kernel, 17, N, K, 'rm', batch, pad=3)              # row-major, padded, C[m ldc + n]
                add(kernel, 17, N, K, 'ct', batch, pad=3)              # C transposed: C[m + n ldc] (the frame-rate projection)
    for kernel, Ns in (('kc418', (1, 15, 16, 17, 63, 64, 65)), ('kc1016', (1, 15, 16, 17))):
        for M in M_TAILS:
            for N in Ns:
                for K in K_KC:
                    if K in (576, 1088) and (M not in (1, 17) or N not in (1, 17, 65)):
                        continue                                        # (the long K at the tail tiles only)
                    add(kernel, M, N, K, 'rm', 1, pad=0 if (M + N + K // 2) % 2 else 4)
    for M in (1, 63, 64, 65):
        for N in (1, 63, 64, 65):
            for K in (1, 31, 32, 33, 65):
                add('nt', M, N, K, 'rm', 1, pad=3)
    return out


GEMM_CASES = _gemm_cases()


def gemm_facts(c):
    """What the kernel's own index arithmetic makes of the case's K."""
    K, k = c['K'], c['kernel']
    if k.startswith('mfma'):
        nU = (K + 31) // 32
        return dict(nU=nU, rounds=(nU + NWG - 1) // NWG, idle=max(0, NWG - nU), prefetch=nU > NWG, ktail=K % 32 != 0)
    if k.startswith('kc'):
        nC = (K + 7) // 8
        cpw = (nC + NWG - 1) // NWG
        share = [max(0, min(nC, (w + 1) * cpw) - w * cpw) for w in range(NWG)]
        NB = NB_OF[k]
        return dict(nC=nC, cpw=cpw, idle=sum(s == 0 for s in share), short=any(0 < s < cpw for s in share),
                    batches=(cpw + NB - 1) // NB, partial_batch=cpw % NB != 0, ktail=K % 8)
    return dict(steps=(K + 31) // 32, ktail=K % 32 != 0)


def _chunk_scales(K, rng):
    nch = (K + 7) // 8
    frac = (rng.permutation(nch) + 0.5) / nch
    return np.repeat(10.0 ** (-3.0 + 6.0 * frac), 8)[:K]


def _place(vals, off, s0, s1, sb, size):
    """a flat NaN buffer of `size` doubles with vals[b, i, j] at off + b sb + i s0 + j s1"""
    buf = np.full(size, NAN)
    nb, n0, n1 = vals.shape
    idx = off + sb * np.arange(nb)[:, None, None] + s0 * np.arange(n0)[None, :, None] + s1 * np.arange(n1)[None, None, :]
    buf[idx.ravel()] = vals.ravel()
    return buf


@functools.lru_cache(maxsize=None)
def _gemm_case(name):
    c = [c for c in GEMM_CASES if c['name'] == name][0]
    rng = np.random.default_rng(1000 + c['seed'])
    M, N, K, nb, pad, pat, k = c['M'], c['N'], c['K'], c['batch'], c['pad'], c['pat'], c['kernel']
    A = rng.uniform(0.5, 2.0, (nb, M, K)) * rng.choice([-1.0, 1.0], (nb, M, K)) * _chunk_scales(K, rng)
    B = rng.uniform(0.5, 2.0, (nb, N, K)) * rng.choice([-1.0, 1.0], (nb, N, K))
    zrow = M // 2 if M >= 3 else None
    if zrow is not None:
        A[:, zrow, :] = 0.0
    d = dict(c, A=A, B=B, zrow=zrow)
    # operand layouts (strides in doubles); offsets keep the 16-byte alignment the kc kernels need
    if pat in ('tr', 'trbvec'):                                     # A[m + k lda]
        lda = M + pad
        d['sa'], a_sz = (1, lda, lda * K + 5), None
    else:
        lda = K + pad
        d['sa'] = (lda, 1, lda * M + 6)
    d['a_off'] = 2
    d['Abuf'] = _place(A, 2, d['sa'][0], d['sa'][1], d['sa'][2], 2 + d['sa'][2] * nb + 4)
    if k == 'kc1016':                                               # B[k ldb + n]
        ldb = N + pad
        d['sb'] = (1, ldb, ldb * K + 6)
    elif pat in ('bvec', 'trbvec'):                                 # one vector per batch element, sbn = 0
        d['sb'] = (0, 1, K + pad)
    else:
        ldb = K + pad
        d['sb'] = (ldb, 1, ldb * N + 6)
    d['b_off'] = 2
    d['Bbuf'] = _place(B, 2, d['sb'][0], d['sb'][1], d['sb'][2], 2 + d['sb'][2] * nb + 4)
    if pat in ('bvec', 'trbvec'):                                   # C[m], scn = 0
        d['sc'] = (1, 0, M + pad)
    elif pat == 'ct':
        ldc = M + pad
        d['sc'] = (1, ldc, ldc * N + 5)
    else:
        ldc = N + pad
        d['sc'] = (ldc, 1, ldc * M + 5)
    d['c_off'] = 3
    d['c_size'] = 3 + d['sc'][2] * nb + 4
    idx = 3 + d['sc'][2] * np.arange(nb)[:, None, None] + d['sc'][0] * np.arange(M)[None, :, None] + \
        d['sc'][1] * np.arange(N)[None, None, :]
    d['c_idx'] = idx
    assert len(np.unique(idx)) == idx.size and idx.max() < d['c_size']
    Al, Bl = A.astype(LD), B.astype(LD)
    d['ref'] = np.einsum('bmk,bnk->bmn', Al, Bl)
    d['mag'] = np.einsum('bmk,bnk->bmn', np.abs(A), np.abs(B))
    d['bound'] = (K + 8) * U53 * d['mag']
    return d


def gemm_case(c):
    """The case with its operands: A (batch, M, K), B (batch, N, K); the flat device images Abuf, Bbuf (NaN in every gap)
    with the offsets a_off, b_off and strides sa = (sam, sak, sAb), sb = (sbn, sbk, sBb); the result's layout c_off, sc,
    c_size and index array c_idx (batch, M, N); ref (longdouble), mag = |A||B| and bound.  Cached: treat as read-only."""
    return _gemm_case(c['name'])


def gemm_ratio(d, C):
    """worst |C - ref| / bound over the entries (C as (batch, M, N)); a zero operand row must be exactly zero"""
    err = np.abs(C.astype(LD) - d['ref']).astype(float)
    if d['zrow'] is not None:
        assert np.all(C[:, d['zrow'], :] == 0.0), "the zero row of A gave a non-zero (or NaN) row of C"
    live = d['bound'] > 0
    if np.any(~np.isfinite(C)) or np.any(err[~live] != 0.0):
        return float('inf')
    return float(np.max(err[live] / d['bound'][live])) if live.any() else 0.0


def gemm_mirror(d, fault=None):
    """numpy (float64) mirror of the kernel's blocking on the flat images: tiles with clamped row pointers, K handed to the
    eight waves in the kernel's chunks with the tail masked, partial tiles added in wave order, guarded stores into a buffer
    pre-filled with SENTINEL.  Returns the flat C buffer.  fault: 'ktail' (the tail of K not masked: whatever lies at the
    address is multiplied in), 'drop_wave' (the last working wave's share is lost), 'double_chunk' (the first chunk counted
    twice), 'clamp_write' (rows of a tail tile loaded unclamped and stored at the clamped index)."""
    k, M, N, K, nb = d['kernel'], d['M'], d['N'], d['K'], d['batch']
    Ab, Bb = d['Abuf'], d['Bbuf']
    sam, sak, sAb = d['sa']
    sbn, sbk, sBb = d['sb']
    scm, scn, sCb = d['sc']
    TM, TN = (64, 64) if k == 'nt' else (16, 16 * NT_OF[k])
    if k == 'nt':
        shares = [[(k0, k0 + 32) for k0 in range(0, K, 32)]]
    elif k.startswith('mfma'):
        nU = (K + 31) // 32
        shares = [[(32 * u, 32 * u + 32) for u in range(w, nU, NWG)] for w in range(NWG)]
    else:
        nC = (K + 7) // 8
        cpw = (nC + NWG - 1) // NWG
        shares = [[(8 * ch, 8 * ch + 8) for ch in range(w * cpw, min(nC, (w + 1) * cpw))] for w in range(NWG)]
    if fault == 'drop_wave':
        w = max(i for i, s in enumerate(shares) if s)
        shares[w] = []
    if fault == 'double_chunk':
        shares[0] = [shares[0][0]] + shares[0]
    Cb = np.full(d['c_size'], SENTINEL)

    def rd(buf, idx):
        return buf[np.minimum(idx, buf.size - 1)]
    for b in range(nb):
        for m0 in range(0, M, TM):
            for n0 in range(0, N, TN):
                rows, cols = np.arange(m0, m0 + TM), np.arange(n0, n0 + TN)
                lrow = rows if (fault == 'clamp_write' and m0 + TM > M) else np.minimum(rows, M - 1)
                lcol = np.minimum(cols, N - 1)
                acc = None
                for sh in shares:
                    part = np.zeros((TM, TN))
                    for k_lo, k_hi in sh:
                        ks = np.arange(k_lo, k_hi)
                        if fault != 'ktail':
                            ks = ks[ks < K]
                        a = rd(Ab, d['a_off'] + b * sAb + lrow[:, None] * sam + ks[None, :] * sak)
                        bb = rd(Bb, d['b_off'] + b * sBb + lcol[:, None] * sbn + ks[None, :] * sbk)
                        part = part + a.dot(bb.T)
                    acc = part if acc is None else acc + part
                for i, m in enumerate(rows):
                    if fault == 'clamp_write':
                        m = min(m, M - 1)
                    if m >= M:
                        continue
                    nn = cols[cols < N]
                    Cb[d['c_off'] + b * sCb + m * scm + nn * scn] = acc[i, :nn.size]
    return Cb


def gemm_result(d, Cb):
    """(C (batch, M, N), untouched) from a flat result buffer: untouched = everything outside the result still SENTINEL"""
    mask = np.ones(Cb.size, bool)
    mask[d['c_idx'].ravel()] = False
    return Cb[d['c_idx']], bool(np.all(Cb[mask] == SENTINEL))


# ----------------------------------------------------------------------------------------------------------------------
# interpolation shared by the features and the STA
# ----------------------------------------------------------------------------------------------------------------------
def interp_knots(nT, Tstim, dt, dt_stim):
    """np.interp's bracketing on longdouble positions: (i0, w, beyond) per bin; value = f[i0] + (f[i0 + 1] - f[i0]) w,
    or f[Tstim - 1] where beyond."""
    x = LD(dt) * np.arange(nT, dtype=LD)
    if Tstim < 2:
        return np.zeros(nT, int), np.zeros(nT, LD), np.ones(nT, bool)
    xp = LD(dt_stim) * np.arange(Tstim, dtype=LD)
    beyond = x >= xp[-1]
    i0 = np.clip(np.searchsorted(xp, x, side='right') - 1, 0, Tstim - 2)
    w = (x - xp[i0]) / (xp[i0 + 1] - xp[i0])
    return i0, np.where(beyond, LD(0), w), beyond


def interp_ref(stim, nT, dt, dt_stim):
    """(value (nT, D) longdouble, absolute term |f0| + |f1|, position term (i0 + 2) max |f1 - f0| over the knot's interval
    and its neighbours) -- the two error carriers of the bound"""
    Tstim = stim.shape[0]
    s = stim.astype(LD)
    i0, w, beyond = interp_knots(nT, Tstim, dt, dt_stim)
    if Tstim < 2:
        v = np.repeat(s[:1], nT, axis=0)
        return v, 2.0 * np.abs(v).astype(float), np.zeros(v.shape)
    f0, f1 = s[i0], s[i0 + 1]
    v = np.where(beyond[:, None], s[-1][None, :], f0 + (f1 - f0) * w[:, None])
    df = np.abs(np.diff(stim, axis=0))                               # (Tstim - 1, D)
    dmax = np.maximum(df, np.maximum(np.vstack((df[:1], df[:-1])), np.vstack((df[1:], df[-1:]))))
    a = np.where(beyond[:, None], 2.0 * np.abs(stim[-1])[None, :], np.abs(stim[i0]) + np.abs(stim[i0 + 1]))
    p = (i0[:, None] + 2.0) * dmax[i0]                               # (a bin at the last knot may come from the interval before it)
    return v, a, p


def _causal(z, bt):
    """out[t, x, b] = sum_{tau = 1 .. Rt} z[t - tau, x] bt[tau - 1, b]"""
    nT, Rt = z.shape[0], bt.shape[0]
    pad = np.vstack((np.zeros((Rt, z.shape[1]), z.dtype), z))
    out = np.zeros((nT, z.shape[1], bt.shape[1]), z.dtype)
    for tau in range(1, Rt + 1):
        out += pad[Rt - tau:Rt - tau + nT, :, None] * bt[tau - 1][None, None, :]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# features
# ----------------------------------------------------------------------------------------------------------------------
DT = 0.001


def _feature_cases():
    out = []

    def add(tag, nT, Rt, Bt, Bx, D, ident, layout, Tstim, dt_stim, offset=0):
        out.append(dict(name='%s-nT%d-Rt%d-Bt%d-Bx%d-%s-l%d-Ts%d' % (tag, nT, Rt, Bt, Bx, 'id' if ident else 'D%d' % D, layout, Tstim),
                        nT=nT, Rt=Rt, Bt=Bt, Bx=Bx, D=D, ident=ident, layout=layout, Tstim=Tstim, dt_stim=dt_stim,
                        seed=len(out), offset=offset))
    for nT in (1, 255, 256, 257, 513):                               # block tails of k_stim_conv; Rt = 300 > nT for the first four
        add('nT', nT, 300, 3, 3, 5, False, 0, nT // 7 + 2, 0.007)
    for Rt in (1, 2, 255, 256, 257, 300):                            # the LDS window Rt + 256 against the 256 threads
        add('Rt', 513, Rt, 3, 3, 3, True, Rt % 2, 513 // 7 + 2, 0.007)
    for Bt in (1, 3, 4):
        for Bx in (1, 3):
            for ident in (True, False):
                for layout in (0, 1):
                    add('B', 257, 17, Bt, Bx, Bx if ident else 4, ident, layout, 40, 0.007)
    add('Tstim1', 257, 33, 3, 3, 5, False, 0, 1, 0.1)                # clamped everywhere
    add('Tstim2', 257, 33, 3, 3, 5, False, 1, 2, 0.1)                # one interval, then the hold
    add('short', 513, 33, 3, 3, 3, True, 0, 20, 0.007)               # the stimulus ends at bin 133: the last frame is held
    add('q1', 257, 33, 3, 3, 3, True, 0, 300, 0.001)                 # every bin on a knot
    add('q100', 513, 33, 3, 3, 5, False, 0, 7, 0.1)
    add('q3.3', 513, 33, 3, 3, 5, False, 1, 170, 0.0033)             # dt_stim / dt no integer
    return out


FEATURE_CASES = _feature_cases()


@functools.lru_cache(maxsize=None)
def _feature_case(name):
    c = [c for c in FEATURE_CASES if c['name'] == name][0]
    rng = np.random.default_rng(2000 + c['seed'])
    stim = rng.standard_normal((c['Tstim'], c['D'])) * 10.0 ** rng.uniform(-2, 2, (c['Tstim'], 1))
    bt = rng.standard_normal((c['Rt'], c['Bt'])) * 10.0 ** rng.uniform(-1, 1, (c['Rt'], 1))
    bx = None if c['ident'] else rng.standard_normal((c['D'], c['Bx']))
    v, a, p = interp_ref(stim, c['nT'], DT, c['dt_stim'])
    bxl = np.eye(c['D']) if bx is None else bx
    f = _causal(v.dot(bxl.astype(LD)), bt.astype(LD))                # (nT, Bx, Bt)
    fa = _causal(a.dot(np.abs(bxl)), np.abs(bt))
    fp = _causal(p.dot(np.abs(bxl)), np.abs(bt))
    D_eff = 1 if bx is None else c['D']
    bound = U53 * ((c['Rt'] + D_eff + 6) * fa + 4.0 * fp)

    def lay(z):                                                      # layout 0: column bt Bx + bx; layout 1: bx Bt + bt
        return (np.transpose(z, (0, 2, 1)) if c['layout'] == 0 else z).reshape(c['nT'], -1)
    return dict(c, stim=stim, basis_t=bt, basis_x=bx, ref=lay(f), bound=lay(bound))


def feature_case(c):
    return _feature_case(c['name'])


def feature_ratio(d, F):
    err = np.abs(F.astype(LD) - d['ref']).astype(float)
    live = d['bound'] > 0
    if np.any(~np.isfinite(F)) or np.any(err[~live] != 0.0):
        return float('inf')
    return float(np.max(err[live] / d['bound'][live])) if live.any() else 0.0


def feature_numpy(d, shift=0):
    """float64 numpy: np.interp, the projection, np.convolve.  shift = 1: the convolution window one bin late (tau from 0)."""
    nT = d['nT']
    t, ts = DT * np.arange(nT), d['dt_stim'] * np.arange(d['Tstim'])
    s = np.stack([np.interp(t, ts, d['stim'][:, j]) for j in range(d['D'])], axis=1)
    z = s if d['basis_x'] is None else s.dot(d['basis_x'])
    out = np.zeros((nT, d['Bx'], d['Bt']))
    for b in range(d['Bt']):
        kern = np.concatenate(([0.0] * (1 - shift), d['basis_t'][:, b]))
        for x in range(d['Bx']):
            out[:, x, b] = np.convolve(z[:, x], kern)[:nT]
    return (np.transpose(out, (0, 2, 1)) if d['layout'] == 0 else out).reshape(nT, -1)


# ----------------------------------------------------------------------------------------------------------------------
# STA
# ----------------------------------------------------------------------------------------------------------------------
STA_EVENTS = (0, 1, 255, 256, 257, 700)                            # events (bins that hold spikes) of neurons 0 .. 5
STA_SEL = (5, 2, 2, 0, 3, 1, 4)                                    # unordered, one repeat


def _sta_cases():
    out = []

    def add(L, D, Tstim, q, sel=STA_SEL):
        nT = min(3000, max(1000, Tstim * q + 400))
        out.append(dict(name='LD%dx%d-Ts%d-q%d-sel%d' % (L, D, Tstim, q, len(sel)), L=L, D=D, Tstim=Tstim, q=q, nT=nT,
                        sel=tuple(sel), seed=len(out)))
    for (L, D), Tstim, q in (((1, 1), 2, 1), ((85, 3), 3, 7), ((64, 4), 24, 100), ((257, 1), 25, 100), ((120, 5), 24, 7),
                             ((256, 1), 2, 100), ((17, 15), 25, 1), ((30, 20), 3, 100), ((51, 5), 24, 1), ((5, 51), 2, 7)):
        add(L, D, Tstim, q)
    add(16, 3, 24, 7, sel=(1,))                                      # one neuron, one event, 64 chunks: 63 of them empty
    add(16, 3, 25, 7, sel=(3,))                                      # 256 events over 64 chunks: four each
    add(100, 6, 24, 7, sel=(4, 0, 5))                                # xb nSel = 9: echunks = 64 against 257 events, per = 5: chunks 52 .. 63 empty
    return out


STA_CASES = _sta_cases()


def sta_facts(c):
    """the launch arithmetic of pgl_sta for the case"""
    LDn, nSel = c['L'] * c['D'], len(c['sel'])
    xb = (LDn + 255) // 256
    echunks = int(min(64, max(1, 4096 // (xb * nSel))))
    ev = [STA_EVENTS[n] for n in c['sel']]
    per = [-(-e // echunks) for e in ev]
    empty = [sum(1 for ch in range(echunks) if ch * p >= e) for e, p in zip(ev, per)]
    frame = c['Tstim'] % 2 == 0 and c['Tstim'] >= 2                  # (q is an integer in every case)
    return dict(xb=xb, echunks=echunks, per=per, empty=empty, frame_rate=frame)


@functools.lru_cache(maxsize=None)
def _sta_case(name):
    c = [c for c in STA_CASES if c['name'] == name][0]
    rng = np.random.default_rng(3000 + c['seed'])
    nT, L, D, Tstim, q = c['nT'], c['L'], c['D'], c['Tstim'], c['q']
    dt_stim = DT * q
    S = np.zeros((nT, len(STA_EVENTS)), np.uint8)
    last_frame_bin = (Tstim - 1) * q
    for n, E in enumerate(STA_EVENTS):
        if E == 0:
            continue
        must = [nT - 1] if E == 1 else [0, min(L, nT) - 1, nT - 1, min(nT - 2, last_frame_bin + 1)]
        bins = set(must[:E])
        rest = [t for t in rng.permutation(nT) if t not in bins]
        bins |= set(rest[:E - len(bins)])
        bins = np.array(sorted(bins))
        S[bins, n] = 1 + (rng.random(E) < 0.3) * rng.integers(1, 4, E)      # counts above 1
    stim = rng.standard_normal((Tstim, D)) * 10.0 ** rng.uniform(-2, 2, (Tstim, 1))
    v, a, p = interp_ref(stim, nT, DT, dt_stim)
    scale = LD(DT) / LD(dt_stim)
    nSel = len(c['sel'])
    ref = np.zeros((nSel, L, D), LD)
    bound = np.zeros((nSel, L, D))
    for i, n in enumerate(c['sel']):
        cnt = S[:, n].astype(float)
        tot, E = cnt.sum(), int(np.count_nonzero(cnt))
        if tot == 0:
            ref[i], bound[i] = np.nan, np.nan
            continue
        for l in range(L):
            w = cnt[l:]                                               # events at t >= l see bin t - l
            ref[i, l] = (w.astype(LD)[:, None] * v[:nT - l]).sum(0) * scale / LD(tot)
            bound[i, l] = U53 * ((E + 48) * w.dot(a[:nT - l]) + 4.0 * w.dot(p[:nT - l])) * float(scale) / tot
    return dict(c, S=S, stim=stim, dt_stim=dt_stim, ref=ref, bound=bound)


def sta_case(c):
    return _sta_case(c['name'])


def sta_ratio(d, A):
    """worst ratio over the rows of neurons that spike; a silent neuron's row must be NaN throughout"""
    worst = 0.0
    for i, n in enumerate(d['sel']):
        if STA_EVENTS[n] == 0:
            assert np.all(np.isnan(A[i])), "a silent neuron's row must be NaN"
            continue
        err = np.abs(A[i].astype(LD) - d['ref'][i]).astype(float)
        live = d['bound'][i] > 0
        if np.any(~np.isfinite(A[i])) or np.any(err[~live] != 0.0):
            return float('inf')
        if live.any():
            worst = max(worst, float(np.max(err[live] / d['bound'][i][live])))
    return worst


def sta_numpy(d, fault=None):
    """float64 mirror of the event form (k_sta on np.interp's stimulus).  fault: 'neg_tt' (an event at t < l reads bin
    t - l + nT, the wrap of a missing tt >= 0 test), 'no_hold' (bins behind the last frame read zero instead of it)."""
    nT, L, D = d['nT'], d['L'], d['D']
    t, ts = DT * np.arange(nT), d['dt_stim'] * np.arange(d['Tstim'])
    ist = np.stack([np.interp(t, ts, d['stim'][:, j]) for j in range(D)], axis=1)
    if fault == 'no_hold':
        ist[t > ts[-1]] = 0.0
    out = np.zeros((len(d['sel']), L, D))
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, n in enumerate(d['sel']):
            ev = np.nonzero(d['S'][:, n])[0]
            cnt = d['S'][ev, n].astype(float)
            for l in range(L):
                tt = ev - l
                ok = tt >= 0
                if fault == 'neg_tt':
                    tt, ok = np.where(ok, tt, tt + nT), np.ones(len(tt), bool)
                out[i, l] = cnt[ok].dot(ist[tt[ok]]) if ok.any() else 0.0
            out[i] = out[i] * (DT / d['dt_stim']) / cnt.sum()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# leading singular pairs
# ----------------------------------------------------------------------------------------------------------------------
LSP_SMALL = (1, 2, 15, 16, 17, 63, 64, 65)
LSP_LARGE = (1, 31, 33, 257, 300)
LSP_RATIOS = (0.1, 0.9, 0.98)


def _lsp_cases():
    out = []
    i = 0
    for small in LSP_SMALL:
        for large in LSP_LARGE:
            if small > large:
                continue
            for wide in ((True, False) if small != large else (True,)):
                L, D = (small, large) if wide else (large, small)
                rank1 = i % 5 == 4
                out.append(dict(name='L%d-D%d-%s' % (L, D, 'rank1' if rank1 else 'r%g' % LSP_RATIOS[i % 3]), L=L, D=D,
                                ratio=0.0 if rank1 else LSP_RATIOS[i % 3], n=5 if i % 4 == 1 else 1, seed=i))
                i += 1
    return out


LSP_CASES = _lsp_cases()


def lsp_matrices(c):
    """(A (n, L, D), s1 (n,)): U diag(s) V^T, s = s1 (1, ratio, ratio / 2, ratio / 3, ...); the matrices of a batch differ in
    their factors and by a scale 10^(b - 2)"""
    rng = np.random.default_rng(4000 + c['seed'])
    L, D, m = c['L'], c['D'], min(c['L'], c['D'])
    A, s1 = np.zeros((c['n'], L, D)), np.zeros(c['n'])
    for b in range(c['n']):
        U = np.linalg.qr(rng.standard_normal((L, m)))[0]
        V = np.linalg.qr(rng.standard_normal((D, m)))[0]
        s = np.concatenate(([1.0], c['ratio'] / np.arange(1, m))) * 10.0 ** (b - 2)
        A[b], s1[b] = (U * s).dot(V.T), s[0]
    return A, s1


def lsp_sign(u, v):
    """the library's sign convention: the component of u of largest magnitude is positive"""
    j = int(np.argmax(np.abs(u)))
    return (-u, -v) if u[j] < 0 else (u, v)


def lsp_refine(A):
    """LAPACK's leading pair of A (L, D), refined by the alternating iteration in longdouble until stationary:
    (u, sigma, v) longdouble, signed like the library's"""
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    Al = A.astype(LD)
    u, v = U[:, 0].astype(LD), Vt[0].astype(LD)
    for _ in range(20000):
        v1 = Al.T.dot(u)
        v1 /= np.sqrt(v1.dot(v1))
        u1 = Al.dot(v1)
        sig = np.sqrt(u1.dot(u1))
        u1 /= sig
        step = max(np.max(np.abs(u1 - u)), np.max(np.abs(v1 - v)))
        u, v = u1, v1
        if step < 4 * np.finfo(LD).eps:
            break
    else:
        raise AssertionError("the refinement did not become stationary")
    u, v = lsp_sign(u, v)
    return u, sig, v


def lsp_errors(u, sig, v, ref):
    """(vector error: max |.| over u and v, relative sigma error) against a refined pair"""
    ur, sr, vr = ref
    u, v = lsp_sign(np.asarray(u), np.asarray(v))
    ev = max(float(np.max(np.abs(u.astype(LD) - ur))), float(np.max(np.abs(v.astype(LD) - vr))))
    return ev, float(abs(LD(sig) - sr) / sr)


def lsp_bounds(c, A):
    """(vector bound, sigma bound) of a matrix: 8 e0 with e0 the error of np.linalg.svd itself against the refined pair, and
    the floors of the module docstring"""
    ref = lsp_refine(A)
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    e0v, e0s = lsp_errors(U[:, 0], s[0], Vt[0], ref)
    big = max(c['L'], c['D'])
    return ref, max(8 * e0v, 16 * big * U53 / (1.0 - c['ratio'])), max(8 * e0s, 16 * big * U53)
