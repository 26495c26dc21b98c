"""The set of fused kernel instantiations the dispatcher can reach, from a dry run of make_plan (csrc/pglm_plan.h) and the
launchers (csrc/pglm_launch.h) over a grid of shapes (pgl_plan_kernels: no GPU needed), against the instantiations in the
built library:

    python tools/reachable_kernels.py            # summary + instantiations no plan reaches + reachable ones with scratch
    python tools/reachable_kernels.py --emit-cases   # rewrite tests/dispatch_cases.json (one cheap case per instantiation)
    python tools/reachable_kernels.py --emit-hvp-cases   # rewrite tests/hvp_cases.json (the Hessian-vector paths)

`reachable(auto_only)` is what tests/test_capi_symbols.py uses: every instantiation reachable WITHOUT a forcing option
must exist in the library and use no scratch.  tests/test_dispatch_cases.py holds the committed case table to the same
set, tests/test_gpu_dispatch_sweep.py runs every case against the oracle.

The Hessian-vector products have a table of their own (paths 3 / 4 of pgl_plan_kernels: pgl_hvp_prepare_* and
pgl_hvp_apply_dev): tests/hvp_cases.json, one case per reachable (prepare sequence, apply sequence) plus, for every column
pair of k_hvp5, one case per form of call (HVP_FORMS).  tests/test_hvp_cases.py holds it complete,
tests/test_gpu_hvp_sweep.py runs it against a float64 reference."""
import functools, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib

CASES = os.path.join(ROOT, 'tests', 'dispatch_cases.json')
FIELDS = ('N', 'B', 'R', 'Dstim', 'nT', 'stim', 'n_lo', 'count', 'path', 'opt_kernel', 'opt_f32')

FUSED = ('k_fused2<', 'k_fused3<', 'k_fused5<', 'k_fused6<', 'k_fused7<', 'k_fused8<', 'k_fused<')


def shapes():
    Ns = list(range(1, 137)) + list(range(144, 521, 8))
    for N in Ns:
        counts = sorted(set(c for c in (N, 1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 100, 128) if c <= N))
        for B in range(1, 9):
            for nT in (16, 64, 600000):          # (one and four 16-bin tiles: the kernels' tile-pair forms need four)
                for stim, Ds in ((0, 0), (0, 2), (0, 9), (0, 200), (1, 3 + 24), (2, 3 + 24), (3, 3 + 24), (2, 4 + 1024)):
                    for count in counts:
                        yield N, B, nT, stim, Ds, count


@functools.lru_cache(maxsize=None)
def reachable_both():
    """({kernel name: example shape} for the automatic dispatch, the same including the forcing options).  Computed once
    per process (~1 min); callers must not modify the dicts."""
    auto, forced = {}, {}
    for N, B, nT, stim, Ds, count in shapes():
        for ok in (0, 2, 3, 4, 6, 7):
            for f32 in ((0, 1, 2) if stim == 0 else (0,)):           # (2: f32 resident blocks of the narrow-shard kernel)
                for path in (0, 1, 2):
                    if path == 2 and count != N:
                        continue
                    key = (N, B, nT, stim, Ds, count, path, ok, f32)
                    try:
                        names = _lib.plan_kernels(N, B=B, R=200, Dstim=Ds, nT=nT, stim=stim, count=count, path=path,
                                                  opt_kernel=ok, opt_f32=f32)
                    except _lib.PglError as e:
                        if 'no kernel instantiation' not in str(e):
                            continue                 # no plan for this shape (the evaluation raises the same error)
                        names = ['MISSING: N=%d B=%d nT=%d stim=%d Dstim=%d count=%d path=%d opt_kernel=%d f32=%d' % key]
                    for n in names:
                        forced.setdefault(n, key)
                        if ok == 0:
                            auto.setdefault(n, key)
    return auto, forced


def reachable(auto_only=True):
    return reachable_both()[0 if auto_only else 1]


def case_names(case):
    """The dry run's launch sequence for one case of the table (a dict with FIELDS)."""
    c = dict((k, int(case[k])) for k in FIELDS)
    return _lib.plan_kernels(c['N'], B=c['B'], R=c['R'], Dstim=c['Dstim'], nT=c['nT'], stim=c['stim'], n_lo=c['n_lo'],
                             count=c['count'], path=c['path'], opt_kernel=c['opt_kernel'], opt_f32=c['opt_f32'])


def _case_cost(c):
    """Oracle work of a case (multiply-adds, roughly): features + the contraction of every evaluated row, both ways.  A
    separable stimulus is checked on its dense features (Bt = 3 temporal bases times Dstim - 3 spatial ones)."""
    ds = 3 * (c['Dstim'] - 3) if c['stim'] else c['Dstim']
    return c['nT'] * (c['N'] * c['B'] * 12 + 2 * c['count'] * (c['N'] * c['B'] + ds))


def emit_cases(nT=3000, short_nT=45, R=200):
    """One case per reachable instantiation: the cheapest shape of the grid that reaches it at nT bins (not a multiple of
    16: a ragged last time tile), or at short_nT where only a recording of fewer than four tiles reaches it; a neuron
    sub-range that ends at the last neuron (n_lo > 0) and a ragged last post tile where the same launches allow it.  A case
    reaches several instantiations: cases are taken cheapest first and an instantiation already run by a taken case gets
    none of its own."""
    want = set(reachable_both()[1])
    best = {}
    for T in (nT, short_nT):
        want -= set(n for n in best)                    # (the short recording only for what nT bins do not reach)
        for N, B, _, stim, Ds, count in (s for s in shapes() if s[2] == 16):
            for ok in (0, 2, 3, 4, 6, 7):
                for f32 in ((0, 1, 2) if stim == 0 else (0,)):
                    for path in (0, 1, 2):
                        if path == 2 and count != N:
                            continue
                        c = dict(N=N, B=B, R=R, Dstim=Ds, nT=T, stim=stim, n_lo=0, count=count, path=path, opt_kernel=ok,
                                 opt_f32=f32)
                        try:
                            names = case_names(c)
                        except _lib.PglError:
                            continue
                        cost = _case_cost(c)
                        if not any(n in want and (n not in best or cost < best[n][0][0]) for n in names):
                            continue
                        if count < N:                   # the last neurons: n_lo > 0, and (count % 16) rows in the last tile
                            c2 = dict(c, n_lo=N - count)
                            try:
                                if case_names(c2) == names:
                                    c = c2
                            except _lib.PglError:
                                pass
                        # prefer a ragged last post tile and n_lo > 0 at up to twice the cost
                        key = (_case_cost(c) * (1 if count % 16 else 2) * (1 if c['n_lo'] else 2), sorted(c.items()))
                        for n in names:
                            if n in want and (n not in best or key < best[n][0]):
                                best[n] = (key, c, names)
        if set(best) >= want:
            break
    missing = sorted(set(reachable_both()[1]) - set(best))
    if missing:
        raise RuntimeError("no case at nT = %d / %d reaches %s" % (nT, short_nT, missing))
    cases, covered = [], set()
    for n in sorted(best, key=lambda n: best[n][0]):
        if n in covered:
            continue
        _, c, names = best[n]
        cases.append(dict(c, names=names))
        covered.update(names)
    cases.sort(key=lambda c: (c['names'][0], _case_cost(c)))
    return cases


def write_cases(cases, path=CASES):
    with open(path, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(c, sort_keys=True) for c in cases) + '\n]\n')


def load_cases(path=CASES):
    with open(path) as f:
        return json.load(f)


def built_fused():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import kernel_resources as KR
    res = KR.kernel_resources(_lib.LIB_PATH)
    return dict((KR.short(n), r) for n, r in res.items())


# ---- Hessian-vector products (pgl_hvp_prepare_* / pgl_hvp_apply_dev) -------------------------------------------------
HVP_CASES = os.path.join(ROOT, 'tests', 'hvp_cases.json')
# list: 1 = the neurons are passed as a permuted list (pgl_hvp_prepare_list_dev); [t_lo, t_hi): the time range of the call
HVP_FIELDS = ('N', 'B', 'R', 'Dstim', 'nT', 'n_lo', 'count', 'opt_kernel', 'opt_f32', 'list', 't_lo', 't_hi')
HVP_OPTS = tuple((ok, f32) for ok in (0, 2, 4) for f32 in (0, 1))
DRY_CUS = 256                # the dry run's context has 256 CUs (the MI355X's): a resident-tile plan of one post block
                             # (<= 128 neurons, the only kind k_hvp5 runs) cuts the recording into min(256, tiles) chunks
# the forms of call every column pair of k_hvp5 runs in beside its base case (tests/test_gpu_hvp_sweep.py):
#   ring    every workgroup walks three time tiles (the DMA ring L_{i+1} / H_{i+1}); a sub-range that ends at the last
#           neuron with a ragged last post tile
#   list    a permuted, non-contiguous neuron list; at most one tile per workgroup (as trange, dstim)
#   trange  a time range with t_lo > 0 and t_hi not a multiple of 16
#   dstim   dense stimulus columns in a call of >= 65 neurons on the automatic dispatch
#   short   (one pair only) a recording of fewer than 16 bins
HVP_FORMS = ('ring', 'list', 'trange', 'dstim')
HVP_NT, HVP_RING_NT, HVP_SHORT_NT = 2989, 16 * 3 * DRY_CUS - 5, 11


def hvp_names(c):
    """The dry run's (prepare sequence, apply sequence) of one case (a dict with HVP_FIELDS)."""
    kw = dict(B=int(c['B']), R=int(c['R']), Dstim=int(c['Dstim']), nT=int(c['nT']), stim=0, n_lo=int(c['n_lo']),
              count=int(c['count']), opt_kernel=int(c['opt_kernel']), opt_f32=int(c['opt_f32']))
    return _lib.plan_kernels(int(c['N']), path=3, **kw), _lib.plan_kernels(int(c['N']), path=4, **kw)


def hvp_pair(names):
    """'KTL, KTH' of the k_hvp5 launch among the names, or None"""
    for n in names:
        if n.startswith('k_hvp5<'):
            return n[len('k_hvp5<'):].rsplit(',', 1)[0]
    return None


@functools.lru_cache(maxsize=None)
def hvp_reachable_both():
    """({kernel name: example}, the same including the forcing options, {(prepare sequence, apply sequence): example}) of
    the Hessian-vector paths over the shape grid (dense stimulus columns only: a separable stimulus is unsupported)."""
    auto, forced, seqs = {}, {}, {}
    for N, B, nT, stim, Ds, count in shapes():
        if stim:
            continue
        for ok, f32 in HVP_OPTS:
            c = dict(N=N, B=B, R=200, Dstim=Ds, nT=nT, n_lo=0, count=count, opt_kernel=ok, opt_f32=f32)
            key = (N, B, nT, Ds, count, ok, f32)
            try:
                prep, app = hvp_names(c)
            except _lib.PglError as e:
                if 'no kernel instantiation' not in str(e):
                    continue
                prep = app = ['MISSING: N=%d B=%d nT=%d Dstim=%d count=%d opt_kernel=%d f32=%d' % key]
            seqs.setdefault((tuple(prep), tuple(app)), key)
            for n in prep + app:
                forced.setdefault(n, key)
                if ok == 0 and f32 == 0:
                    auto.setdefault(n, key)
    return auto, forced, seqs


def hvp_roles(seqs):
    """What the table must hold, exactly: (role, key) -- a base case per sequence pair, a case per form and k_hvp5 column
    pair, one 'short' case."""
    pairs = sorted(set(hvp_pair(s[1]) for s in seqs) - {None})
    want = [('base', ' | '.join(s[0]) + ' || ' + ' | '.join(s[1])) for s in seqs]
    want += [(f, p) for f in HVP_FORMS for p in pairs]
    if pairs:
        want.append(('short', ''))
    return sorted(want)


def hvp_case_role(c):
    if c['role'] == 'base':
        return ('base', ' | '.join(c['prepare']) + ' || ' + ' | '.join(c['apply']))
    return (c['role'], '' if c['role'] == 'short' else hvp_pair(c['apply']))


def emit_hvp_cases(R=200):
    seqs = hvp_reachable_both()[2]
    pairs = sorted(set(hvp_pair(s[1]) for s in seqs) - {None})
    best = {}

    def offer(role, c, cost):
        key = (cost, sorted(c.items()))
        if role not in best or key < best[role][0]:
            best[role] = (key, c)

    for N, B, _, stim, Ds, count in (s for s in shapes() if s[2] == 16 and s[3] == 0):
        for ok, f32 in HVP_OPTS:
            c = dict(N=N, B=B, R=R, Dstim=Ds, nT=HVP_NT, n_lo=0, count=count, opt_kernel=ok, opt_f32=f32, list=0, t_lo=0,
                     t_hi=HVP_NT)
            try:
                prep, app = hvp_names(c)
            except _lib.PglError:
                continue
            cost = _case_cost(dict(c, stim=0))
            sub = None
            if count < N:                               # the last neurons: n_lo > 0
                sub = dict(c, n_lo=N - count)
                if hvp_names(sub) != (prep, app):
                    sub = None
            # base: a ragged last post tile and n_lo > 0 preferred at up to twice the cost (as emit_cases)
            b = sub or c
            offer(('base', ' | '.join(prep) + ' || ' + ' | '.join(app)), dict(b, role='base', prepare=prep, apply=app),
                  cost * (1 if count % 16 else 2) * (1 if b['n_lo'] else 2))
            pair = hvp_pair(app)
            if pair is None:
                continue
            if sub and count % 16 and count >= 4:
                ring = dict(sub, nT=HVP_RING_NT, t_hi=HVP_RING_NT)
                if hvp_names(ring) == (prep, app):
                    offer(('ring', pair), dict(ring, role='ring', prepare=prep, apply=app), _case_cost(dict(ring, stim=0)))
            if 4 <= count <= N - 3 and count % 16:
                offer(('list', pair), dict(c, list=1, role='list', prepare=prep, apply=app), cost)
            if count >= 4:
                offer(('trange', pair), dict(b, t_lo=112, t_hi=2501, role='trange', prepare=prep, apply=app),
                      cost * (1 if count % 16 else 2))
            if Ds > 0 and count >= 65 and ok == 0 and f32 == 0:
                offer(('dstim', pair), dict(b, role='dstim', prepare=prep, apply=app), cost)
            short = dict(b, nT=HVP_SHORT_NT, t_hi=HVP_SHORT_NT)
            if count >= 4 and hvp_names(short) == (prep, app):
                offer(('short', ''), dict(short, role='short', prepare=prep, apply=app), _case_cost(dict(short, stim=0)))
    missing = sorted(set(hvp_roles(seqs)) - set(best))
    if missing:
        raise RuntimeError("no case of the grid for %s" % missing)
    order = dict((r, i) for i, r in enumerate(('base',) + HVP_FORMS + ('short',)))
    cases = [best[r][1] for r in sorted(best, key=lambda r: (order[r[0]], r[1]))]
    return cases


if __name__ == '__main__':
    if '--emit-hvp-cases' in sys.argv:
        cs = emit_hvp_cases()
        write_cases(cs, HVP_CASES)
        print("%d cases for %d instantiations, reference work ~%.2g multiply-adds -> %s"
              % (len(cs), len(set(n for c in cs for n in c['prepare'] + c['apply'])),
                 sum(_case_cost(dict(c, stim=0)) for c in cs), HVP_CASES))
        sys.exit(0)
    if '--emit-cases' in sys.argv:
        cs = emit_cases()
        write_cases(cs)
        print("%d cases for %d instantiations, oracle work ~%.2g multiply-adds -> %s"
              % (len(cs), len(set(n for c in cs for n in c['names'])), sum(_case_cost(c) for c in cs), CASES))
        sys.exit(0)
    auto, forced = reachable_both()
    built = built_fused()
    bf = dict((n, r) for n, r in built.items() if n.startswith(FUSED))
    print("fused instantiations built: %d; reachable by the automatic dispatch: %d; reachable with a forcing option: %d"
          % (len(bf), len(auto), len(forced)))
    miss = sorted(n for n in forced if n not in bf)
    print("reachable but NOT built (%d): %s" % (len(miss), miss))
    dead = sorted(n for n in bf if n not in forced)
    print("built but not reachable (%d):" % len(dead))
    for n in dead:
        print("   ", n)
    bad = sorted(n for n in auto if n in bf and bf[n]['scratch'] > 0)
    print("automatically dispatched with scratch (%d): %s" % (len(bad), [(n, bf[n]['scratch'], auto[n]) for n in bad]))
    bad2 = sorted(n for n in forced if n in bf and bf[n]['scratch'] > 0 and n not in auto)
    print("reachable only with a forcing option, with scratch (%d): %s" % (len(bad2), [(n, bf[n]['scratch'], forced[n]) for n in bad2]))
    hauto, hforced, hseqs = hvp_reachable_both()
    hb = dict((n, r) for n, r in built.items() if n.startswith('k_hvp5<'))
    print("Hessian-vector paths: %d instantiations reachable by the automatic dispatch, %d with a forcing option, "
          "%d (prepare, apply) sequences" % (len(hauto), len(hforced), len(hseqs)))
    for n in sorted(hforced):
        print("    %-34s %s" % (n, 'auto' if n in hauto else 'forced only'))
    print("reachable by a product but NOT built: %s" % sorted(n for n in hforced if n not in built))
    print("k_hvp5 built but not reachable: %s" % sorted(n for n in hb if n not in hforced))
    print("reachable by a product, with scratch: %s" % sorted(n for n in hforced if n in built and built[n]['scratch'] > 0))
