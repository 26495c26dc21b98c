"""The set of fused kernel instantiations the dispatcher can reach, from a dry run of make_plan / the launch switches over
a grid of shapes (pgl_plan_kernels: no GPU needed), against the instantiations in the built library:

    python tools/reachable_kernels.py            # summary + instantiations no plan reaches + reachable ones with scratch
    python tools/reachable_kernels.py --emit-cases   # rewrite tests/dispatch_cases.json (one cheap case per instantiation)

`reachable(auto_only)` is what tests/test_capi_symbols.py uses: every instantiation reachable WITHOUT a forcing option
must exist in the library and use no scratch.  tests/test_dispatch_cases.py holds the committed case table to the same
set, tests/test_gpu_dispatch_sweep.py runs every case against the oracle."""
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


if __name__ == '__main__':
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
