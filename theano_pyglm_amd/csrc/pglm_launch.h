// Launch layer of the fused kernels (host side; included by pglm_capi.hip after pglm_plan.h): the dry run's record, ONE launch
// primitive (launch_kernel), ONE dispatcher from run-time plan fields to template instantiations (dispatch over the lists of
// pglm_plan.h, limited by its *_built predicates), and a launcher per kernel family on top of the two.
// The compiler emits the kernels in the order the launchers below name them -- launcher after launcher, list element after
// list element, outer dispatch before inner -- and the code it generates for some of them (k_fused2 / 6 / 8) differs in
// details with their place in the code object.  To keep the code object byte for byte, keep this order when editing: compare
// the kernel symbol order of the built library (tools/kernel_resources.py has the extraction) before and after.
#pragma once

// Dry run of the dispatch (pgl_plan_kernels): when g_dry is set launch_kernel records the name of the kernel
// instantiation it would launch (as the code object's demangled symbol reads) and launches nothing.  The recorded set
// over a grid of shapes is the set of instantiations the dispatcher can reach: tests/test_capi_symbols.py holds every
// one of them to zero bytes of scratch, tools/reachable_kernels.py diffs it against the built library.  When g_rec is set
// instead (a real evaluation with PGL_OPT_RECORD_KERNELS), the name is recorded the same way and the launch goes ahead:
// returns true when the caller must NOT launch.
static bool dry_record(const char* fam, std::initializer_list<int> args, const char* tail = nullptr)
{
    if (!g_dry && !g_rec) return false;
    std::string n = std::string(fam) + "<";
    bool first = true;
    for (int a : args) {
        if (!first) n += ", ";
        n += std::to_string(a);
        first = false;
    }
    if (tail) n += std::string(", ") + tail;
    n += ">";
    (g_dry ? g_dry : g_rec)->push_back(n);
    return g_dry != nullptr;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) costs several microseconds of host time: it is issued once per
// kernel instantiation and device (and again only for a larger size), not on every launch -- the small configurations
// are bound by the host's submission rate (tools/step_bench.py)
template <typename K>
static hipError_t ensure_dyn_lds(K kern, size_t bytes)
{
    static std::map<std::pair<const void*, int>, size_t> have;      // (kernel, device) -> size already granted
    static std::mutex mu;                                           // ctypes drops the GIL: one handle per thread is legal
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    size_t& h = have[std::make_pair(reinterpret_cast<const void*>(kern), dev)];
    if (bytes <= h) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e == hipSuccess) h = bytes;
    return e;
}

// record -> (dry run: return) -> dynamic LDS grant -> launch -> launch error: every fused and k_hvp5 launch goes through
// here.  fam / targs / tail spell the instantiation's name for dry_record, whose early return is the first thing that happens.
template <typename K, typename... A>
static hipError_t launch_kernel(K kern, const char* fam, std::initializer_list<int> targs, const char* tail, dim3 grid,
                                dim3 block, size_t lds, hipStream_t s, const A&... args)
{
    if (dry_record(fam, targs, tail)) return hipSuccess;
    hipError_t e = ensure_dyn_lds(kern, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, V>) for the V of the list that equals v; hipErrorInvalidValue when none does (under the dry
// run: "no kernel instantiation for this plan").  PGL_CV(c): the value of such a constant, usable as a template argument.
template <int... Vs, typename F>
static hipError_t dispatch(IntList<Vs...>, int v, F&& f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(... || (v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)));
    return e;
}
#define PGL_CV(c) decltype(c)::value

// version 4: the two-pass kernel with in-kernel features; the second pass (other half of G) for the gradient only
static hipError_t launch_fused3(const Plan& pl, const FusedParams& fp, hipStream_t s)
{
    return dispatch(KTilesHalf{}, pl.KTW, [&](auto kth) -> hipError_t {
        constexpr int KTH = PGL_CV(kth);
        hipError_t e = launch_kernel(k_fused3<KTH, PGL_CAP, 1>, "k_fused3", {KTH, PGL_CAP, 1}, nullptr, dim3(pl.blocks),
                                     dim3(512), pl.lds, s, fp);
        if (e != hipSuccess || !fp.want_grad) return e;
        return launch_kernel(k_fused3<KTH, PGL_CAP, 2>, "k_fused3", {KTH, PGL_CAP, 2}, nullptr, dim3(pl.blocks), dim3(512),
                             pl.lds, s, fp);
    });
}

// version 5, the two-pass kernel on resident tiles: one launch of the form (PASS, XIN, PART) for the plan's column pair, with
// helper waves when the plan asks for them.  Pass 1 takes the plan's LDS, pass 2 two images of the part it contracts.
// Hlps / Forms: the helper variants and forms a call site can ask for.
constexpr int form5(int pass, int xin, int part) { return pass << 4 | xin << 2 | part; }
template <typename Hlps, typename Forms>
static hipError_t launch_fused5_form(const Plan& pl, const FusedParams& fp, hipStream_t s, int form)
{
    return dispatch(Hlps{}, pl.hlp, [&](auto hlp) -> hipError_t {
        return dispatch(ColPairs{}, col_pair(pl.ktl, pl.kth), [&](auto pr) -> hipError_t {
            return dispatch(Forms{}, form, [&](auto f) -> hipError_t {
                constexpr int KTL = pair_l(PGL_CV(pr)), KTH = pair_h(PGL_CV(pr)), HLP = PGL_CV(hlp);
                constexpr int PASS = PGL_CV(f) >> 4, XIN = PGL_CV(f) >> 2 & 3, PART = PGL_CV(f) & 3;
                if constexpr (fused5_built(KTL, XIN, PART, HLP)) {
                    const size_t lds = PASS == 1 ? pl.lds : (size_t)2 * pgl_img_bytes(PART ? KTL : KTH) + 256;
                    return launch_kernel(k_fused5<KTL, KTH, PASS, XIN, PART, HLP>, "k_fused5", {KTL, KTH, PASS, XIN, PART, HLP},
                                         nullptr, dim3(pl.blocks), dim3(512), lds, s, fp);
                } else {
                    return hipErrorInvalidValue;
                }
            });
        });
    });
}

// passes: 1, 2, or 0 = both back to back (pass 2 for the gradient only).  xin = 1: the slab-input form of pass 1 (separable
// stimulus at the frame rate, 65 .. 128 neurons: at least 5 post tiles of >= 2 bases; it has no helper variant, make_plan)
static hipError_t launch_fused5(const Plan& pl, const FusedParams& fp, hipStream_t s, int pass = 0, int xin = 0)
{
    using Plain = IntList<form5(1, 0, 0), form5(2, 0, 0)>;
    hipError_t e = hipSuccess;
    if (pass != 2)
        e = !xin ? launch_fused5_form<IntList<1, 0>, Plain>(pl, fp, s, form5(1, 0, 0))
                 : launch_fused5_form<IntList<0>, IntList<form5(1, 1, 0)>>(pl, fp, s, form5(1, 1, 0));
    if (e == hipSuccess && pass != 1 && fp.want_grad) e = launch_fused5_form<IntList<1, 0>, Plain>(pl, fp, s, form5(2, 0, 0));
    return e;
}

// column slices of a wide population (N > 128 or more than 640 feature columns) on resident tiles.  mode 0: forward only,
// the slice's partial currents written to the slab; 1: forward only, added to the slab; 2: the last slice -- pass 1 from the
// slab (epilogue, residuals out, G of its L columns); 3: pass 2 on the H part; 4: pass 2 on the L part (the gradient of the
// L columns of a slice whose pass 1 was forward only)
static hipError_t launch_fused5_wide(const Plan& pl, const FusedParams& fp, hipStream_t s, int mode)
{
    using Modes = IntList<form5(1, 2, 0), form5(1, 3, 0), form5(1, 1, 0), form5(2, 0, 0), form5(2, 0, 1)>;
    if (mode < 0 || mode > 4) return hipErrorInvalidValue;
    return launch_fused5_form<IntList<1, 0>, Modes>(pl, fp, s, Modes::values[mode]);
}

// fused apply (fwo = 0) / forward-only curvature pass (fwo = 1) of the Hessian-vector product on resident tiles (k_hvp5)
static hipError_t launch_hvp5(const Plan& pl, const FusedParams& fp, const double* cslab, hipStream_t s, int fwo)
{
    return dispatch(ColPairs{}, col_pair(pl.ktl, pl.kth), [&](auto pr) -> hipError_t {
        return dispatch(IntList<0, 1>{}, fwo, [&](auto f) -> hipError_t {
            constexpr int KTL = pair_l(PGL_CV(pr)), KTH = pair_h(PGL_CV(pr)), FWO = PGL_CV(f);
            if constexpr (hvp5_built(KTL)) {
                constexpr size_t lds = (size_t)2 * pgl_img_bytes(KTL) + pgl_img_bytes(KTH);
                return launch_kernel(k_hvp5<KTL, KTH, FWO>, "k_hvp5", {KTL, KTH, FWO}, nullptr, dim3(pl.blocks), dim3(512), lds,
                                     s, fp, cslab);
            } else {
                return hipErrorInvalidValue;
            }
        });
    });
}

// version 6, the K-split scheme on resident tiles.  occ != nullptr: no launch, *occ = workgroups of this instantiation a CU
// holds with pl.lds bytes of LDS
template <int KTW, int PTW, int MT, int NW, int DB = 1>
static hipError_t launch_fused6_t(const Plan& pl, const FusedParams& fp, hipStream_t s, int* occ)
{
    constexpr size_t need = (size_t)(DB ? 2 : 1) * MT * pgl_img_bytes(KTW * (NW / PTW)) + (size_t)MT * NW * 2048 + 256 + (size_t)NW * 384;
    if constexpr (need <= 160 * 1024 && KTW * 4 <= 40 && (DB == 0 || fused6_built(KTW, PTW, MT, NW))) {
        auto kern = k_fused6<KTW, PTW, MT, NW, DB>;
        if (occ) {
            if (g_dry) return hipErrorInvalidValue;              // (dry run: no device to ask; the caller's default holds)
            hipError_t e = ensure_dyn_lds(kern, pl.lds);
            if (e != hipSuccess) return e;
            return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kern, NW * 64, pl.lds);
        }
        return launch_kernel(kern, "k_fused6", {KTW, PTW, MT, NW, DB}, nullptr, dim3(pl.blocks), dim3(NW * 64), pl.lds, s, fp);
    } else {
        return hipErrorInvalidValue;
    }
}

template <int NW>
static hipError_t launch_fused6_nw(const Plan& pl, const FusedParams& fp, hipStream_t s, int* occ)
{
    return dispatch(IntList<1, 2, 4>{}, pl.PTW, [&](auto ptw) -> hipError_t {
        return dispatch(IntList<1, 2>{}, pl.mt, [&](auto mt) -> hipError_t {
            return dispatch(KTilesSplit{}, pl.KTW, [&](auto ktw) -> hipError_t {
                return launch_fused6_t<PGL_CV(ktw), PGL_CV(ptw), PGL_CV(mt), NW>(pl, fp, s, occ);
            });
        });
    });
}

static hipError_t launch_fused6(const Plan& pl, const FusedParams& fp, hipStream_t s, int* occ = nullptr)
{
    if (pl.nw6 == 4) return launch_fused6_nw<4>(pl, fp, s, occ);
    if (pl.sb6 == 2) {                             // one post tile of a 25 .. 40 k-tile row: per-wave block rings
        if (pl.mt != 1 || pl.PTW != 1 || pl.KTW != 5 || occ) return hipErrorInvalidValue;
        return dispatch(IntList<1, 0>{}, pl.img32, [&](auto img32) -> hipError_t {
            return launch_kernel(k_fused8<5, kRing8, PGL_CV(img32)>, "k_fused8", {5, kRing8, PGL_CV(img32)}, nullptr,
                                 dim3(pl.blocks), dim3(512), pl.lds, s, fp);
        });
    }
    if (pl.sb6) {                                  // one image buffer: 640-column rows for two post tiles
        if (pl.mt == 1 && pl.PTW == 2 && pl.KTW == 10) return launch_fused6_t<10, 2, 1, 8, 0>(pl, fp, s, occ);
        return hipErrorInvalidValue;
    }
    return launch_fused6_nw<8>(pl, fp, s, occ);
}

// workgroups per CU of the k_fused6 instantiation a plan selects (registers and LDS), cached per shape
static int fused6_wg_per_cu(const Plan& pl)
{
    // dry run (pgl_plan_kernels): no device to ask -- the default, and neither read nor written to the cache, so that the
    // answer does not depend on what real evaluations of this process have cached.  (Occupancy sets the number of time
    // chunks only, never which instantiation a plan launches: the dry run's names hold on any device.)
    if (g_dry) return (pl.nw6 == 4) ? 2 : 1;
    // occupancy is a property of the kernel and the architecture (every device of a node is the same gfx950 part)
    static int cache[2][11][5][3][9];          // [sb6][KTW][PTW][mt][nw6]; 0 = not asked yet
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    int& c = cache[pl.sb6 ? 1 : 0][pl.KTW][pl.PTW][pl.mt][pl.nw6];
    if (c == 0) {
        int occ = 0;
        FusedParams fp{};
        if (launch_fused6(pl, fp, nullptr, &occ) != hipSuccess || occ < 1) occ = (pl.nw6 == 4) ? 2 : 1;
        c = occ;
    }
    return c;
}

// version 7: one wave per post tile carries the whole row.  xio 1 .. 3: the slab-input forms of a separable stimulus at the
// frame rate -- 2: stimulus current inside the forward contraction, 3: its backward inside the kernel as well (no residual slab)
static hipError_t launch_fused7(const Plan& pl, const FusedParams& fp, hipStream_t s, int xio = 0)
{
    return dispatch(IntList<3, 2, 1, 0>{}, xio, [&](auto x) -> hipError_t {
        return dispatch(IntList<1, 2, 4>{}, pl.nw7, [&](auto nwv) -> hipError_t {
            return dispatch(KTilesRow{}, pl.KT, [&](auto kt) -> hipError_t {
                constexpr int KT = PGL_CV(kt), NWV = PGL_CV(nwv), XIO = PGL_CV(x);
                if constexpr (fused7_built(KT, NWV, XIO))
                    return launch_kernel(k_fused7<KT, NWV, XIO>, "k_fused7", {KT, NWV, XIO}, nullptr, dim3(pl.blocks),
                                         dim3(NWV * 64), pl.lds, s, fp);
                else
                    return hipErrorInvalidValue;
            });
        });
    });
}

// versions 2 / 3: the K-split kernel with in-kernel features, f64 or f32
static hipError_t launch_fused2(const Plan& pl, const FusedParams& fp, hipStream_t s)
{
    return dispatch(IntList<1, 0>{}, pl.version == 3 ? 1 : 0, [&](auto f32) -> hipError_t {
        using FT = std::conditional_t<PGL_CV(f32) == 1, float, double>;
        return dispatch(IntList<1, 2, 4>{}, pl.PTW, [&](auto ptw) -> hipError_t {
            return dispatch(KTilesSplit{}, pl.KTW, [&](auto ktw) -> hipError_t {
                constexpr int KTW = PGL_CV(ktw), PTW = PGL_CV(ptw), NW = 8;
                if constexpr (fused2_built(KTW, NW / PTW))
                    return launch_kernel(k_fused2<KTW, PTW, NW, PGL_CAP, FT>, "k_fused2", {KTW, PTW, NW, PGL_CAP},
                                         sizeof(FT) == 4 ? "float" : "double", dim3(pl.blocks), dim3(NW * 64), pl.lds, s, fp);
                else
                    return hipErrorInvalidValue;
            });
        });
    });
}

// the fused launch(es) of a plan, whatever its version
static hipError_t launch_plan(const Plan& pl, const FusedParams& fp, hipStream_t s)
{
    if (pl.version == 7) return launch_fused7(pl, fp, s);
    if (pl.version == 6) return launch_fused6(pl, fp, s);
    if (pl.version == 5) return launch_fused5(pl, fp, s);
    if (pl.version == 4) return launch_fused3(pl, fp, s);
    return launch_fused2(pl, fp, s);
}

// the weighted Gram contraction of the dense Hessian: slab = layout of the prepared curvature (0 rows, 1 accumulator-layout slab)
static hipError_t launch_hess(const HessParams& hp, int slab, unsigned blocks, size_t lds, hipStream_t s)
{
    return dispatch(IntList<0, 1>{}, slab, [&](auto sl) -> hipError_t {
        return launch_kernel(k_hess<PGL_CV(sl)>, "k_hess", {PGL_CV(sl)}, nullptr, dim3(blocks), dim3(512), lds, s, hp);
    });
}
