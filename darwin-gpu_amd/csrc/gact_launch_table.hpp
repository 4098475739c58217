// gact_launch_table.hpp -- WHICH kernel a plan's MainK / SeedK names (gact_policy.hpp says what a pass runs as, gact_launch.hpp
// launches it).  The main kernels and the packed seed kernels are named HERE and nowhere else: the launches, the occupancy
// queries behind the persistent grids (gact_hip_create) and the warm-up launches (gact_hip_prepare) all read these tables, so
// a new layout is one row of main_kernel.  Included by gact_engine.hip behind the kernels' headers (it needs `fail`).
#pragma once

// every main kernel takes the same arguments, every packed seed kernel the same
typedef void (*MainFn)(gact::KParams, gact::P16Consts, gact::SeqSetDev, gact::SeqSetDev, gact::SeqSetDev, int, gact_overlap *,
                       gact::ChainQueues, uint32_t *);
typedef void (*SeedFn)(gact::KParams, gact::P16Consts, gact::SeqSetDev, gact::SeqSetDev, gact::SeqSetDev, const gact_candidate *, int, int,
                       int, int, gact_overlap *, gact::ChainQueues, uint32_t *);

// The forms of one main kernel: [0] on the pass its layout names, [1] on the row-drifted pass (gact_lin.hpp 12.), each for
// one set of queues and for two (overlapped seeding, ChainQueues::more_flag).  Null: the kernel has no such form.
struct MainEntry {
    MainFn plain[2], row[2];
    int threads;                         // of a block: kBlockThreads, or kRoleThreads
};

// C: columns per lane of the engine (20 or 32).  The linear-gap and the drifted affine kernels exist at 20 only.
template <int C> MainEntry main_kernel(gact_policy::MainK k)
{
    using M = gact_policy::MainK;
    using gact::extend_p16_kernel;
    constexpr int b256 = gact::kBlockThreads;
    if constexpr (C == 20) {
        using Lin = gact::SplitLayoutLin<7, 13>;
        using Row = gact::SplitLayoutLinRow<7, 13>;
        switch (k) {
        case M::RolesLin: return {{gact::extend_roles_kernel<Lin, false>, gact::extend_roles_kernel<Lin, true>},
                                  {gact::extend_roles_kernel<Row, false>, gact::extend_roles_kernel<Row, true>}, gact::kRoleThreads};
        case M::CoopLin: return {{gact::extend_coop_kernel<Lin, false>, gact::extend_coop_kernel<Lin, true>},
                                 {gact::extend_coop_kernel<Row, false>, gact::extend_coop_kernel<Row, true>}, b256};
        case M::SplitLin: return {{extend_p16_kernel<Lin, false>, extend_p16_kernel<Lin, false, true>},
                                  {extend_p16_kernel<Row, false>, extend_p16_kernel<Row, false, true>}, b256};
        case M::SplitLinTeam: return {{extend_p16_kernel<gact::SplitLayoutLinTeam<7, 13>, false>, nullptr},
                                      {extend_p16_kernel<gact::SplitLayoutLinRowTeam<7, 13>, false>, nullptr}, b256};
        case M::WideLin: return {{extend_p16_kernel<gact::WideLayoutLin, false>, extend_p16_kernel<gact::WideLayoutLin, false, true>}, {}, b256};
        case M::SplitAffNeg: return {{extend_p16_kernel<gact::SplitLayoutAff<7, 13, true>, false>, nullptr}, {}, b256};
        case M::SplitAff: return {{extend_p16_kernel<gact::SplitLayoutAff<7, 13, false>, false>, nullptr}, {}, b256};
        default: break;
        }
    }
    switch (k) {
    case M::WideTaggedRaw: return {{extend_p16_kernel<gact::WideLayoutTagged, true>, nullptr}, {}, b256};
    case M::WideTagged: return {{extend_p16_kernel<gact::WideLayoutTagged, false>, nullptr}, {}, b256};
    case M::WideRaw: return {{extend_p16_kernel<gact::WideLayout, true>, nullptr}, {}, b256};
    case M::Wide: return {{extend_p16_kernel<gact::WideLayout, false>, nullptr}, {}, b256};
    case M::SplitTaggedRaw: return {{extend_p16_kernel<gact::SplitLayout<7, 13, true>, true>, nullptr}, {}, b256};
    case M::SplitTagged: return {{extend_p16_kernel<gact::SplitLayout<7, 13, true>, false>, nullptr}, {}, b256};
    case M::SplitRaw: return {{extend_p16_kernel<gact::SplitLayout<7, 13>, true>, nullptr}, {}, b256};
    case M::Split: return {{extend_p16_kernel<gact::SplitLayout<7, 13>, false>, nullptr}, {}, b256};
    case M::UniformTaggedRaw: return {{extend_p16_kernel<gact::UniformLayout<C, gact::kGroup, true>, true>, nullptr}, {}, b256};
    case M::UniformTagged: return {{extend_p16_kernel<gact::UniformLayout<C, gact::kGroup, true>, false>, nullptr}, {}, b256};
    case M::UniformRaw: return {{extend_p16_kernel<gact::UniformLayout<C>, true>, nullptr}, {}, b256};
    case M::Uniform: return {{extend_p16_kernel<gact::UniformLayout<C>, false>, nullptr}, {}, b256};
    default: break;
    }
    return {{}, {}, b256};               // MainK::None; a linear-gap or affine kernel at 32 columns per lane
}

// SeedK::Int32 is chain_kernel<C, SeedSink>, with arguments of its own: launched where it is planned (gact_launch.hpp launch_seed)
template <int C> SeedFn seed_kernel(gact_policy::SeedK k)
{
    using S = gact_policy::SeedK;
    if constexpr (C == 20) {
        switch (k) {
        case S::P16Lin: return gact::seed_p16_kernel<C, false, 1>;
        case S::P16Aff: return gact::seed_p16_kernel<C, false, 2>;
        case S::P16AffNeg: return gact::seed_p16_kernel<C, false, 3>;
        default: break;
        }
    }
    switch (k) {
    case S::P16Raw: return gact::seed_p16_kernel<C, true>;
    case S::P16: return gact::seed_p16_kernel<C, false>;
    default: break;
    }
    return nullptr;
}

inline MainEntry main_entry(int C, gact_policy::MainK k) { return C == 20 ? main_kernel<20>(k) : main_kernel<32>(k); }
inline SeedFn seed_entry(int C, gact_policy::SeedK k) { return C == 20 ? seed_kernel<20>(k) : seed_kernel<32>(k); }

// The form of `k` a launch takes, the fallbacks stated once: a kernel without a row-drifted form runs on the pass its layout
// names (WideLin, and everything that is not linear-gap), one without a two-set form runs its one-set form (SplitLinTeam, the
// affine kernels, everything that is not linear-gap).  A kernel this engine does not have at all is an error, not a launch of
// nothing.
inline int resolve_main(int C, gact_policy::MainK k, bool row_drift, bool two_sets, MainFn *fn, int *threads)
{
    const MainEntry en = main_entry(C, k);
    const MainFn *forms = (row_drift && en.row[0]) ? en.row : en.plain;
    *fn = (two_sets && forms[1]) ? forms[1] : forms[0];
    *threads = en.threads;
    if (!*fn) return fail(GACT_HIP_EDEVICE, "main launch: no kernel %s at %d columns per lane", gact_policy::name(k), C);
    return 0;
}

inline int resolve_seed(int C, gact_policy::SeedK k, SeedFn *fn)
{
    *fn = seed_entry(C, k);
    if (!*fn) return fail(GACT_HIP_EDEVICE, "seed launch: no kernel %s at %d columns per lane", gact_policy::name(k), C);
    return 0;
}

// The fewest resident blocks per CU over `kernels` at `threads` per block, at least one (nulls -- forms a row does not have --
// are passed over).
inline int min_resident_blocks(const std::vector<const void *> &kernels, int threads, int *out)
{
    int m = 0x7fffffff;
    for (const void *k : kernels) {
        if (!k) continue;
        int b = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k, threads, 0));
        m = std::min(m, b);
    }
    *out = std::max(1, m == 0x7fffffff ? 0 : m);
    return 0;
}

// The kernels behind each persistent grid of gact_hip_create: a grid holds as many blocks per CU as the LEAST of its kernels
// keeps resident.  The lists are what each grid has been measured with, and some are incomplete: the cooperative kernels are
// in none (they run on lin_grid_blocks), nor are SplitAff (aff_grid_blocks is SplitAffNeg's) and the P16Aff
// seed kernel.  Changing a list changes a grid, which is a change of behaviour with a measurement of its own.
// (The linear-gap kernels exist at 20 columns per lane only; their grids are asked for at either C, as they always were: an
//  engine at 32 whose scoring is linear sizes its workspace by them.)
enum class Grid { Main, Lin, WideLin, Role, Aff, Seed, SeedLin };
inline int grid_blocks_per_cu(int C, Grid g, int *out)
{
    using M = gact_policy::MainK;
    using S = gact_policy::SeedK;
    auto p = [](auto f) { return reinterpret_cast<const void *>(f); };
    const int b256 = gact::kBlockThreads;
    switch (g) {
    case Grid::Main: {                   // the int32 kernels and the twelve main kernels that are neither linear-gap nor drifted affine
        std::vector<const void *> ks = {C == 20 ? p(gact::chain_kernel<20, gact::SeedSink>) : p(gact::chain_kernel<32, gact::SeedSink>),
                                        C == 20 ? p(gact::align_tiles_kernel<20>) : p(gact::align_tiles_kernel<32>)};
        for (int k = (int)M::WideTaggedRaw; k <= (int)M::Uniform; k++) ks.push_back(p(main_entry(C, (M)k).plain[0]));
        return min_resident_blocks(ks, b256, out);
    }
    case Grid::Lin: {                    // the one-set split launches, on either pass: one grid serves whichever the scoring takes
        const MainEntry s = main_kernel<20>(M::SplitLin), t = main_kernel<20>(M::SplitLinTeam);
        return min_resident_blocks({p(s.plain[0]), p(t.plain[0]), p(s.row[0]), p(t.row[0])}, b256, out);
    }
    case Grid::WideLin: return min_resident_blocks({p(main_kernel<20>(M::WideLin).plain[0])}, b256, out);
    case Grid::Role: {
        const MainEntry r = main_kernel<20>(M::RolesLin);
        return min_resident_blocks({p(r.plain[0]), p(r.plain[1]), p(r.row[0]), p(r.row[1])}, r.threads, out);
    }
    case Grid::Aff: return min_resident_blocks({p(main_kernel<20>(M::SplitAffNeg).plain[0])}, b256, out);
    case Grid::Seed: return min_resident_blocks({p(seed_entry(C, S::P16Raw)), p(seed_entry(C, S::P16)), p(seed_entry(C, S::P16AffNeg))}, b256, out);
    case Grid::SeedLin:                  // the linear-gap seed kernel fits three waves per SIMD (at 32 columns per lane there is none: P16's figure)
        return min_resident_blocks({p(seed_entry(C, S::P16Lin) ? seed_entry(C, S::P16Lin) : seed_entry(C, S::P16))}, b256, out);
    }
    return 0;
}
