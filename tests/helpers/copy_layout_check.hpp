// copy_layout_check.hpp -- the layout of a call's one copy (llcomp_amd/csrc/windows_plan.hpp: CopyLayout) as the stand-alone planner
// checks see it (windows_plan_check.cpp, pad_plan_check.cpp, warp_plan_check.cpp): for a plan's table and a tail's block of
// `block_bytes`, without a gather and with one of the classes' slices at up to the per-slice entry limit, without chains and with
// those of up to `views` views -- where the gather's arrays, the block and the chains sit, and the whole copy against the sum the
// entry points hand the driver as its bound: stage_bound + *bound (the call's tables bound; null: none holds, an output larger than the
// image) + photo_tables_bound(views) where there are chains.  The including program links photo_plan.cpp for that last bound.
#pragma once
#include <cstdio>
#include <random>

#include "../../include/llcomp_mi.h"
#include "container.hpp"
#include "photo_plan.hpp"
#include "windows_plan.hpp"

namespace llcomp_mi {

#define COPY_LAYOUT_CHECK(x)                                                          \
    do {                                                                              \
        if (!(x)) {                                                                   \
            std::printf("FAILED %s (copy_layout_check.hpp line %d)\n", #x, __LINE__); \
            return false;                                                             \
        }                                                                             \
    } while (0)

inline bool copy_layout_ok(const Geometry& g, const WindowsPlan& p, bool tail, uint64_t block_bytes, uint64_t views, const uint64_t* bound, uint32_t seed) {
    std::mt19937 rng(seed);  // (a generator of its own: the including program's rounds keep their draws)
    // a gather of the classes' slices: any payload up to the entry limit of every slice, now and then the limit itself
    RegionsGather gp;
    for (uint32_t i = 0; i < p.n_classes; ++i) gp.n_slices += p.classes[i].sub.n_slices;
    COPY_LAYOUT_CHECK(gp.n_slices <= g.n_slices);
    const uint64_t most = uint64_t(gp.n_slices) * (g.slice_cap - 16);
    gp.payload_bytes = rng() % 4 == 0 ? most : rng() % (most + 1);
    // no chains, every view's, and those of some of the views (the active groups')
    const uint64_t chain_counts[3] = {0, views, views ? 1 + rng() % views : 0};
    for (const RegionsGather* src : {static_cast<const RegionsGather*>(nullptr), static_cast<const RegionsGather*>(&gp)})
        for (uint64_t n_chains : chain_counts) {
            if (n_chains && !tail) continue;  // (only the calls with a tail take chains)
            const uint64_t chain_bytes = n_chains * sizeof(llcomp_mi_photo_chain);
            const CopyLayout cl(p.tab.size(), src, tail, block_bytes, chain_bytes);
            COPY_LAYOUT_CHECK(cl.stage.len_at == p.tab.size() * sizeof(RegionsFrame) && cl.stage.off_at % 8 == 0);
            COPY_LAYOUT_CHECK(cl.stage.off_at >= cl.stage.len_at + 4 * uint64_t(src ? gp.n_slices : 0));
            COPY_LAYOUT_CHECK(cl.stage.pay_at == cl.stage.off_at + 8 * uint64_t(src ? gp.n_slices : 0));
            COPY_LAYOUT_CHECK(cl.stage.bytes == cl.stage.pay_at + (src ? gp.payload_bytes : 0));
            COPY_LAYOUT_CHECK(cl.rs_at % 16 == 0 && cl.rs_at >= cl.stage.bytes && cl.rs_at < cl.stage.bytes + 16);
            COPY_LAYOUT_CHECK(cl.block_end == (tail ? cl.rs_at + block_bytes : cl.stage.bytes));
            COPY_LAYOUT_CHECK(cl.chains_at % 16 == 0 && cl.chains_at >= cl.block_end && cl.chains_at < cl.block_end + 16);
            COPY_LAYOUT_CHECK(cl.bytes == (n_chains ? cl.chains_at + chain_bytes : cl.block_end));
            if (bound) COPY_LAYOUT_CHECK(cl.bytes <= stage_bound(g) + *bound + (n_chains ? photo_tables_bound(views) : 0));
        }
    return true;
}

}  // namespace llcomp_mi
