// pad_plan_check.cpp -- the host planner of the padded calls (llcomp_amd/csrc/windows_plan.hpp: padded_setup, padded_views_setup;
// resize_plan.hpp: pad_axis, padded_frame_weights) under a sanitizer: over seeded random geometries, pad modes, fills and batches every
// source rectangle lies inside the image, the windows are those of the unpadded plan for the source rectangles, no tap and no bias or fill
// offset leaves its array, the block -- put into a heap buffer of exactly its size -- and the call's one copy stay within the padded
// tables bound, a views plan's unions are the bounding boxes of its views' source rectangles, and every refusal is refused.  Host code
// only; built and run by tests/test_pad_plan.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/pad_plan_check.cpp llcomp_amd/csrc/container.cpp llcomp_amd/csrc/windows_plan.cpp llcomp_amd/csrc/resize_plan.cpp
//       llcomp_amd/csrc/photo_plan.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "container.hpp"
#include "copy_layout_check.hpp"
#include "windows_plan.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

namespace {

std::mt19937 rng(20261019);
uint32_t pick(uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); }

uint32_t limit_of(uint32_t mode, uint32_t n) { return mode == LLCOMP_MI_PAD_REFLECT ? n - 1 : n; }

// one axis of a rectangle: inside the image, out by one side or by both, or at the mode's limit
void pick_axis(uint32_t mode, uint32_t n, int32_t& x, int32_t& r) {
    const uint32_t lim = limit_of(mode, n), kind = pick(0, 5);
    const uint32_t p = kind == 0 || kind == 3 ? 0 : kind == 4 ? lim : pick(0, lim);
    const uint32_t e = kind == 0 || kind == 2 ? 0 : kind == 5 ? lim : pick(0, lim);
    const int64_t a = p ? -int64_t(p) : int64_t(pick(0, n - 1));
    const int64_t b = e ? int64_t(n) + e : int64_t(pick(uint32_t(std::max<int64_t>(a, 0)) + 1, n));
    x = int32_t(a);
    r = int32_t(b - a);
}

// the block of a padded plan: every entry inside its box, every tap inside the entry's source rectangle, the bias and fill inside the
// weights; the block in exactly bytes() bytes; the copy within stage_bound + the padded tables bound for the most a gather can stage
int check_block(const Geometry& g, const WindowsPlan& p, const ResampleTail& t, uint32_t boxes, bool with_bias, const uint8_t* fill, uint64_t bound) {
    const ResampleBlock& b = t.block;
    CHECK(b.biased.size() == (with_bias ? b.rs.size() : 0));
    uint64_t entries = 0;
    for (const ResampleGroup& vg : t.groups) {
        CHECK(vg.first == entries && vg.chunk >= 1 && vg.chunk <= vg.n);
        entries += vg.n;
        CHECK(uint64_t(vg.chunk) * vg.mh * vg.ow * g.c <= t.mid_bytes);
        for (uint32_t i = 0; i < vg.n; ++i) {
            const ResizeFrame& z = b.rs[vg.first + i];
            CHECK(uint64_t(z.ox) + z.rw <= p.wmax && uint64_t(z.oy) + z.rh <= p.hmax && z.box < boxes);
            CHECK(z.rh <= vg.mh && z.kx && z.ky && z.kx <= 129 && z.ky <= 129);
            CHECK(uint64_t(z.hx) + uint64_t(vg.ow) * (z.kx + 1) <= b.w.size() && uint64_t(z.vy) + uint64_t(vg.oh) * (z.ky + 1) <= b.w.size());
            for (uint32_t o = 0; o < vg.ow; ++o) CHECK(b.w[z.hx + o] >= 0 && uint64_t(b.w[z.hx + o]) + z.kx <= z.rw);
            for (uint32_t o = 0; o < vg.oh; ++o) CHECK(b.w[z.vy + o] >= 0 && uint64_t(b.w[z.vy + o]) + z.ky <= z.rh);
            if (!with_bias) {
                CHECK(z.pad[0] == 0 && z.pad[1] == 0);
                continue;
            }
            CHECK(uint64_t(z.pad[0]) + vg.ow + vg.oh <= b.w.size() && uint64_t(z.pad[1]) + g.c <= b.w.size());
            bool any = false;
            for (uint32_t o = 0; o < vg.ow + vg.oh; ++o) any = any || b.w[z.pad[0] + o] != 0;
            CHECK(any == (b.biased[vg.first + i] != 0));
            for (uint32_t ch = 0; ch < g.c; ++ch) CHECK(b.w[z.pad[1] + ch] == int32_t(fill[ch]));
        }
    }
    CHECK(entries == b.rs.size());
    CHECK(t.box_bytes == uint64_t(boxes) * p.wmax * p.hmax * g.c && t.box_bytes <= uint64_t(g.frames) * g.w * g.h * g.c);
    std::unique_ptr<uint8_t[]> heap(new uint8_t[b.bytes()]);
    b.put(heap.get());
    RegionsGather gp;
    for (uint32_t i = 0; i < p.n_classes; ++i) gp.n_slices += p.classes[i].sub.n_slices;
    gp.payload_bytes = uint64_t(gp.n_slices) * (g.slice_cap - 16);
    for (const RegionsGather* src : {static_cast<const RegionsGather*>(nullptr), static_cast<const RegionsGather*>(&gp)}) {
        const CopyLayout cl(p.tab.size(), src, &t);
        CHECK(cl.rs_at % 16 == 0 && cl.bytes == cl.rs_at + b.bytes());
        if (bound) CHECK(cl.bytes <= stage_bound(g) + bound);
    }
    // ... and with photometric chains behind the block, as a padded photo views call lays them
    CHECK(copy_layout_ok(g, p, true, b.bytes(), b.rs.size(), bound ? &bound : nullptr, uint32_t(b.bytes()) + 977u * uint32_t(p.tab.size())));
    return 0;
}

bool same_class(const RegionsClass& a, const RegionsClass& b) {
    return a.first == b.first && a.sub.frames == b.sub.frames && a.sub.w == b.sub.w && a.sub.h == b.sub.h && a.sub.n_slices == b.sub.n_slices &&
           a.sub.tile_w == b.sub.tile_w && a.sub.tile_h == b.sub.tile_h && a.sub.flags == b.sub.flags && a.sub.lane_shift == b.sub.lane_shift &&
           a.sub.lpw == b.sub.lpw && a.sub.slice_cap == b.sub.slice_cap;
}

}  // namespace

int main() {
    const uint32_t shapes[][5] = {{97, 24, 32, 1, 3}, {70, 41, 40, 8, 4}, {33, 17, 16, 4, 2}, {300, 200, 64, 64, 3}, {40, 40, 0, 0, 1}};
    const Tuning tune{};
    const float mean[4] = {0.485f, 0.456f, 0.406f, 0.5f}, sd[4] = {0.229f, 0.224f, 0.225f, 0.25f};
    const llcomp_mi_output_format f32chw = {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F32, LLCOMP_MI_LAYOUT_CHW, 1, mean, sd};
    void* const d_out = reinterpret_cast<void*>(uintptr_t(0x10000));  // (an address the planner checks and never follows)
    uint32_t rounds = 0;
    for (const auto& sh : shapes) {
        const uint32_t w = sh[0], h = sh[1], tw = sh[2], th = sh[3], c = sh[4];
        for (int round = 0; round < 160; ++round) {
            const uint32_t frames = pick(1, 6), mode = uint32_t(round) % 4;
            Geometry g;
            CHECK(make_geometry(g, frames, w, h, c, tw, th, 1, tune));
            uint8_t fill[4] = {uint8_t(pick(0, 255)), uint8_t(pick(0, 255)), uint8_t(pick(0, 255)), uint8_t(pick(0, 255))};
            if (round % 8 >= 4) std::memset(fill, 0, sizeof fill);
            const llcomp_mi_pad pad{uint32_t(sizeof(llcomp_mi_pad)), mode, round % 16 >= 12 ? nullptr : fill};
            const bool with_bias = mode == LLCOMP_MI_PAD_CONSTANT && pad.fill && std::any_of(fill, fill + c, [](uint8_t v) { return v != 0; });
            const llcomp_mi_output_format* fmt = round % 3 == 0 ? &f32chw : nullptr;

            // ---- 1. a padded resized plan -----------------------------------------------------------------------------------------
            std::vector<int32_t> rects(4 * frames);
            std::vector<uint8_t> flags(frames);
            // (outputs no larger than the image and no smaller than 3/16 of it: r <= 3 n stays within Lanczos' 64 / 3)
            const uint32_t ow = pick((3 * w + 15) / 16 + 1, w), oh = pick((3 * h + 15) / 16 + 1, h);
            for (uint32_t f = 0; f < frames; ++f) {
                pick_axis(mode, w, rects[4 * f], rects[4 * f + 2]);
                pick_axis(mode, h, rects[4 * f + 1], rects[4 * f + 3]);
                flags[f] = uint8_t(pick(0, 1) | LLCOMP_MI_FLAG_FILTER(round % 5 == 0 ? uint32_t(LLCOMP_MI_FILTER_LANCZOS) : pick(0, 5)));
            }
            std::vector<uint32_t> src(4 * frames, 0xFFFFFFFFu);
            CHECK(llcomp_mi_padded_regions_plan(w, h, rects.data(), frames, &pad, src.data()) == LLCOMP_MI_OK);
            for (uint32_t f = 0; f < frames; ++f) {
                const uint32_t* s = src.data() + 4 * f;
                CHECK(s[2] >= 1 && s[3] >= 1 && uint64_t(s[0]) + s[2] <= w && uint64_t(s[1]) + s[3] <= h);
                if (rects[4 * f] >= 0 && rects[4 * f] + rects[4 * f + 2] <= int32_t(w)) CHECK(int32_t(s[0]) == rects[4 * f] && int32_t(s[2]) == rects[4 * f + 2]);
            }
            ResizedPlan pp;
            std::vector<uint32_t> planned;
            CHECK(padded_setup(g, tune, rects.data(), flags.data(), ow, oh, &pad, fmt, d_out, pp, planned) == LLCOMP_MI_OK);
            CHECK(planned == src);
            // the windows: the unpadded plan's for the source rectangles, and llcomp_mi_resized_regions_plan's
            std::vector<uint8_t> bilinear(frames, 0);  // (the source rectangle may be too small a downscale for no filter: the limit is r -> out's)
            ResizedPlan up;
            CHECK(resized_setup(g, tune, src.data(), bilinear.data(), ow, oh, fmt, d_out, up) == LLCOMP_MI_OK);
            CHECK(pp.wmax == up.wmax && pp.hmax == up.hmax && pp.n_classes == up.n_classes && pp.tab.size() == up.tab.size());
            CHECK(std::memcmp(pp.tab.data(), up.tab.data(), up.tab.size() * sizeof(RegionsFrame)) == 0);
            for (uint32_t i = 0; i < up.n_classes; ++i) CHECK(same_class(pp.classes[i], up.classes[i]));
            std::vector<uint32_t> windows(4 * frames);
            uint32_t n_classes = 0;
            CHECK(llcomp_mi_resized_regions_plan(w, h, c, tw, th, 1, src.data(), frames, windows.data(), &n_classes) == LLCOMP_MI_OK);
            CHECK(n_classes == pp.n_classes);
            for (const RegionsFrame& e : pp.tab) CHECK(e.wx0 == windows[4 * e.frame] && e.wy0 == windows[4 * e.frame + 1]);
            CHECK(pp.tail.box_bytes == up.tail.box_bytes && pp.tail.mid_bytes == up.tail.mid_bytes);
            for (uint32_t f = 0; f < frames; ++f) {
                const ResizeFrame &a = pp.tail.block.rs[f], &b = up.tail.block.rs[f];
                CHECK(a.ox == b.ox && a.oy == b.oy && a.rw == b.rw && a.rh == b.rh && a.box == b.box && a.rw == src[4 * f + 2] && a.rh == src[4 * f + 3]);
            }
            if (check_block(g, pp, pp.tail, frames, with_bias, fill, padded_tables_bound(g, frames))) return 1;
            // the largest tables there are: every frame another Lanczos rectangle at the pad limit on both axes, to the image's own size
            {
                std::vector<int32_t> big(4 * frames);
                std::vector<uint8_t> lz(frames, uint8_t(LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_LANCZOS)));
                for (uint32_t f = 0; f < frames; ++f) {
                    const int32_t lx = int32_t(limit_of(mode, w)) - int32_t(f % w), ly = int32_t(limit_of(mode, h)) - int32_t(f % h);
                    big[4 * f] = -lx;
                    big[4 * f + 1] = -ly;
                    big[4 * f + 2] = int32_t(w) + 2 * lx;
                    big[4 * f + 3] = int32_t(h) + 2 * ly;
                }
                ResizedPlan bp;
                std::vector<uint32_t> bsrc;
                CHECK(padded_setup(g, tune, big.data(), lz.data(), w, h, &pad, &f32chw, d_out, bp, bsrc) == LLCOMP_MI_OK);
                if (check_block(g, bp, bp.tail, frames, with_bias, fill, padded_tables_bound(g, frames))) return 1;
            }

            // ---- 2. a padded views plan: the unions are the bounding boxes of the views' source rectangles ---------------------------------
            {
                const uint32_t n_groups = pick(1, 3);
                std::vector<std::vector<llcomp_mi_view>> views(n_groups), sviews(n_groups);
                std::vector<llcomp_mi_view_group> groups(n_groups), sgroups(n_groups);
                std::vector<uint32_t> x0(frames, 0xFFFFFFFFu), y0(frames, 0xFFFFFFFFu), x1(frames, 0), y1(frames, 0);
                uint64_t total = 0;
                for (uint32_t gi = 0; gi < n_groups; ++gi) {
                    const uint32_t n = pick(1, 5);
                    for (uint32_t i = 0; i < n; ++i) {
                        int32_t r[4];
                        pick_axis(mode, w, r[0], r[2]);
                        pick_axis(mode, h, r[1], r[3]);
                        const uint32_t f = pick(0, frames - 1);
                        views[gi].push_back(llcomp_mi_view{f, uint32_t(r[0]), uint32_t(r[1]), uint32_t(r[2]), uint32_t(r[3]),
                                                           pick(0, 1) | LLCOMP_MI_FLAG_FILTER(pick(0, 5))});
                        uint32_t s[4];
                        CHECK(llcomp_mi_padded_regions_plan(w, h, r, 1, &pad, s) == LLCOMP_MI_OK);
                        sviews[gi].push_back(llcomp_mi_view{f, s[0], s[1], s[2], s[3], 0});
                        x0[f] = std::min(x0[f], s[0]);
                        y0[f] = std::min(y0[f], s[1]);
                        x1[f] = std::max(x1[f], s[0] + s[2]);
                        y1[f] = std::max(y1[f], s[1] + s[3]);
                    }
                    total += n;
                    const uint32_t gw = pick((3 * w + 15) / 16 + 1, w), gh = pick((3 * h + 15) / 16 + 1, h);
                    groups[gi] = llcomp_mi_view_group{uint32_t(sizeof(llcomp_mi_view_group)), n, views[gi].data(), gw, gh, (round + gi) % 2 ? &f32chw : nullptr, d_out};
                    sgroups[gi] = groups[gi];
                    sgroups[gi].views = sviews[gi].data();
                }
                ViewsPlan vp;
                CHECK(padded_views_setup(g, tune, groups.data(), n_groups, &pad, vp) == LLCOMP_MI_OK);
                uint32_t n_used = 0;
                for (uint32_t f = 0; f < frames; ++f) {
                    const uint32_t* u = vp.u.rects.data() + 4 * f;
                    if (!x1[f]) {
                        CHECK(!u[0] && !u[1] && !u[2] && !u[3]);
                        continue;
                    }
                    CHECK(vp.u.used[n_used++] == f);
                    CHECK(u[0] == x0[f] && u[1] == y0[f] && u[2] == x1[f] - x0[f] && u[3] == y1[f] - y0[f]);
                }
                CHECK(n_used == vp.u.used.size() && vp.tab.size() == n_used && vp.u.total_views == total && vp.tail.block.rs.size() == total);
                // ... and what llcomp_mi_views_plan says of the source rectangles
                std::vector<uint32_t> unions(4 * frames), wins(4 * frames);
                uint32_t used = 0, classes = 0;
                CHECK(llcomp_mi_views_plan(w, h, c, tw, th, 1, frames, sgroups.data(), n_groups, unions.data(), wins.data(), &used, &classes) == LLCOMP_MI_OK);
                CHECK(used == n_used && classes == vp.n_classes && std::memcmp(unions.data(), vp.u.rects.data(), 16 * size_t(frames)) == 0);
                for (const RegionsFrame& e : vp.tab) CHECK(e.wx0 == wins[4 * e.frame] && e.wy0 == wins[4 * e.frame + 1] && vp.u.used[e.out] == e.frame);
                if (check_block(g, vp, vp.tail, n_used, with_bias, fill, padded_tables_bound(g, total))) return 1;
            }

            // ---- 3. refusals ---------------------------------------------------------------------------------------------------------
            {
                const uint32_t bad = pick(0, frames - 1);
                auto resized = [&](const std::vector<int32_t>& r, const llcomp_mi_pad* pd, uint32_t ow_, uint32_t oh_, const std::vector<uint8_t>& fl) {
                    ResizedPlan p;
                    std::vector<uint32_t> s;
                    return padded_setup(g, tune, r.data(), fl.data(), ow_, oh_, pd, fmt, d_out, p, s);
                };
                auto viewed = [&](const std::vector<int32_t>& r, const llcomp_mi_pad* pd, uint32_t ow_, uint32_t oh_, const std::vector<uint8_t>& fl,
                                  uint32_t struct_size) {
                    std::vector<llcomp_mi_view> views(frames);
                    for (uint32_t f = 0; f < frames; ++f)
                        views[f] = llcomp_mi_view{f, uint32_t(r[4 * f]), uint32_t(r[4 * f + 1]), uint32_t(r[4 * f + 2]), uint32_t(r[4 * f + 3]), fl[f]};
                    const llcomp_mi_view_group gr{struct_size, frames, views.data(), ow_, oh_, fmt, d_out};
                    ViewsPlan p;
                    return padded_views_setup(g, tune, &gr, 1, pd, p);
                };
                const uint32_t gs = uint32_t(sizeof(llcomp_mi_view_group));
                auto both_refuse = [&](const std::vector<int32_t>& r, const llcomp_mi_pad* pd, uint32_t ow_, uint32_t oh_, const std::vector<uint8_t>& fl) {
                    return resized(r, pd, ow_, oh_, fl) == LLCOMP_MI_BAD_ARGS && viewed(r, pd, ow_, oh_, fl, gs) == LLCOMP_MI_BAD_ARGS;
                };
                CHECK(resized(rects, &pad, ow, oh, flags) == LLCOMP_MI_OK && viewed(rects, &pad, ow, oh, flags, gs) == LLCOMP_MI_OK);
                CHECK(viewed(rects, &pad, ow, oh, flags, gs + 8) == LLCOMP_MI_BAD_ARGS);  // a view group of another struct_size
                CHECK(both_refuse(rects, nullptr, ow, oh, flags));                         // no pad
                llcomp_mi_pad pd = pad;
                pd.struct_size = uint32_t(sizeof(llcomp_mi_pad)) - 1;
                CHECK(both_refuse(rects, &pd, ow, oh, flags));
                pd = pad;
                pd.mode = 4;
                CHECK(both_refuse(rects, &pd, ow, oh, flags));
                const int32_t lx = int32_t(limit_of(mode, w)), ly = int32_t(limit_of(mode, h));
                std::vector<int32_t> r = rects;  // a pad above the limit: left, right, top, bottom
                r[4 * bad] = -lx - 1;
                r[4 * bad + 2] = lx + 2;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;
                r[4 * bad] = 0;
                r[4 * bad + 2] = int32_t(w) + lx + 1;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;
                r[4 * bad + 1] = -ly - 1;
                r[4 * bad + 3] = ly + 2;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;
                r[4 * bad + 1] = int32_t(h) - 1;
                r[4 * bad + 3] = ly + 2;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;  // no image pixel: wholly left of the image, starting at its right edge, wholly above, starting at the bottom
                r[4 * bad] = -3;
                r[4 * bad + 2] = 3;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r[4 * bad] = int32_t(w);
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;
                r[4 * bad + 1] = int32_t(h);
                r[4 * bad + 3] = 1;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r = rects;  // an empty and a negative size
                r[4 * bad + 2 + round % 2] = 0;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                r[4 * bad + 2 + round % 2] = -5;
                CHECK(both_refuse(r, &pad, ow, oh, flags));
                CHECK(both_refuse(rects, &pad, 0, oh, flags) && both_refuse(rects, &pad, ow, 0, flags));  // an output side of 0
                std::vector<uint8_t> fl = flags;
                fl[bad] = uint8_t(LLCOMP_MI_FLAG_FILTER(6) | 1);
                CHECK(both_refuse(rects, &pad, ow, oh, fl));
                // the downscale limit is r -> out's, not the source interval's: Lanczos on 3 sides' worth of rectangle into 1/8 of a side
                if (mode != LLCOMP_MI_PAD_REFLECT && w >= 32) {
                    fl = flags;
                    fl[bad] = uint8_t(LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_LANCZOS));
                    r = rects;
                    r[4 * bad] = -int32_t(w);
                    r[4 * bad + 2] = 3 * int32_t(w);
                    CHECK(both_refuse(r, &pad, w / 8, oh, fl));
                    CHECK(resized(r, &pad, w, oh, fl) == LLCOMP_MI_OK);
                }
                uint32_t keep[4] = {7, 7, 7, 7};
                CHECK(llcomp_mi_padded_regions_plan(w, h, rects.data(), 0, &pad, keep) == LLCOMP_MI_BAD_ARGS);
                CHECK(llcomp_mi_padded_regions_plan(w, h, nullptr, 1, &pad, keep) == LLCOMP_MI_BAD_ARGS);
                CHECK(llcomp_mi_padded_regions_plan(w, h, rects.data(), 1, &pad, nullptr) == LLCOMP_MI_BAD_ARGS);
                CHECK(llcomp_mi_padded_regions_plan(w, h, r.data() + 4 * bad, 1, nullptr, keep) == LLCOMP_MI_BAD_ARGS);
                CHECK(keep[0] == 7 && keep[3] == 7);
            }
            ++rounds;
        }
    }
    std::printf("ok %u\n", rounds);
    return 0;
}
