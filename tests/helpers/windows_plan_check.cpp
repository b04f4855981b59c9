// windows_plan_check.cpp -- the host planner of the windowed decodes (llcomp_amd/csrc/windows_plan.hpp) under a sanitizer: the regions,
// resized and views plans over seeded random rectangles, the layout of the call's one copy (the block is put into a heap buffer of
// exactly its size, so a write past it is seen) against the bounds the codec sizes its buffers by, a resized plan against the views plan
// of one view per frame, and the refusals.  Host code only; built and run by tests/test_windows_plan.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/windows_plan_check.cpp llcomp_amd/csrc/container.cpp llcomp_amd/csrc/windows_plan.cpp llcomp_amd/csrc/resize_plan.cpp
//       llcomp_amd/csrc/photo_plan.cpp
// Prints "ok <rounds>".
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

// every entry's crop of bw x bh inside its class's sub-image, out / frame in range, and the classes' entries tiling the table
int check_windows(const Geometry& g, const WindowsPlan& p, uint32_t outs) {
    CHECK(p.n_classes >= 1 && p.n_classes <= kRegionsClasses);
    uint32_t next = 0;
    for (uint32_t i = 0; i < p.n_classes; ++i) {
        const RegionsClass& rc = p.classes[i];
        CHECK(rc.first == next && rc.sub.frames >= 1);
        next += rc.sub.frames;
        CHECK(next <= p.tab.size());
        for (uint32_t j = 0; j < rc.sub.frames; ++j) {
            const RegionsFrame& e = p.tab[rc.first + j];
            CHECK(uint64_t(e.cx0) + p.wmax <= rc.sub.w && uint64_t(e.cy0) + p.hmax <= rc.sub.h);
            CHECK(e.out < outs && e.frame < g.frames);
        }
    }
    CHECK(next == p.tab.size());
    return 0;
}

// every entry's rectangle inside its box; the copy's offsets; the block put into exactly bytes() bytes; the total against `bound`
// (0: no bound holds, an output larger than the image) for the most a gather over the plan's windows can stage
int check_tail(const Geometry& g, const WindowsPlan& p, const ResampleTail& t, uint32_t boxes, uint64_t bound, std::mt19937& rng) {
    const ResampleBlock& b = t.block;
    for (const ResizeFrame& z : b.rs) CHECK(uint64_t(z.ox) + z.rw <= p.wmax && uint64_t(z.oy) + z.rh <= p.hmax && z.box < boxes);
    uint64_t entries = 0;
    for (const ResampleGroup& vg : t.groups) {
        CHECK(vg.first == entries && vg.chunk >= 1 && vg.chunk <= vg.n);
        entries += vg.n;
        CHECK(uint64_t(vg.chunk) * vg.mh * vg.ow * g.c <= t.mid_bytes);
        for (uint32_t i = 0; i < vg.n; ++i) {
            const ResizeFrame& z = b.rs[vg.first + i];
            CHECK(z.rh <= vg.mh && z.kx && z.ky);
            CHECK(uint64_t(z.hx) + uint64_t(vg.ow) * (z.kx + 1) <= b.w.size() && uint64_t(z.vy) + uint64_t(vg.oh) * (z.ky + 1) <= b.w.size());
        }
        if (!vg.out.plain) CHECK(vg.table_at % 16 == 0 && vg.table_at + vg.out.table_bytes(g.c) <= b.tables.size());
    }
    CHECK(entries == b.rs.size());
    CHECK(t.box_bytes == uint64_t(boxes) * p.wmax * p.hmax * g.c);
    std::unique_ptr<uint8_t[]> heap(new uint8_t[b.bytes()]);
    b.put(heap.get());
    CHECK(b.tables.empty() || std::memcmp(heap.get() + b.tables_at(), b.tables.data(), b.tables.size()) == 0);
    // a gather of the classes' slices: any payload up to the entry limit of every slice, now and then the limit itself
    RegionsGather gp;
    for (uint32_t i = 0; i < p.n_classes; ++i) gp.n_slices += p.classes[i].sub.n_slices;
    CHECK(gp.n_slices <= g.n_slices);
    const uint64_t most = uint64_t(gp.n_slices) * (g.slice_cap - 16);
    gp.payload_bytes = rng() % 4 == 0 ? most : rng() % (most + 1);
    for (const RegionsGather* src : {static_cast<const RegionsGather*>(nullptr), static_cast<const RegionsGather*>(&gp)}) {
        const CopyLayout cl(p.tab.size(), src, &t);
        CHECK(cl.stage.len_at == p.tab.size() * sizeof(RegionsFrame) && cl.stage.off_at % 8 == 0 && cl.rs_at % 16 == 0);
        CHECK(cl.stage.off_at >= cl.stage.len_at + 4 * uint64_t(src ? gp.n_slices : 0) && cl.rs_at >= cl.stage.bytes);
        CHECK((cl.rs_at + b.w_at()) % 4 == 0 && (b.tables.empty() || (cl.rs_at + b.tables_at()) % 16 == 0));
        CHECK(cl.bytes == cl.rs_at + b.bytes());
        if (bound) CHECK(cl.bytes <= stage_bound(g) + bound);
    }
    // ... and with photometric chains behind the block, as a photo views call lays them (one chain per view at the most)
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
    std::mt19937 rng(20241018);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    const uint32_t shapes[][4] = {{300, 200, 64, 64}, {1100, 24, 480, 1}, {160, 41, 40, 2}, {97, 61, 0, 0}, {32, 32, 12, 10}};
    const uint32_t c = 3;
    const Tuning tune{};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const llcomp_mi_output_format formats[2] = {
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F32, LLCOMP_MI_LAYOUT_CHW, 1, mean, sd},
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_HWC, 0, nullptr, nullptr}};
    void* const d_out = reinterpret_cast<void*>(uintptr_t(0x10000));  // (an address the planner checks and never follows)
    uint32_t rounds = 0;
    for (const auto& sh : shapes) {
        const uint32_t w = sh[0], h = sh[1], tw = sh[2], th = sh[3];
        for (int round = 0; round < 200; ++round) {
            const uint32_t frames = pick(1, 6);
            Geometry g;
            CHECK(make_geometry(g, frames, w, h, c, tw, th, 1, tune));

            // ---- 1. a regions plan: one size, an origin per frame -----------------------------------------------------------------
            {
                WindowsPlan p;
                p.wmax = pick(1, w);
                p.hmax = pick(1, h);
                std::vector<uint32_t> xy(2 * frames);
                for (uint32_t f = 0; f < frames; ++f) {
                    xy[2 * f] = round % 4 == 0 ? w - p.wmax : pick(0, w - p.wmax);  // (every fourth round: all at the right edge)
                    xy[2 * f + 1] = pick(0, h - p.hmax);
                }
                p.tab.resize(frames);
                CHECK(regions_setup(g, tune, xy.data(), p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes) == LLCOMP_MI_OK);
                if (check_windows(g, p, frames)) return 1;
                for (const RegionsFrame& e : p.tab) CHECK(e.out == e.frame);
                const CopyLayout cl(p.tab.size(), nullptr, nullptr);
                CHECK(cl.bytes == frames * sizeof(RegionsFrame));
                const uint64_t no_tables = 0;  // (a call without a tail adds nothing to stage_bound)
                CHECK(copy_layout_ok(g, p, false, 0, 0, &no_tables, 131u * p.wmax + p.hmax));
            }

            // ---- 2. a resized plan: a rectangle, a mirror bit and a filter per frame; outputs below and above the image's size -----------
            // (no side below 3/64 of the image's: no filter's downscale limit is met)
            const bool larger = round % 5 == 4;
            const uint32_t ow = larger ? pick(w, w + 40) : pick((3 * w + 63) / 64, w), oh = larger ? pick(h, h + 40) : pick((3 * h + 63) / 64, h);
            const llcomp_mi_output_format* fmt = round % 3 == 0 ? nullptr : &formats[round % 3 - 1];
            std::vector<uint32_t> rects(4 * frames);
            std::vector<uint8_t> flags(frames);
            for (uint32_t f = 0; f < frames; ++f) {
                uint32_t* r = rects.data() + 4 * f;
                r[2] = pick(1, w);
                r[3] = pick(1, h);
                r[0] = pick(0, w - r[2]);
                r[1] = pick(0, h - r[3]);
                flags[f] = uint8_t(pick(0, 1) | LLCOMP_MI_FLAG_FILTER(pick(0, 5)));
            }
            ResizedPlan rp;
            CHECK(resized_setup(g, tune, rects.data(), flags.data(), ow, oh, fmt, d_out, rp) == LLCOMP_MI_OK);
            if (check_windows(g, rp, frames)) return 1;
            CHECK(rp.tail.groups.size() == 1 && rp.tail.groups[0].n == frames && rp.tail.groups[0].chunk == frames && rp.tail.groups[0].table_at == 0);
            CHECK(rp.tail.groups[0].mh == rp.hmax && rp.tail.mid_bytes == uint64_t(frames) * rp.hmax * ow * c && rp.tail.groups[0].d_out == d_out);
            if (check_tail(g, rp, rp.tail, frames, larger ? 0 : resized_tables_bound(g), rng)) return 1;

            // ---- 3. ... equals the views plan of one group with one view per frame ------------------------------------------------
            {
                std::vector<llcomp_mi_view> views(frames);
                for (uint32_t f = 0; f < frames; ++f)
                    views[f] = llcomp_mi_view{f, rects[4 * f], rects[4 * f + 1], rects[4 * f + 2], rects[4 * f + 3], flags[f]};
                const llcomp_mi_view_group gr{uint32_t(sizeof(llcomp_mi_view_group)), frames, views.data(), ow, oh, fmt, d_out};
                ViewsPlan vp;
                CHECK(views_setup(g, tune, &gr, 1, vp) == LLCOMP_MI_OK);
                CHECK(vp.wmax == rp.wmax && vp.hmax == rp.hmax && vp.n_classes == rp.n_classes && vp.tab.size() == rp.tab.size());
                CHECK(std::memcmp(vp.tab.data(), rp.tab.data(), rp.tab.size() * sizeof(RegionsFrame)) == 0);
                for (uint32_t i = 0; i < rp.n_classes; ++i) CHECK(same_class(vp.classes[i], rp.classes[i]));
                const ResampleBlock &a = rp.tail.block, &b = vp.tail.block;
                CHECK(a.rs.size() == frames && b.rs.size() == frames);
                for (uint32_t f = 0; f < frames; ++f) {
                    ResizeFrame x = a.rs[f], y = b.rs[f];
                    // (the two plans append weights in different orders -- table order and view order: contents, not offsets)
                    CHECK(x.kx == y.kx && std::memcmp(a.w.data() + x.hx, b.w.data() + y.hx, 4 * size_t(ow) * (x.kx + 1)) == 0);
                    CHECK(x.ky == y.ky && std::memcmp(a.w.data() + x.vy, b.w.data() + y.vy, 4 * size_t(oh) * (x.ky + 1)) == 0);
                    x.hx = x.vy = y.hx = y.vy = 0;
                    CHECK(std::memcmp(&x, &y, sizeof(ResizeFrame)) == 0);
                }
                CHECK(a.tables == b.tables && vp.tail.groups[0].table_at == 0 && vp.tail.box_bytes == rp.tail.box_bytes);
                CHECK(vp.tail.groups[0].mh == rp.hmax);
            }

            // ---- 4. a views plan: two or three groups, a frame list with gaps every third round -----------------------------------------
            {
                const uint32_t n_groups = pick(2, 3);
                std::vector<std::vector<llcomp_mi_view>> views(n_groups);
                std::vector<llcomp_mi_view_group> groups(n_groups);
                uint64_t total = 0;
                bool small = true;
                for (uint32_t gi = 0; gi < n_groups; ++gi) {
                    const uint32_t n = pick(1, 5);
                    for (uint32_t i = 0; i < n; ++i) {
                        llcomp_mi_view v;
                        v.frame = round % 3 == 0 ? pick(0, frames - 1) / 2 * 2 % frames : pick(0, frames - 1);
                        v.rw = pick(1, w);
                        v.rh = pick(1, h);
                        v.x = pick(0, w - v.rw);
                        v.y = pick(0, h - v.rh);
                        v.flags = pick(0, 1) | LLCOMP_MI_FLAG_FILTER(pick(0, 5));
                        views[gi].push_back(v);
                    }
                    total += n;
                    const uint32_t gw = larger && gi == 0 ? w + pick(1, 40) : pick((3 * w + 63) / 64, w), gh = pick((3 * h + 63) / 64, h);
                    small = small && gw <= w;
                    groups[gi] = llcomp_mi_view_group{uint32_t(sizeof(llcomp_mi_view_group)), n, views[gi].data(), gw, gh,
                                                      (round + gi) % 3 == 0 ? nullptr : &formats[(round + gi) % 3 - 1], d_out};
                }
                ViewsPlan vp;
                CHECK(views_setup(g, tune, groups.data(), n_groups, vp) == LLCOMP_MI_OK);
                const uint32_t n_used = uint32_t(vp.u.used.size());
                CHECK(vp.tab.size() == n_used && vp.u.total_views == total && vp.tail.block.rs.size() == total && vp.tail.groups.size() == n_groups);
                if (check_windows(g, vp, n_used)) return 1;
                for (const RegionsFrame& e : vp.tab) CHECK(vp.u.used[e.out] == e.frame);
                if (check_tail(g, vp, vp.tail, n_used, small ? views_tables_bound(g, total) : 0, rng)) return 1;
            }

            // ---- 5. refusals, each with the status the calls have always given; a refused plan is not looked at -----------------------
            {
                const uint32_t bad = pick(0, frames - 1);
                auto resized = [&](const std::vector<uint32_t>& r, const std::vector<uint8_t>& fl, uint32_t ow_, uint32_t oh_) {
                    ResizedPlan p;
                    return resized_setup(g, tune, r.data(), fl.data(), ow_, oh_, fmt, d_out, p);
                };
                auto viewed = [&](const std::vector<uint32_t>& r, const std::vector<uint8_t>& fl, uint32_t ow_, uint32_t oh_, uint32_t frame_of_bad) {
                    std::vector<llcomp_mi_view> views(frames);
                    for (uint32_t f = 0; f < frames; ++f)
                        views[f] = llcomp_mi_view{f == bad ? frame_of_bad : f, r[4 * f], r[4 * f + 1], r[4 * f + 2], r[4 * f + 3], fl[f]};
                    const llcomp_mi_view_group gr{uint32_t(sizeof(llcomp_mi_view_group)), frames, views.data(), ow_, oh_, fmt, d_out};
                    ViewsPlan p;
                    return views_setup(g, tune, &gr, 1, p);
                };
                auto plain = [&](const std::vector<uint32_t>& r) {  // (the bad frame's size for every frame)
                    std::vector<uint32_t> xy(2 * frames);
                    for (uint32_t f = 0; f < frames; ++f) {
                        xy[2 * f] = f == bad ? r[4 * f] : 0;
                        xy[2 * f + 1] = f == bad ? r[4 * f + 1] : 0;
                    }
                    std::vector<RegionsFrame> tab(frames);
                    RegionsClass classes[kRegionsClasses];
                    uint32_t n = 0;
                    return regions_setup(g, tune, xy.data(), r[4 * bad + 2], r[4 * bad + 3], tab.data(), classes, n);
                };
                std::vector<uint32_t> r = rects;
                std::vector<uint8_t> fl = flags;
                // a rectangle outside the image: past the right edge, past the bottom edge
                r[4 * bad] = w - r[4 * bad + 2] + 1;
                CHECK(resized(r, fl, ow, oh) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, ow, oh, bad) == LLCOMP_MI_BAD_ARGS && plain(r) == LLCOMP_MI_BAD_ARGS);
                r = rects;
                r[4 * bad + 1] = h - r[4 * bad + 3] + 1;
                CHECK(resized(r, fl, ow, oh) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, ow, oh, bad) == LLCOMP_MI_BAD_ARGS && plain(r) == LLCOMP_MI_BAD_ARGS);
                // an empty rectangle
                r = rects;
                r[4 * bad + 2 + round % 2] = 0;
                CHECK(resized(r, fl, ow, oh) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, ow, oh, bad) == LLCOMP_MI_BAD_ARGS && plain(r) == LLCOMP_MI_BAD_ARGS);
                // an output side of 0
                r = rects;
                CHECK(resized(r, fl, 0, oh) == LLCOMP_MI_BAD_ARGS && resized(r, fl, ow, 0) == LLCOMP_MI_BAD_ARGS);
                CHECK(viewed(r, fl, 0, oh, bad) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, ow, 0, bad) == LLCOMP_MI_BAD_ARGS);
                // a filter code of 6
                fl[bad] = uint8_t(LLCOMP_MI_FLAG_FILTER(6) | 1);
                CHECK(resized(r, fl, ow, oh) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, ow, oh, bad) == LLCOMP_MI_BAD_ARGS);
                // a downscale above the filter's limit: Lanczos takes 64 / 3 at the most, and every shape is at least 32 wide and high
                fl = flags;
                fl[bad] = uint8_t(LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_LANCZOS));
                r[4 * bad] = r[4 * bad + 1] = 0;
                r[4 * bad + 2] = w;
                r[4 * bad + 3] = h;
                CHECK(resized(r, fl, 1, h) == LLCOMP_MI_BAD_ARGS && resized(r, fl, w, 1) == LLCOMP_MI_BAD_ARGS);
                CHECK(viewed(r, fl, 1, h, bad) == LLCOMP_MI_BAD_ARGS && viewed(r, fl, w, 1, bad) == LLCOMP_MI_BAD_ARGS);
                CHECK(resized(r, fl, w, h) == LLCOMP_MI_OK && viewed(r, fl, w, h, bad) == LLCOMP_MI_OK);
                // a view of a frame the batch does not have, and a frame list that names one
                CHECK(viewed(rects, flags, ow, oh, frames) == LLCOMP_MI_BAD_ARGS);
                std::vector<uint32_t> used(frames);
                for (uint32_t f = 0; f < frames; ++f) used[f] = f;
                used[bad] = frames + pick(0, 2);
                std::vector<RegionsFrame> tab(frames);
                RegionsClass classes[kRegionsClasses];
                uint32_t n = 0;
                CHECK(regions_setup_sized(g, tune, rects.data(), rp.wmax, rp.hmax, tab.data(), classes, n, used.data(), frames) == LLCOMP_MI_BAD_ARGS);
                used[bad] = bad;
                CHECK(regions_setup_sized(g, tune, rects.data(), rp.wmax, rp.hmax, tab.data(), classes, n, used.data(), frames) == LLCOMP_MI_OK);
            }
            ++rounds;
        }
    }
    std::printf("ok %u\n", rounds);
    return 0;
}
