// perspective_plan_check.cpp -- the host planner of the perspective views (llcomp_amd/csrc/warp_plan.hpp: persp_source_rect, persp_setup,
// WarpTail::put) and the rule's host functions (warp_rule.hpp, llcomp_mi_perspective_reference) under a sanitizer, on degenerate
// inputs: 1 x 1 outputs, calls whose views are all empty, a group of 65535 views, coefficients at the limits -- and seeded random
// keystones in between.  Every entry's source rectangle inside its frame's box, the block put into a heap buffer of exactly its size
// and within the bound the staging buffer is sized by, the reference with image and output in heap buffers of exactly their sizes,
// every pixel the rule reads inside the source rectangle.  Host code only; built and run by tests/test_perspective_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/perspective_plan_check.cpp llcomp_amd/csrc/container.cpp llcomp_amd/csrc/windows_plan.cpp
//       llcomp_amd/csrc/resize_plan.cpp llcomp_amd/csrc/warp_plan.cpp llcomp_amd/csrc/photo_plan.cpp
// Prints "ok <rounds>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "container.hpp"
#include "copy_layout_check.hpp"
#include "warp_plan.hpp"
#include "warp_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

namespace {

const uint32_t kFilters[3] = {LLCOMP_MI_FILTER_NEAREST, LLCOMP_MI_FILTER_BILINEAR, LLCOMP_MI_FILTER_BICUBIC};

// The reference on a heap image of exactly w * h * c bytes into a heap output of exactly ow * oh * c.  Then the source rectangle:
// inside the image, holding every pixel the rule reads for an output pixel inside, and empty exactly when there is none.
int check_reference(uint32_t w, uint32_t h, uint32_t c, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, std::mt19937& rng) {
    std::unique_ptr<uint8_t[]> img(new uint8_t[size_t(w) * h * c]);
    for (size_t i = 0; i < size_t(w) * h * c; ++i) img[i] = uint8_t(rng());
    uint8_t fill[8];
    for (uint8_t& f : fill) f = uint8_t(rng());
    std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(ow) * oh * c]);
    CHECK(llcomp_mi_perspective_reference(img.get(), w, h, c, a, filter, fill, ow, oh, out.get()) == LLCOMP_MI_OK);
    uint32_t rect[4], empty = 7;
    CHECK(llcomp_mi_perspective_source_rect(w, h, a, filter, ow, oh, rect, &empty) == LLCOMP_MI_OK && empty <= 1);
    if (!empty) CHECK(rect[2] && rect[3] && uint64_t(rect[0]) + rect[2] <= w && uint64_t(rect[1]) + rect[3] <= h);
    bool any = false;
    for (uint32_t y = 0; y < oh; ++y)
        for (uint32_t x = 0; x < ow; ++x) {
            double xin, yin;
            persp_xy(a, x, y, xin, yin);
            if (!warp_inside(xin, yin, w, h)) {
                for (uint32_t ch = 0; ch < c; ++ch) CHECK(out[(size_t(y) * ow + x) * c + ch] == fill[ch]);
                continue;
            }
            any = true;
            CHECK(!empty);
            if (filter == LLCOMP_MI_FILTER_NEAREST) {
                const int32_t xi = persp_index(xin, w), yi = persp_index(yin, h);
                CHECK(xi >= 0 && yi >= 0 && uint32_t(xi) >= rect[0] && uint32_t(xi) < rect[0] + rect[2] && uint32_t(yi) >= rect[1] &&
                      uint32_t(yi) < rect[1] + rect[3]);
                continue;
            }
            const WarpTap t = warp_tap(xin, yin);
            const int32_t lo = filter == LLCOMP_MI_FILTER_BICUBIC ? -1 : 0, hi = filter == LLCOMP_MI_FILTER_BICUBIC ? 2 : 1;
            for (int32_t d = lo; d <= hi; ++d) {
                const uint32_t col = uint32_t(warp_cl(t.X + d, int32_t(w))), row = uint32_t(warp_cl(t.Y + d, int32_t(h)));
                CHECK(col >= rect[0] && col < rect[0] + rect[2] && row >= rect[1] && row < rect[1] + rect[3]);
            }
        }
    CHECK(any == !empty);
    if (empty) CHECK(!rect[0] && !rect[1] && !rect[2] && !rect[3]);
    return 0;
}

int check_plan(const Geometry& g, const WarpPlan& p, const std::vector<llcomp_mi_perspective_group>& groups) {
    const WarpTail& t = p.tail;
    const uint32_t boxes = uint32_t(p.u.used.size());
    CHECK(p.tab.size() == boxes && t.groups.size() == groups.size() && t.ws.empty() && t.tabs.empty());
    CHECK(t.box_bytes == uint64_t(boxes) * p.wmax * p.hmax * g.c);
    uint64_t entries = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const WarpOut& vg = t.groups[gi];
        CHECK(vg.first == entries && vg.n == groups[gi].n_views && vg.ow == groups[gi].ow && vg.oh == groups[gi].oh);
        entries += vg.n;
        CHECK(uint64_t(vg.fill_at) + g.c <= t.fills.size());
        if (!vg.out.plain) CHECK(vg.table_at % 16 == 0 && vg.table_at + vg.out.table_bytes(g.c) <= t.tables.size());
        for (uint32_t i = 0; i < vg.n; ++i) {
            const PerspEntry& z = t.ps[vg.first + i];
            const llcomp_mi_perspective_view& v = groups[gi].views[i];
            const uint32_t filter = LLCOMP_MI_FLAG_FILTER_OF(z.flags & 0xFFu);
            CHECK((z.flags & 1u) == (v.flags & 1u) && filter == LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu));
            CHECK(std::memcmp(z.a, v.a, sizeof z.a) == 0);
            uint32_t rect[4];
            bool empty = false;
            CHECK(persp_source_rect(g.w, g.h, v.a, filter, vg.ow, vg.oh, rect, empty) == LLCOMP_MI_OK);
            CHECK(empty == ((z.flags & kPerspEmpty) != 0));
            if (empty) continue;
            CHECK(z.box < boxes && z.bx >= 0 && z.by >= 0 && uint64_t(z.bx) + p.wmax <= g.w && uint64_t(z.by) + p.hmax <= g.h);
            CHECK(p.u.used[z.box] == v.frame);
            CHECK(rect[0] >= uint32_t(z.bx) && rect[0] + rect[2] <= uint32_t(z.bx) + p.wmax && rect[1] >= uint32_t(z.by) &&
                  rect[1] + rect[3] <= uint32_t(z.by) + p.hmax);
        }
    }
    CHECK(entries == t.ps.size() && entries == p.total_views);
    std::unique_ptr<uint8_t[]> heap(new uint8_t[t.bytes()]);
    t.put(heap.get());
    CHECK(std::memcmp(heap.get(), t.ps.data(), t.ps.size() * sizeof(PerspEntry)) == 0);
    CHECK(std::memcmp(heap.get() + t.fills_at(), t.fills.data(), t.fills.size()) == 0);
    CHECK(t.tables.empty() || std::memcmp(heap.get() + t.tables_at(), t.tables.data(), t.tables.size()) == 0);
    CHECK(t.tabs_at() % 8 == 0 && (t.tables.empty() || t.tables_at() % 16 == 0));
    const uint64_t bound = persp_tables_bound(g, p.total_views);
    CHECK(t.bytes() + 16 <= bound);
    CHECK(copy_layout_ok(g, p, true, t.bytes(), p.total_views, &bound, uint32_t(t.bytes()) + 977u * uint32_t(p.tab.size())));
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20261020);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double(rng()) / 4294967296.0); };
    const uint32_t c = 3;
    const Tuning tune{};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const llcomp_mi_output_format formats[2] = {
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F32, LLCOMP_MI_LAYOUT_CHW, 1, mean, sd},
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_HWC, 0, nullptr, nullptr}};
    void* const d_out = reinterpret_cast<void*>(uintptr_t(0x10000));  // (an address the planner checks and never follows)
    const uint8_t fill[3] = {1, 2, 3};
    uint32_t rounds = 0;
    // kind 0, 1: a keystone around a scaled rotation; 2: the identity; 3: nothing inside; 4: a strong denominator
    auto random_map = [&](uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, uint32_t kind, double* a) {
        const double ang = real(-0.6, 0.6), sx = real(0.5, 1.5) * w / ow, sy = real(0.5, 1.5) * h / oh;
        a[0] = sx * std::cos(ang), a[1] = sx * std::sin(ang), a[2] = real(-0.3 * w, 0.5 * w);
        a[3] = -sy * std::sin(ang), a[4] = sy * std::cos(ang), a[5] = real(-0.3 * h, 0.5 * h);
        a[6] = real(-0.3, 0.6) / ow, a[7] = real(-0.3, 0.6) / oh;
        if (kind == 2) a[0] = a[4] = 1.0, a[1] = a[2] = a[3] = a[5] = a[6] = a[7] = 0.0;
        if (kind == 3) a[2] += 20.0 * w + 50.0;
        if (kind == 4) a[6] = real(1.0, 4.0) / ow, a[7] = real(-0.45, 3.0) / oh;
    };
    const uint32_t shapes[][4] = {{300, 200, 64, 64}, {97, 61, 0, 0}, {48, 40, 16, 16}, {48, 40, 16, 1}};
    for (const auto& sh : shapes) {
        const uint32_t w = sh[0], h = sh[1], tw = sh[2], th = sh[3];
        for (int round = 0; round < 100; ++round) {
            const uint32_t frames = pick(1, 5);
            Geometry g;
            CHECK(make_geometry(g, frames, w, h, c, tw, th, 1, tune));
            const uint32_t n_groups = pick(1, 3);
            std::vector<std::vector<llcomp_mi_perspective_view>> views(n_groups);
            std::vector<llcomp_mi_perspective_group> groups(n_groups);
            const bool all_empty = round % 13 == 0;
            for (uint32_t gi = 0; gi < n_groups; ++gi) {
                const bool tiny = round % 5 == 1;  // 1 x 1 outputs
                const uint32_t ow = tiny ? 1 : pick(1, w), oh = tiny ? 1 : pick(1, h);
                views[gi].resize(pick(1, 6));
                for (llcomp_mi_perspective_view& v : views[gi]) {
                    v.frame = pick(0, frames - 1);
                    v.flags = LLCOMP_MI_FLAG_FILTER(kFilters[rng() % 3]) | (rng() & 1u);
                    random_map(w, h, ow, oh, all_empty ? 3 : uint32_t(rng() % 5), v.a);
                }
                groups[gi] = llcomp_mi_perspective_group{uint32_t(sizeof(llcomp_mi_perspective_group)), uint32_t(views[gi].size()), views[gi].data(), ow, oh,
                                                         gi ? &formats[gi - 1] : nullptr, d_out, (rng() & 1) ? fill : nullptr};
            }
            WarpPlan p;
            CHECK(persp_setup(g, tune, groups.data(), n_groups, p) == LLCOMP_MI_OK);
            if (all_empty) CHECK(p.u.used.empty() && p.tab.empty() && !p.n_classes && !p.tail.box_bytes);
            if (check_plan(g, p, groups)) return 1;
            std::vector<uint32_t> uni(4 * frames, 9), win(4 * frames, 9);
            uint32_t used = 9, cls = 9;
            CHECK(llcomp_mi_perspective_views_plan(w, h, c, tw, th, 1, frames, groups.data(), n_groups, uni.data(), win.data(), &used, &cls) == LLCOMP_MI_OK);
            CHECK(used == p.u.used.size() && cls == p.n_classes && std::memcmp(uni.data(), p.u.rects.data(), 16 * frames) == 0);
            // a refusal in the middle of a call leaves nothing half done
            views[n_groups - 1].back().a[7] = std::numeric_limits<double>::quiet_NaN();
            WarpPlan q;
            CHECK(persp_setup(g, tune, groups.data(), n_groups, q) == LLCOMP_MI_BAD_ARGS);
            ++rounds;
        }
    }
    // 65535 views in one group (the most a group takes), every one a 1 x 1 output, half of them empty; and one view more
    {
        Geometry g;
        CHECK(make_geometry(g, 3, 48, 40, c, 16, 16, 1, tune));
        std::vector<llcomp_mi_perspective_view> views(65536);
        for (size_t i = 0; i < views.size(); ++i) {
            views[i].frame = uint32_t(i % 3);
            views[i].flags = LLCOMP_MI_FLAG_FILTER(kFilters[i % 3]) | uint32_t(i & 1);
            random_map(48, 40, 1, 1, i % 2 ? 3 : 0, views[i].a);
        }
        std::vector<llcomp_mi_perspective_group> groups(1, llcomp_mi_perspective_group{uint32_t(sizeof(llcomp_mi_perspective_group)), 65535, views.data(), 1,
                                                                                         1, &formats[1], d_out, fill});
        WarpPlan p;
        CHECK(persp_setup(g, tune, groups.data(), 1, p) == LLCOMP_MI_OK && p.total_views == 65535);
        if (check_plan(g, p, groups)) return 1;
        groups[0].n_views = 65536;
        WarpPlan q;
        CHECK(persp_setup(g, tune, groups.data(), 1, q) == LLCOMP_MI_BAD_ARGS);
        ++rounds;
    }
    // the reference and the source rectangle on the corner cases: 1 x 1 and 1 x N images and outputs, the identity, views wholly or half outside
    const uint32_t sides[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {13, 7}, {39, 31}};
    for (const auto& s : sides)
        for (uint32_t filter : kFilters)
            for (uint32_t kind = 0; kind < 5; ++kind)
                for (int rep = 0; rep < 8; ++rep) {
                    const uint32_t ow = rep == 0 ? 1 : pick(1, 24), oh = rep == 0 ? 1 : pick(1, 24);
                    double a[8];
                    random_map(s[0], s[1], ow, oh, kind, a);
                    for (uint32_t ch : {1u, 3u, 5u})
                        if (check_reference(s[0], s[1], ch, a, filter, ow, oh, rng)) return 1;
                    ++rounds;
                }
    // coefficients at the limits: just inside they plan and run, at them they are refused with the outputs untouched
    {
        uint32_t rect[4] = {7, 7, 7, 7}, empty = 7;
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity(), big = 1073741824.0;
        const double bad[][8] = {{nan, 0, 0, 0, 1, 0, 0, 0},      {1, 0, inf, 0, 1, 0, 0, 0},        {1, 0, 0, 0, 1, 0, -inf, 0},    {1, 0, 0, 0, 1, 0, 0, nan},
                                 {1e300, 0, 0, 0, 1, 0, 0, 0},    {1, 0, big, 0, 1, 0, 0, 0},        {1, 0, 0, 0, 1, -big - 8, 0, 0}, {1, 0, 0, 0, 1, 0, -0.125, -0.125},
                                 {1, 0, 0, 0, 1, 0, -2.0, 0},     {1, 0, 0, 0, 1, 0, 0, -1e300}};
        for (const auto& a : bad)
            for (uint32_t filter : kFilters) {
                CHECK(llcomp_mi_perspective_source_rect(20, 10, a, filter, 8, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
                CHECK(rect[0] == 7 && rect[3] == 7 && empty == 7);
            }
        const double ident[8] = {1, 0, 0, 0, 1, 0, 0, 0};
        CHECK(llcomp_mi_perspective_source_rect(20, 10, ident, LLCOMP_MI_FILTER_LANCZOS, 8, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
        CHECK(llcomp_mi_perspective_source_rect(20, 10, ident, LLCOMP_MI_FILTER_BILINEAR, 0, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
        CHECK(llcomp_mi_perspective_source_rect(20, 10, ident, LLCOMP_MI_FILTER_BILINEAR, 20, 10, rect, &empty) == LLCOMP_MI_OK);
        CHECK(rect[0] == 0 && rect[1] == 0 && rect[2] == 20 && rect[3] == 10 && empty == 0);
        // just below 2^30, and denominators of 2^-10 .. 2^-40 at the last corner (the small ones are planned pixel by pixel)
        const double edge[8] = {1, 0, std::nextafter(big, 0.0) - 8, 0, 1, 0, 0, 0};
        for (uint32_t filter : kFilters)
            if (check_reference(20, 10, 3, edge, filter, 8, 8, rng)) return 1;
        for (int e = 10; e <= 40; e += 5) {
            const double a[8] = {std::ldexp(1.0, -e), 0, 0, 0, std::ldexp(1.0, -e), 0, 0, -(1.0 - std::ldexp(1.0, -e)) / 7.5};
            for (uint32_t filter : kFilters)
                if (check_reference(20, 10, 1, a, filter, 8, 8, rng)) return 1;
            ++rounds;
        }
        // the largest finite coefficients that still give corner coordinates below 2^30
        const double huge[8] = {1e8, -1e8, 0, 1e8, 1e8, -5e8, 0, 0};
        for (uint32_t filter : kFilters)
            if (check_reference(20, 10, 1, huge, filter, 3, 3, rng)) return 1;
    }
    std::printf("ok %u\n", rounds);
    return 0;
}
