// warp_plan_check.cpp -- the host planner of the warped views (llcomp_amd/csrc/warp_plan.hpp) and the rule's host functions
// (warp_rule.hpp, llcomp_mi_warp_reference) under a sanitizer: seeded random groups of affine views -- every entry's source rectangle
// inside its frame's box, the block put into a heap buffer of exactly its size, the whole copy within the bound the codec sizes its
// staging buffer by -- the reference on the corner cases with image and output in heap buffers of exactly their sizes, every pixel the
// rule reads inside the source rectangle, and the refusals.  Host code only; built and run by tests/test_warp_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/warp_plan_check.cpp llcomp_amd/csrc/container.cpp llcomp_amd/csrc/windows_plan.cpp llcomp_amd/csrc/resize_plan.cpp
//       llcomp_amd/csrc/warp_plan.cpp llcomp_amd/csrc/photo_plan.cpp
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

// The reference on a heap image of exactly w * h * c bytes into a heap output of exactly ow * oh * c: under the sanitizer, no read or
// write outside either.  Then the source rectangle: inside the image, and every pixel the rule reads for an output pixel inside it.
int check_reference(uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, std::mt19937& rng) {
    std::unique_ptr<uint8_t[]> img(new uint8_t[size_t(w) * h * c]);
    for (size_t i = 0; i < size_t(w) * h * c; ++i) img[i] = uint8_t(rng());
    uint8_t fill[8];
    for (uint8_t& f : fill) f = uint8_t(rng());
    std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(ow) * oh * c]);
    CHECK(llcomp_mi_warp_reference(img.get(), w, h, c, m, filter, fill, ow, oh, out.get()) == LLCOMP_MI_OK);
    uint32_t rect[4], empty = 7;
    CHECK(llcomp_mi_warp_source_rect(w, h, m, filter, ow, oh, rect, &empty) == LLCOMP_MI_OK && empty <= 1);
    if (empty) {
        for (size_t i = 0; i < size_t(ow) * oh * c; ++i) CHECK(out[i] == fill[i % c]);
        CHECK(!rect[0] && !rect[1] && !rect[2] && !rect[3]);
        return 0;
    }
    CHECK(rect[2] && rect[3] && uint64_t(rect[0]) + rect[2] <= w && uint64_t(rect[1]) + rect[3] <= h);
    // NEAREST reads single pixels: every pixel it copies lies in the rectangle
    if (filter == LLCOMP_MI_FILTER_NEAREST) {
        std::vector<int32_t> xt(ow), yt(oh);
        int32_t A[6];
        const bool scale = warp_is_scale(m);
        if (scale) {
            warp_scale_table(m[0], m[2], ow, w, xt.data());
            warp_scale_table(m[4], m[5], oh, h, yt.data());
        } else {
            warp_fixed_matrix(m, A);
        }
        for (uint32_t y = 0; y < oh; ++y)
            for (uint32_t x = 0; x < ow; ++x) {
                int32_t xi, yi;
                if (scale)
                    xi = xt[x], yi = yt[y];
                else
                    warp_fixed_xy(A, x, y, xi, yi);
                if (xi < 0 || xi >= int32_t(w) || yi < 0 || yi >= int32_t(h)) continue;
                CHECK(uint32_t(xi) >= rect[0] && uint32_t(xi) < rect[0] + rect[2] && uint32_t(yi) >= rect[1] && uint32_t(yi) < rect[1] + rect[3]);
            }
        return 0;
    }
    for (uint32_t y = 0; y < oh; ++y)
        for (uint32_t x = 0; x < ow; ++x) {
            double xin, yin;
            warp_xy(m, x, y, xin, yin);
            if (!warp_inside(xin, yin, w, h)) continue;
            const WarpTap t = warp_tap(xin, yin);
            const int32_t lo = filter == LLCOMP_MI_FILTER_BICUBIC ? -1 : 0, hi = filter == LLCOMP_MI_FILTER_BICUBIC ? 2 : 1;
            for (int32_t d = lo; d <= hi; ++d) {
                const uint32_t col = uint32_t(warp_cl(t.X + d, int32_t(w))), row = uint32_t(warp_cl(t.Y + d, int32_t(h)));
                CHECK(col >= rect[0] && col < rect[0] + rect[2] && row >= rect[1] && row < rect[1] + rect[3]);
            }
        }
    return 0;
}

int check_plan(const Geometry& g, const WarpPlan& p, const std::vector<llcomp_mi_warp_group>& groups) {
    const WarpTail& t = p.tail;
    const uint32_t boxes = uint32_t(p.u.used.size());
    CHECK(p.tab.size() == boxes && t.groups.size() == groups.size());
    CHECK(t.box_bytes == uint64_t(boxes) * p.wmax * p.hmax * g.c);
    uint64_t entries = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const WarpOut& vg = t.groups[gi];
        CHECK(vg.first == entries && vg.n == groups[gi].n_views && vg.ow == groups[gi].ow && vg.oh == groups[gi].oh);
        entries += vg.n;
        CHECK(uint64_t(vg.fill_at) + g.c <= t.fills.size());
        if (!vg.out.plain) CHECK(vg.table_at % 16 == 0 && vg.table_at + vg.out.table_bytes(g.c) <= t.tables.size());
        for (uint32_t i = 0; i < vg.n; ++i) {
            const WarpEntry& z = t.ws[vg.first + i];
            const llcomp_mi_warp_view& v = groups[gi].views[i];
            const uint32_t form = (z.flags >> kWarpFormShift) & 3u, filter = LLCOMP_MI_FLAG_FILTER_OF(z.flags);
            CHECK((z.flags & 1u) == (v.flags & 1u) && filter == LLCOMP_MI_FLAG_FILTER_OF(v.flags));
            uint32_t rect[4];
            bool empty = false;
            CHECK(warp_source_rect(g.w, g.h, v.m, filter, vg.ow, vg.oh, rect, empty) == LLCOMP_MI_OK);
            CHECK(empty == (form == kWarpEmpty));
            if (empty) continue;
            // the source rectangle inside the entry's box, the box inside its frame
            CHECK(z.box < boxes && z.bx >= 0 && z.by >= 0 && uint64_t(z.bx) + p.wmax <= g.w && uint64_t(z.by) + p.hmax <= g.h);
            CHECK(p.u.used[z.box] == v.frame);
            CHECK(rect[0] >= uint32_t(z.bx) && rect[0] + rect[2] <= uint32_t(z.bx) + p.wmax && rect[1] >= uint32_t(z.by) &&
                  rect[1] + rect[3] <= uint32_t(z.by) + p.hmax);
            if (form == kWarpTable) {
                CHECK(filter == LLCOMP_MI_FILTER_NEAREST && warp_is_scale(v.m));
                CHECK(uint64_t(z.t[0]) + vg.ow <= t.tabs.size() && uint64_t(z.t[1]) + vg.oh <= t.tabs.size());
                for (uint32_t x = 0; x < vg.ow; ++x) CHECK(t.tabs[z.t[0] + x] >= -1 && t.tabs[z.t[0] + x] < int32_t(g.w));
                for (uint32_t y = 0; y < vg.oh; ++y) CHECK(t.tabs[z.t[1] + y] >= -1 && t.tabs[z.t[1] + y] < int32_t(g.h));
            } else {
                CHECK((form == kWarpFixed) == (filter == LLCOMP_MI_FILTER_NEAREST));
            }
        }
    }
    CHECK(entries == t.ws.size() && entries == p.total_views);
    std::unique_ptr<uint8_t[]> heap(new uint8_t[t.bytes()]);
    t.put(heap.get());
    CHECK(t.tables.empty() || std::memcmp(heap.get() + t.tables_at(), t.tables.data(), t.tables.size()) == 0);
    CHECK(t.tabs_at() % 8 == 0 && (t.tables.empty() || t.tables_at() % 16 == 0));
    // the block against the bound the staging buffer is sized by (outputs no larger than the image)
    CHECK(t.bytes() + 16 <= warp_tables_bound(g, p.total_views));
    // the whole copy, with and without a gather, with and without photometric chains, against the bounds the entry points pass on
    const uint64_t bound = warp_tables_bound(g, p.total_views);
    CHECK(copy_layout_ok(g, p, true, t.bytes(), p.total_views, &bound, uint32_t(t.bytes()) + 977u * uint32_t(p.tab.size())));
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20261019);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double(rng()) / 4294967296.0); };
    const uint32_t shapes[][4] = {{300, 200, 64, 64}, {160, 41, 40, 2}, {97, 61, 0, 0}, {48, 40, 16, 16}, {48, 40, 16, 1}};
    const uint32_t c = 3;
    const Tuning tune{};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const llcomp_mi_output_format formats[2] = {
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F32, LLCOMP_MI_LAYOUT_CHW, 1, mean, sd},
        {uint32_t(sizeof(llcomp_mi_output_format)), LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_HWC, 0, nullptr, nullptr}};
    void* const d_out = reinterpret_cast<void*>(uintptr_t(0x10000));  // (an address the planner checks and never follows)
    const uint8_t fill[3] = {1, 2, 3};
    uint32_t rounds = 0;
    auto random_map = [&](uint32_t w, uint32_t h, uint32_t kind, double* m) {
        const double ang = real(0, 6.283185307179586), sx = real(0.4, 2.5), sy = real(0.4, 2.5);
        m[0] = sx * std::cos(ang), m[1] = sx * std::sin(ang) + real(-0.5, 0.5), m[2] = real(-0.5 * w, 1.2 * w);
        m[3] = -sy * std::sin(ang), m[4] = sy * std::cos(ang), m[5] = real(-0.5 * h, 1.2 * h);
        if (kind == 1) m[1] = m[3] = 0.0, m[0] = (rng() & 1) ? sx : -sx;          // a pure scale (NEAREST: the table form)
        if (kind == 2) m[0] = m[4] = 1.0, m[1] = m[3] = 0.0, m[2] = std::floor(m[2]), m[5] = std::floor(m[5]);  // an integer translate
        if (kind == 3) m[2] += 20.0 * w;                                         // nothing inside
    };
    for (const auto& sh : shapes) {
        const uint32_t w = sh[0], h = sh[1], tw = sh[2], th = sh[3];
        for (int round = 0; round < 120; ++round) {
            const uint32_t frames = pick(1, 5);
            Geometry g;
            CHECK(make_geometry(g, frames, w, h, c, tw, th, 1, tune));
            const uint32_t n_groups = pick(1, 3);
            std::vector<std::vector<llcomp_mi_warp_view>> views(n_groups);
            std::vector<llcomp_mi_warp_group> groups(n_groups);
            const bool all_empty = round % 17 == 0;
            for (uint32_t gi = 0; gi < n_groups; ++gi) {
                views[gi].resize(pick(1, 6));
                for (llcomp_mi_warp_view& v : views[gi]) {
                    v.frame = pick(0, frames - 1);
                    v.flags = LLCOMP_MI_FLAG_FILTER(kFilters[rng() % 3]) | (rng() & 1u);
                    random_map(w, h, all_empty ? 3 : uint32_t(rng() % 5), v.m);
                }
                groups[gi] = llcomp_mi_warp_group{uint32_t(sizeof(llcomp_mi_warp_group)), uint32_t(views[gi].size()), views[gi].data(), pick(1, w), pick(1, h),
                                                  gi ? &formats[gi - 1] : nullptr, d_out, (rng() & 1) ? fill : nullptr};
            }
            WarpPlan p;
            CHECK(warp_setup(g, tune, groups.data(), n_groups, p) == LLCOMP_MI_OK);
            if (all_empty) CHECK(p.u.used.empty() && p.tab.empty() && !p.n_classes && !p.tail.box_bytes);
            if (check_plan(g, p, groups)) return 1;
            // the public plan: the same unions, and as many used frames
            std::vector<uint32_t> uni(4 * frames, 9), win(4 * frames, 9);
            uint32_t used = 9, cls = 9;
            CHECK(llcomp_mi_warp_views_plan(w, h, c, tw, th, 1, frames, groups.data(), n_groups, uni.data(), win.data(), &used, &cls) == LLCOMP_MI_OK);
            CHECK(used == p.u.used.size() && cls == p.n_classes && std::memcmp(uni.data(), p.u.rects.data(), 16 * frames) == 0);
            // a refusal in the middle of a call leaves nothing half done
            views[n_groups - 1].back().m[4] = std::numeric_limits<double>::quiet_NaN();
            WarpPlan q;
            CHECK(warp_setup(g, tune, groups.data(), n_groups, q) == LLCOMP_MI_BAD_ARGS);
            ++rounds;
        }
    }
    // the reference and the source rectangle on the corner cases: 1 x 1 and 1 x N images, the identity, views wholly or half outside
    const uint32_t sides[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {13, 7}, {39, 31}};
    for (const auto& s : sides)
        for (uint32_t filter : kFilters)
            for (uint32_t kind = 0; kind < 5; ++kind)
                for (int rep = 0; rep < 8; ++rep) {
                    double m[6];
                    random_map(s[0], s[1], kind, m);
                    if (kind == 4) m[0] = m[4] = 1.0, m[1] = m[2] = m[3] = m[5] = 0.0;  // the identity
                    for (uint32_t ch : {1u, 3u, 5u})
                        if (check_reference(s[0], s[1], ch, m, filter, pick(1, 24), pick(1, 24), rng)) return 1;
                    ++rounds;
                }
    // the limits
    {
        uint32_t rect[4] = {7, 7, 7, 7}, empty = 7;
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const double bad[][6] = {{nan, 0, 0, 0, 1, 0}, {1, 0, inf, 0, 1, 0}, {1, 0.5, 32768.0, 0, 1, 0}, {1, 0, 0, 0.25, 1, -32768.0}, {1e300, 0, 0, 0, 1, 0}};
        for (const auto& m : bad) {
            CHECK(llcomp_mi_warp_source_rect(20, 10, m, LLCOMP_MI_FILTER_NEAREST, 8, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
            CHECK(rect[0] == 7 && rect[3] == 7 && empty == 7);
        }
        const double far[6] = {1, 0, 1073741824.0, 0, 1, 0}, ident[6] = {1, 0, 0, 0, 1, 0};
        CHECK(llcomp_mi_warp_source_rect(20, 10, far, LLCOMP_MI_FILTER_BICUBIC, 8, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
        CHECK(llcomp_mi_warp_source_rect(20, 10, ident, LLCOMP_MI_FILTER_LANCZOS, 8, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
        CHECK(llcomp_mi_warp_source_rect(20, 10, ident, LLCOMP_MI_FILTER_BILINEAR, 0, 8, rect, &empty) == LLCOMP_MI_BAD_ARGS);
        CHECK(llcomp_mi_warp_source_rect(20, 10, ident, LLCOMP_MI_FILTER_BILINEAR, 20, 10, rect, &empty) == LLCOMP_MI_OK);
        CHECK(rect[0] == 0 && rect[1] == 0 && rect[2] == 20 && rect[3] == 10 && empty == 0);
    }
    std::printf("ok %u\n", rounds);
    return 0;
}
