// views_plan_check.cpp -- the host side of a views decode under a sanitizer: llcomp_mi_views_plan against a brute-force bounding box over
// seeded random groups (outputs of exactly 4 * frames values, so a write past them is seen), and the gather over a frame list with the
// unused frames' containers NULL (a read of one is seen).  Host code only; built and run by tests/test_views_plan.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc tests/helpers/views_plan_check.cpp
//       llcomp_amd/csrc/container.cpp
// Prints "ok <plans> <gathers>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "container.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    std::mt19937 rng(20240607);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    const uint32_t shapes[][4] = {{300, 200, 64, 64}, {1100, 24, 480, 1}, {160, 41, 40, 2}, {97, 61, 0, 0}, {32, 32, 12, 10}};
    uint32_t plans = 0, gathers = 0;
    for (const auto& sh : shapes) {
        const uint32_t w = sh[0], h = sh[1], tw = sh[2], th = sh[3];
        for (int round = 0; round < 200; ++round) {
            const uint32_t frames = pick(1, 6), n_groups = pick(1, 3);
            std::vector<std::vector<llcomp_mi_view>> views(n_groups);
            std::vector<llcomp_mi_view_group> groups(n_groups);
            std::vector<uint32_t> x0(frames, ~0u), y0(frames, ~0u), x1(frames, 0), y1(frames, 0);
            for (uint32_t g = 0; g < n_groups; ++g) {
                const uint32_t n = pick(1, 5);
                for (uint32_t i = 0; i < n; ++i) {
                    llcomp_mi_view v;
                    v.frame = round % 3 == 0 ? pick(0, frames - 1) / 2 * 2 % frames : pick(0, frames - 1);  // (every third round: even frames only)
                    v.rw = pick(1, w);
                    v.rh = pick(1, h);
                    v.x = pick(0, w - v.rw);
                    v.y = pick(0, h - v.rh);
                    v.flags = pick(0, 1) | LLCOMP_MI_FLAG_FILTER(pick(0, 3));
                    views[g].push_back(v);
                    x0[v.frame] = std::min(x0[v.frame], v.x);
                    y0[v.frame] = std::min(y0[v.frame], v.y);
                    x1[v.frame] = std::max(x1[v.frame], v.x + v.rw);
                    y1[v.frame] = std::max(y1[v.frame], v.y + v.rh);
                }
                groups[g] = llcomp_mi_view_group{uint32_t(sizeof(llcomp_mi_view_group)), n, views[g].data(), (w + 63) / 64 + pick(0, 40),
                                                 (h + 63) / 64 + pick(0, 40), nullptr, nullptr};
            }
            std::vector<uint32_t> unions(4 * frames, 7), windows(4 * frames, 7);
            uint32_t n_used = 0, n_classes = 0;
            CHECK(llcomp_mi_views_plan(w, h, 3, tw, th, 1, frames, groups.data(), n_groups, unions.data(), windows.data(), &n_used, &n_classes) ==
                  LLCOMP_MI_OK);
            std::vector<uint32_t> used, rects;
            for (uint32_t f = 0; f < frames; ++f) {
                const uint32_t* u = unions.data() + 4 * f;
                if (!x1[f]) {
                    CHECK(!u[0] && !u[1] && !u[2] && !u[3] && !windows[4 * f] && !windows[4 * f + 2]);
                    continue;
                }
                CHECK(u[0] == x0[f] && u[1] == y0[f] && u[2] == x1[f] - x0[f] && u[3] == y1[f] - y0[f]);
                used.push_back(f);
                rects.insert(rects.end(), u, u + 4);
            }
            CHECK(n_used == used.size());
            std::vector<uint32_t> win(4 * used.size());
            uint32_t ncls = 0;
            CHECK(llcomp_mi_resized_regions_plan(w, h, 3, tw, th, 1, rects.data(), uint32_t(used.size()), win.data(), &ncls) == LLCOMP_MI_OK);
            CHECK(ncls == n_classes);
            for (size_t i = 0; i < used.size(); ++i)
                for (int j = 0; j < 4; ++j) CHECK(win[4 * i + j] == windows[4 * used[i] + j]);
            ++plans;
            // the gather over the frame list: containers of empty slices for the used frames, NULL for every other frame
            Geometry g1;
            CHECK(make_geometry(g1, 1, w, h, 3, tw, th, 1));
            std::vector<uint8_t> cont(LLCOMP_MI_SLICED_HEADER_BYTES + 4 * size_t(g1.slices_per_frame), 0);
            write_sliced_header(cont.data(), g1);
            std::vector<const uint8_t*> data(frames, nullptr);
            std::vector<size_t> lens(frames, 0);
            for (uint32_t f : used) {
                data[f] = cont.data();
                lens[f] = cont.size();
            }
            ViewsUnion u;
            CHECK(views_union(w, h, frames, groups.data(), n_groups, u) == LLCOMP_MI_OK && u.used == used);
            RegionsGather p, q;
            CHECK(regions_gather_plan_sized(data.data(), lens.data(), frames, u.rects.data(), u.wmax, u.hmax, p, u.used.data(), uint32_t(u.used.size())) ==
                  LLCOMP_MI_OK);
            // ... plans what the existing gather plans for the used frames' containers and rectangles alone
            std::vector<const uint8_t*> d2(used.size(), cont.data());
            std::vector<size_t> l2(used.size(), cont.size());
            CHECK(regions_gather_plan_sized(d2.data(), l2.data(), uint32_t(used.size()), rects.data(), u.wmax, u.hmax, q) == LLCOMP_MI_OK);
            CHECK(p.n_slices == q.n_slices && p.n_classes == q.n_classes && p.n_classes == n_classes && p.runs.size() == q.runs.size());
            for (size_t i = 0; i < p.runs.size(); ++i)
                CHECK(p.runs[i].frame == used[q.runs[i].frame] && p.runs[i].first == q.runs[i].first && p.runs[i].count == q.runs[i].count);
            std::vector<uint32_t> slice_len(p.n_slices + 1, 9);
            std::vector<uint64_t> slice_off(p.n_slices + 1, 9);
            uint8_t payload[1];
            regions_gather_copy(p, data.data(), payload, slice_len.data(), slice_off.data());
            CHECK(slice_len[p.n_slices] == 9 && (!p.n_slices || slice_len[p.n_slices - 1] == 0));
            // a used frame without a container is refused
            data[used[0]] = nullptr;
            CHECK(regions_gather_plan_sized(data.data(), lens.data(), frames, u.rects.data(), u.wmax, u.hmax, p, u.used.data(), uint32_t(u.used.size())) ==
                  LLCOMP_MI_BAD_ARGS);
            ++gathers;
        }
    }
    std::printf("ok %u %u\n", plans, gathers);
    return 0;
}
