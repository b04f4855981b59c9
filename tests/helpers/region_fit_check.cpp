// Host-side check of the region decode's sub-geometry (llcomp_amd/csrc/geometry.hpp: region_box, region_geometry, region_full_id,
// region_fits) over a seeded grid of shapes, tilings and rectangles, under the default tuning and under forced LLCOMP_MI_LANE_SHIFT /
// LLCOMP_MI_LPW values.  For every case: sub-slice j and full slice region_full_id(j) are the same rectangle of the same frame and
// plane (ids in range, no id twice); with the default tuning every sub-geometry fits the full geometry's workspace; with forced hooks
// it fits or is refused.  Prints "ok <cases> <fits> <refused>" or the first failing case.
//   g++ -std=c++17 -O2 -I llcomp_amd/csrc tests/helpers/region_fit_check.cpp
#include <cstdio>
#include <random>
#include <vector>

#include "geometry.hpp"

using namespace llcomp_mi;

static unsigned long cases = 0, fits = 0, refused = 0;

static bool check(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tw, uint32_t th, uint32_t planar, uint32_t x, uint32_t y,
                  uint32_t rw, uint32_t rh, const Tuning& t, bool forced) {
    Geometry full{}, sub{};
    if (!make_geometry(full, frames, w, h, c, tw, th, planar, t)) return true;  // (a shape the format refuses: nothing to check)
    RegionBox b;
    if (!region_box(w, h, tw, th, x, y, rw, rh, b)) {
        std::printf("FAIL box %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    ++cases;
    if (!region_geometry(full, b, t, sub)) {
        std::printf("FAIL sub-geometry %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    const uint32_t planes = planar ? c : 1u;
    if (sub.n_slices != frames * (b.tx1 - b.tx0) * (b.ty1 - b.ty0) * planes || sub.ntx != b.tx1 - b.tx0 || sub.nty != b.ty1 - b.ty0) {
        std::printf("FAIL slice count %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    std::vector<char> seen(full.n_slices, 0);
    for (uint32_t j = 0; j < sub.n_slices; ++j) {
        const uint32_t id = region_full_id(full, sub, b, j);
        if (id >= full.n_slices || seen[id]) {
            std::printf("FAIL id %u -> %u\n", j, id);
            return false;
        }
        seen[id] = 1;
        const SliceRect s = slice_rect(sub, j), f = slice_rect(full, id);
        if (s.frame != f.frame || s.ch != f.ch || s.sw != f.sw || s.sh != f.sh || s.x0 + b.tx0 * full.tile_w != f.x0 ||
            s.y0 + b.ty0 * full.tile_h != f.y0) {
            std::printf("FAIL rect of %u (%u) in %u %u %u %u %u %u %u %u\n", j, id, w, h, tw, th, x, y, rw, rh);
            return false;
        }
    }
    if (region_fits(full, sub)) {
        ++fits;
    } else if (forced) {
        ++refused;
    } else {
        std::printf("FAIL default tuning does not fit %u %u %u %u %u %u %u %u %u\n", frames, w, h, tw, th, x, y, rw, rh);
        return false;
    }
    return true;
}

int main() {
    std::mt19937 rng(20261015);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    std::vector<Tuning> tunes(1);
    for (int s : {0, 2, 6}) { Tuning t; t.lane_shift = s; tunes.push_back(t); }
    for (int p : {1, 4, 32}) { Tuning t; t.lpw = p; tunes.push_back(t); }
    { Tuning t; t.lane_shift = 6; t.lpw = 1; tunes.push_back(t); }
    for (int i = 0; i < 400; ++i) {
        const uint32_t w = pick(1, 700), h = pick(1, 300), c = pick(1, 5), frames = pick(1, 6), planar = pick(0, 1);
        const uint32_t tw = pick(0, 3) == 0 ? 0 : pick(1, w), th = pick(0, 3) == 0 ? 0 : (pick(0, 2) == 0 ? pick(1, 2) : pick(1, h));
        const uint32_t ttw = tw == 0 ? w : tw, tth = th == 0 ? h : th;
        // rectangles: random, single pixel, whole image, inside one tile, touching the far edges, the partial last column / row only
        std::vector<uint32_t> r;
        const uint32_t x = pick(0, w - 1), y = pick(0, h - 1);
        r.insert(r.end(), {x, y, pick(1, w - x), pick(1, h - y)});
        r.insert(r.end(), {x, y, 1, 1});
        r.insert(r.end(), {0, 0, w, h});
        const uint32_t tx = x / ttw * ttw, ty = y / tth * tth;
        r.insert(r.end(), {tx, ty, std::min(ttw, w - tx), std::min(tth, h - ty)});
        r.insert(r.end(), {x, y, w - x, h - y});
        const uint32_t lx = (w - 1) / ttw * ttw, ly = (h - 1) / tth * tth;
        r.insert(r.end(), {lx, ly, w - lx, h - ly});
        r.insert(r.end(), {0, ly, w, h - ly});
        for (size_t k = 0; k < r.size(); k += 4)
            for (size_t ti = 0; ti < tunes.size(); ++ti)
                if (!check(frames, w, h, c, tw, th, planar, r[k], r[k + 1], r[k + 2], r[k + 3], tunes[ti], ti != 0)) return 1;
    }
    // big shapes: many 2-D slices (bank-cache family), few big slices (one per wavefront), 1-row slices, a 1-row remainder of 2-row tiles
    const uint32_t big[][7] = {{16, 3840, 2160, 3, 64, 64, 0}, {16, 3840, 2160, 3, 128, 128, 1}, {16, 3840, 2160, 3, 480, 1, 1},
                               {1, 3840, 2160, 3, 256, 256, 1}, {2, 1000, 1001, 3, 500, 2, 1}, {8, 1920, 1080, 3, 1920, 1080, 0}};
    for (const auto& s : big)
        for (int i = 0; i < 20; ++i) {
            const uint32_t x = pick(0, s[1] - 1), y = pick(0, s[2] - 1);
            for (size_t ti = 0; ti < tunes.size(); ++ti) {
                if (!check(s[0], s[1], s[2], s[3], s[4], s[5], s[6], x, y, pick(1, s[1] - x), pick(1, s[2] - y), tunes[ti], ti != 0)) return 1;
                if (!check(s[0], s[1], s[2], s[3], s[4], s[5], s[6], 0, s[2] - 1, s[1], 1, tunes[ti], ti != 0)) return 1;
            }
        }
    std::printf("ok %lu %lu %lu\n", cases, fits, refused);
    return 0;
}
