// Host-side check of the regions decode's class sub-geometries (llcomp_amd/csrc/geometry.hpp: regions_window, regions_geometry,
// regions_full_id, regions_fits) over a seeded grid of shapes, tilings, rectangle sizes and per-frame offsets, under the default
// tuning and under forced LLCOMP_MI_LANE_SHIFT / LLCOMP_MI_LPW values.  For every batch: each window has the class's size and
// contains the frame's covered box (region_box); every class's sub-slice j and full slice regions_full_id(j) are the same rectangle of
// the same frame and plane, and no full slice is read twice across the classes of a batch; the rectangle lies inside its window;
// with the default tuning every class's sub-geometry fits the full geometry's workspace, with forced hooks it fits or is refused.
// Every batch also runs cut short to 1, 3, 5 ... of its frames (classes of every frame count).
// Prints "ok <classes checked> <fits> <refused>" or the first failing case.
//   g++ -std=c++17 -O2 -I llcomp_amd/csrc tests/helpers/regions_fit_check.cpp
#include <cstdio>
#include <random>
#include <vector>

#include "geometry.hpp"

using namespace llcomp_mi;

static unsigned long cases = 0, fits = 0, refused = 0;

static bool check(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tw, uint32_t th, uint32_t planar, uint32_t rw, uint32_t rh,
                  const std::vector<uint32_t>& xy, const Tuning& t, bool forced) {
    Geometry full{};
    if (!make_geometry(full, frames, w, h, c, tw, th, planar, t)) return true;  // (a shape the format refuses: nothing to check)
    std::vector<RegionBox> win(frames);
    std::vector<uint32_t> cls(frames);
    uint32_t count[kRegionsClasses] = {};
    for (uint32_t f = 0; f < frames; ++f) {
        RegionBox b;
        if (!regions_window(w, h, tw, th, xy[2 * f], xy[2 * f + 1], rw, rh, win[f], cls[f]) ||
            !region_box(w, h, tw, th, xy[2 * f], xy[2 * f + 1], rw, rh, b)) {
            std::printf("FAIL window %u %u %u %u %u %u %u %u\n", w, h, tw, th, xy[2 * f], xy[2 * f + 1], rw, rh);
            return false;
        }
        if (win[f].tx0 > b.tx0 || win[f].ty0 > b.ty0 || win[f].tx1 < b.tx1 || win[f].ty1 < b.ty1 || win[f].tx1 > full.ntx ||
            win[f].ty1 > full.nty || win[f].tx1 - win[f].tx0 != win[0].tx1 - win[0].tx0 || win[f].ty1 - win[f].ty0 != win[0].ty1 - win[0].ty0) {
            std::printf("FAIL containment %u %u %u %u %u %u %u %u\n", w, h, tw, th, xy[2 * f], xy[2 * f + 1], rw, rh);
            return false;
        }
        ++count[cls[f]];
    }
    std::vector<char> seen(full.n_slices, 0);
    const uint32_t planes = planar ? c : 1u;
    for (uint32_t k = 0; k < kRegionsClasses; ++k) {
        if (!count[k]) continue;
        std::vector<RegionsFrame> tab;
        for (uint32_t f = 0; f < frames; ++f)
            if (cls[f] == k)
                tab.push_back(RegionsFrame{f, win[f].tx0, win[f].ty0, xy[2 * f] - win[f].tx0 * full.tile_w, xy[2 * f + 1] - win[f].ty0 * full.tile_h, f, k, 0});
        Geometry sub{};
        ++cases;
        if (!regions_geometry(full, win[tab[0].frame], count[k], t, sub)) {
            std::printf("FAIL sub-geometry %u %u %u %u %u %u class %u\n", w, h, tw, th, rw, rh, k);
            return false;
        }
        const uint32_t wx = win[0].tx1 - win[0].tx0, wy = win[0].ty1 - win[0].ty0;
        if (sub.frames != count[k] || sub.ntx != wx || sub.nty != wy || sub.n_slices != count[k] * wx * wy * planes) {
            std::printf("FAIL slice count %u %u %u %u %u %u class %u\n", w, h, tw, th, rw, rh, k);
            return false;
        }
        for (const RegionsFrame& e : tab)
            if (e.cx0 + rw > sub.w || e.cy0 + rh > sub.h) {
                std::printf("FAIL crop outside the window %u %u %u %u %u %u class %u\n", w, h, tw, th, rw, rh, k);
                return false;
            }
        for (uint32_t j = 0; j < sub.n_slices; ++j) {
            const uint32_t id = regions_full_id(full, sub, tab.data(), j);
            if (id >= full.n_slices || seen[id]) {
                std::printf("FAIL id %u -> %u\n", j, id);
                return false;
            }
            seen[id] = 1;
            const SliceRect s = slice_rect(sub, j), r = slice_rect(full, id);
            const RegionsFrame& e = tab[s.frame];
            if (e.frame != r.frame || s.ch != r.ch || s.sw != r.sw || s.sh != r.sh || s.x0 + e.wx0 * full.tile_w != r.x0 ||
                s.y0 + e.wy0 * full.tile_h != r.y0) {
                std::printf("FAIL rect of %u (%u) in %u %u %u %u %u %u class %u\n", j, id, w, h, tw, th, rw, rh, k);
                return false;
            }
        }
        if (regions_fits(full, sub)) {
            ++fits;
        } else if (forced) {
            ++refused;
        } else {
            std::printf("FAIL default tuning does not fit %u %u %u %u %u %u %u class %u\n", frames, w, h, tw, th, rw, rh, k);
            return false;
        }
    }
    return true;
}

int main() {
    std::mt19937 rng(20261016);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + uint32_t(rng() % (hi - lo + 1)); };
    std::vector<Tuning> tunes(1);
    for (int s : {0, 2, 6}) { Tuning t; t.lane_shift = s; tunes.push_back(t); }
    for (int p : {1, 4, 32}) { Tuning t; t.lpw = p; tunes.push_back(t); }
    { Tuning t; t.lane_shift = 6; t.lpw = 1; tunes.push_back(t); }
    // offsets of one batch: random, the origin, the last partial tile column / row, both, and a tile-aligned one
    auto offsets = [&](uint32_t frames, uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t rw, uint32_t rh) {
        const uint32_t ttw = tw == 0 || tw > w ? w : tw, tth = th == 0 || th > h ? h : th;
        std::vector<uint32_t> xy;
        for (uint32_t f = 0; f < frames; ++f) {
            uint32_t x = pick(0, w - rw), y = pick(0, h - rh);
            switch (f % 5) {
                case 1: x = 0; y = 0; break;
                case 2: x = w - rw; break;
                case 3: x = w - rw; y = h - rh; break;
                case 4: x = std::min(x / ttw * ttw, w - rw); y = std::min(y / tth * tth, h - rh); break;
                default: break;
            }
            xy.push_back(x);
            xy.push_back(y);
        }
        return xy;
    };
    auto run = [&](uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tw, uint32_t th, uint32_t planar, uint32_t rw, uint32_t rh) {
        const std::vector<uint32_t> xy = offsets(frames, w, h, tw, th, rw, rh);
        for (size_t ti = 0; ti < tunes.size(); ++ti) {
            if (!check(frames, w, h, c, tw, th, planar, rw, rh, xy, tunes[ti], ti != 0)) return false;
            // the same offsets as smaller batches: every class frame count from 1 up
            for (uint32_t n = 1; n < frames; n += 2) {
                const std::vector<uint32_t> part(xy.begin(), xy.begin() + 2 * n);
                if (!check(n, w, h, c, tw, th, planar, rw, rh, part, tunes[ti], ti != 0)) return false;
            }
        }
        return true;
    };
    for (int i = 0; i < 300; ++i) {
        const uint32_t w = pick(1, 700), h = pick(1, 300), c = pick(1, 5), frames = pick(1, 9), planar = pick(0, 1);
        const uint32_t tw = pick(0, 3) == 0 ? 0 : pick(1, w), th = pick(0, 3) == 0 ? 0 : (pick(0, 2) == 0 ? pick(1, 2) : pick(1, h));
        const uint32_t ttw = tw == 0 ? w : tw, tth = th == 0 ? h : th;
        // rectangle sizes: random, one pixel, the whole image, one tile
        const uint32_t sizes[][2] = {{pick(1, w), pick(1, h)}, {1, 1}, {w, h}, {std::min(ttw, w), std::min(tth, h)}};
        for (const auto& sz : sizes)
            if (!run(frames, w, h, c, tw, th, planar, sz[0], sz[1])) return 1;
    }
    // big shapes: random crops of 4K batches (1-row slices, 64x64 interleaved = 2 classes, 128x128 planes), a 1-row remainder of 2-row tiles
    const uint32_t big[][7] = {{16, 3840, 2160, 3, 64, 64, 0}, {16, 3840, 2160, 3, 128, 128, 1}, {16, 3840, 2160, 3, 480, 1, 1},
                               {4, 3840, 2160, 3, 256, 256, 1}, {3, 1000, 1001, 3, 500, 2, 1}, {8, 1920, 1080, 3, 1920, 1080, 0}};
    for (const auto& s : big)
        for (uint32_t r : {224u, 512u, 1u, 1000u})
            if (!run(s[0], s[1], s[2], s[3], s[4], s[5], s[6], r, std::min(r, s[2]))) return 1;
    std::printf("ok %lu %lu %lu\n", cases, fits, refused);
    return 0;
}
