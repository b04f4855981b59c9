// Host-side check of the region update's fit rule (llcomp_amd/csrc/geometry.hpp: region_encode_fits, region_sub_id,
// region_snapshot_bound) over a seeded grid of shapes, tilings, rectangles and EVERY frame count 1..8, under the default tuning and under
// the forced hooks LLCOMP_MI_LANE_SHIFT / LLCOMP_MI_LPW / NOROWS / NOSNAP / NOLDSTAB.  For every case: region_sub_id is the inverse of
// region_full_id on the box and ~0u outside it; the sub-geometry's lane groups fit the encoder's own offsets array (n_slices + 1
// entries); with the default tuning the encoder's arrays fit the full geometry's workspace; with forced hooks they fit or the call is
// refused.  Prints "ok <cases> <fits> <refused by forced hooks> <of those: refused for the decoder already>" or the first failing case.
//   g++ -std=c++17 -O2 -I llcomp_amd/csrc tests/helpers/region_encode_fit_check.cpp
#include <cstdio>
#include <random>
#include <vector>

#include "geometry.hpp"

using namespace llcomp_mi;

static unsigned long cases = 0, fits = 0, refused = 0, refused_decode = 0;

static bool check(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tw, uint32_t th, uint32_t planar, uint32_t x, uint32_t y,
                  uint32_t rw, uint32_t rh, const Tuning& t, bool forced) {
    Geometry full{}, sub{};
    if (!make_geometry(full, frames, w, h, c, tw, th, planar, t)) return true;  // (a shape the format refuses: nothing to check)
    RegionBox b;
    if (!region_box(w, h, tw, th, x, y, rw, rh, b) || !region_geometry(full, b, t, sub)) {
        std::printf("FAIL box / sub-geometry %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    ++cases;
    uint32_t covered = 0;
    for (uint32_t id = 0; id < full.n_slices; ++id) {
        const uint32_t j = region_sub_id(full, sub, b, id);
        if (j == ~0u) continue;
        ++covered;
        if (j >= sub.n_slices || region_full_id(full, sub, b, j) != id) {
            std::printf("FAIL sub id %u -> %u in %u %u %u %u %u %u %u %u\n", id, j, w, h, tw, th, x, y, rw, rh);
            return false;
        }
    }
    if (covered != sub.n_slices) {
        std::printf("FAIL covered %u of %u in %u %u %u %u %u %u %u %u\n", covered, sub.n_slices, w, h, tw, th, x, y, rw, rh);
        return false;
    }
    const bool whole = region_is_whole_box(full, sub, b, x, y, rw, rh);
    if (whole != (uint64_t(rw) * rh == uint64_t(sub.w) * sub.h)) {  // (a rectangle inside its box is the box iff it has its area)
        std::printf("FAIL whole box %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    const uint64_t groups = (uint64_t(sub.n_slices) + (1u << sub.lane_shift) - 1) >> sub.lane_shift;
    if (groups + 1 > uint64_t(full.n_slices) + 1) {
        std::printf("FAIL lane groups %u %u %u %u %u %u %u %u\n", w, h, tw, th, x, y, rw, rh);
        return false;
    }
    if (region_encode_fits(full, sub)) {
        ++fits;
    } else if (forced) {
        ++refused;
        if (!region_fits(full, sub)) ++refused_decode;
    } else {
        std::printf("FAIL default tuning does not fit %u %u %u %u %u %u %u %u %u %u %u\n", frames, w, h, c, tw, th, planar, x, y, rw, rh);
        return false;
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
    { Tuning t; t.norows = true; tunes.push_back(t); }
    { Tuning t; t.nosnap = true; tunes.push_back(t); }
    { Tuning t; t.noldstab = true; tunes.push_back(t); }
    { Tuning t; t.norows = t.nosnap = t.noldstab = true; tunes.push_back(t); }
    for (int i = 0; i < 300; ++i) {
        const uint32_t w = pick(1, 700), h = pick(1, 300), c = pick(1, 5), planar = pick(0, 1);
        const uint32_t tw = pick(0, 3) == 0 ? 0 : pick(1, w), th = pick(0, 3) == 0 ? 0 : (pick(0, 2) == 0 ? pick(1, 2) : pick(1, h));
        const uint32_t ttw = tw == 0 ? w : tw, tth = th == 0 ? h : th;
        std::vector<uint32_t> r;
        const uint32_t x = pick(0, w - 1), y = pick(0, h - 1);
        r.insert(r.end(), {x, y, pick(1, w - x), pick(1, h - y)});
        r.insert(r.end(), {x, y, 1, 1});
        r.insert(r.end(), {0, 0, w, h});
        const uint32_t tx = x / ttw * ttw, ty = y / tth * tth;
        r.insert(r.end(), {tx, ty, std::min(ttw, w - tx), std::min(tth, h - ty)});
        const uint32_t lx = (w - 1) / ttw * ttw, ly = (h - 1) / tth * tth;
        r.insert(r.end(), {lx, ly, w - lx, h - ly});
        r.insert(r.end(), {0, ly, w, h - ly});
        r.insert(r.end(), {lx, 0, w - lx, h});
        for (uint32_t frames = 1; frames <= 8; ++frames)
            for (size_t k = 0; k < r.size(); k += 4)
                for (size_t ti = 0; ti < tunes.size(); ++ti)
                    if (!check(frames, w, h, c, tw, th, planar, r[k], r[k + 1], r[k + 2], r[k + 3], tunes[ti], ti != 0)) return 1;
    }
    // big shapes: many 2-D slices (chunked snapshot pass), few big slices (one per wavefront), slices above 16384 samples (table encoder)
    // whose clamped last column / row runs the snapshot pass, 1-row slices, a 1-row remainder of 2-row tiles, a LEGACY-like single slice
    const uint32_t big[][6] = {{3840, 2160, 3, 64, 64, 0}, {3840, 2160, 3, 128, 128, 1}, {3840, 2160, 3, 480, 1, 1}, {3840, 2160, 3, 256, 256, 1},
                               {1000, 1001, 3, 500, 2, 1}, {1920, 1080, 3, 1920, 1080, 0}, {1080, 1080, 3, 256, 256, 1}, {1100, 1100, 1, 512, 512, 0}};
    for (const auto& s : big)
        for (uint32_t frames : {1u, 2u, 3u, 5u, 8u, 16u, 32u, 64u}) {
            const uint32_t lx = (s[0] - 1) / s[3] * s[3], ly = (s[1] - 1) / s[4] * s[4];
            for (int i = 0; i < 6; ++i) {
                const uint32_t x = pick(0, s[0] - 1), y = pick(0, s[1] - 1);
                const uint32_t rw = pick(1, s[0] - x), rh = pick(1, s[1] - y);
                for (size_t ti = 0; ti < tunes.size(); ++ti) {
                    if (!check(frames, s[0], s[1], s[2], s[3], s[4], s[5], x, y, rw, rh, tunes[ti], ti != 0)) return 1;
                    if (i) continue;
                    if (!check(frames, s[0], s[1], s[2], s[3], s[4], s[5], 0, ly, s[0], s[1] - ly, tunes[ti], ti != 0)) return 1;
                    if (!check(frames, s[0], s[1], s[2], s[3], s[4], s[5], lx, 0, s[0] - lx, s[1], tunes[ti], ti != 0)) return 1;
                    if (!check(frames, s[0], s[1], s[2], s[3], s[4], s[5], lx, ly, s[0] - lx, s[1] - ly, tunes[ti], ti != 0)) return 1;
                    if (!check(frames, s[0], s[1], s[2], s[3], s[4], s[5], 0, 0, s[0], s[1], tunes[ti], ti != 0)) return 1;
                }
            }
        }
    std::printf("ok %lu %lu %lu %lu\n", cases, fits, refused, refused_decode);
    return 0;
}
