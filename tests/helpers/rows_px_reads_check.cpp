// Host-side check of the row encoder's pixel reads (slice_kernels.hip, k_encode_slices with SYM = uint8_t; geometry.hpp:
// rows_px_dwords, rows_px_tail, rows_encoder_reads_pixels).  The kernel's load schedule per lane, over a grid of planar 1-row
// geometries with 1..4 channels (ragged tile columns, tiny tiles, one and several frames, narrow and full lane groups):
//   prologue          sample 0, and sample 1 when the slice has two: with the per-lane test (dword below rows_px_dwords, else C bytes)
//   bulk loop         only when every lane of the wavefront has the same sample count n: samples 2 .. n - rows_px_tail(C) + 1 as
//                     dwords, no test
//   loop with tests   every later sample up to n - 1, with the per-lane test
// Every byte any of these reads must lie inside the batch [0, frames*h*w*C), and every lane's offset from its wavefront's first lane
// (the kernel's 32-bit offsets) must stay below 2^31.  Prints "ok <geometries> <lanes> <byte-path reads>" or the first failing case.
//   g++ -std=c++17 -O2 -I llcomp_amd/csrc tests/helpers/rows_px_reads_check.cpp
#include <cstdio>

#include "geometry.hpp"

using namespace llcomp_mi;

static unsigned long geometries = 0, lanes = 0, byte_reads = 0;

static bool check(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tw) {
    Geometry g{};
    if (!make_geometry(g, frames, w, h, c, tw, 1, 1)) return true;
    if (!(g.flags & kGeoRows) || g.c > 4) return true;  // (not the fused family: nothing to check)
    ++geometries;
    const uint64_t batch = uint64_t(frames) * h * w * c;
    for (uint32_t first = 0; first < g.n_slices; first += g.lpw) {  // one wavefront: lanes first .. first + lpw - 1
        const uint32_t end = first + g.lpw < g.n_slices ? first + g.lpw : g.n_slices;
        auto base_of = [&](uint32_t id) {
            const SliceRect r = slice_rect(g, id);
            return (uint64_t(r.frame) * h + r.y0) * w * c + uint64_t(r.x0) * c;
        };
        const uint64_t wbase = base_of(first);
        const uint32_t n0 = slice_rect(g, first).sw;
        bool same = true;
        for (uint32_t id = first; id < end; ++id) same = same && slice_rect(g, id).sw == n0;
        const uint32_t tail = rows_px_tail(c);
        const uint32_t n_bulk = same && n0 > tail ? n0 - tail : 0;
        for (uint32_t id = first; id < end; ++id) {
            ++lanes;
            const uint64_t tbase = base_of(id);
            const uint32_t n = slice_rect(g, id).sw;
            if (tbase < wbase || tbase - wbase + uint64_t(n) * c >= (1ull << 31)) {
                std::printf("FAIL offset %u %u %u %u %u id %u\n", frames, w, h, c, tw, id);
                return false;
            }
            const uint32_t n_dword = rows_px_dwords(tbase, n, c, batch);
            auto read = [&](uint32_t k, bool tested) {
                const uint64_t at = tbase + uint64_t(k) * c;
                const bool dword = !tested || k < n_dword;
                byte_reads += dword ? 0 : 1;
                if (at + (dword ? 4 : c) > batch) {
                    std::printf("FAIL read %u %u %u %u %u id %u sample %u of %u (%s)\n", frames, w, h, c, tw, id, k, n, dword ? "dword" : "bytes");
                    return false;
                }
                return true;
            };
            if (!read(0, true)) return false;
            if (n > 1 && !read(1, true)) return false;
            for (uint32_t i = 0; i < n_bulk; ++i)
                if (!read(i + 2, false)) return false;
            for (uint32_t i = n_bulk; i < n; ++i)
                if (i + 2 < n && !read(i + 2, true)) return false;
        }
    }
    return true;
}

int main() {
    const uint32_t widths[] = {1, 2, 3, 4, 5, 7, 31, 64, 97, 130, 481, 1100};
    const uint32_t tiles[] = {1, 2, 3, 4, 5, 8, 33, 64, 96, 480, 0};
    for (uint32_t c = 1; c <= 4; ++c)
        for (uint32_t frames : {1u, 3u})
            for (uint32_t h : {1u, 2u, 9u})
                for (uint32_t w : widths)
                    for (uint32_t tw : tiles)
                        if (!check(frames, w, h, c, tw)) return 1;
    // narrow and full lane groups: enough slices for 64-lane groups with tails of every length
    for (uint32_t c = 1; c <= 4; ++c)
        for (uint32_t w : {60u, 61u, 62u, 63u, 125u, 1100u})
            for (uint32_t tw : {1u, 2u, 3u, 7u, 480u})
                if (!check(2, w, 40, c, tw)) return 1;
    if (byte_reads == 0) {
        std::printf("FAIL no read took the byte path\n");
        return 1;
    }
    std::printf("ok %lu %lu %lu\n", geometries, lanes, byte_reads);
    return 0;
}
