// photo_sharp_check.cpp -- ADJUST_SHARPNESS of the photometric chains on the host under a sanitizer: the planner's band, halo and chunk
// arithmetic (llcomp_amd/csrc/photo_plan.hpp: photo_setup, photo_sharp_band_rows) over seeded groups of up to 5000 x 5000 under seeded
// staging bounds, the addresses the driver and the kernels derive from a plan walked against a buffer of exactly stage_bytes,
// llcomp_mi_photo_reference with image and output in heap buffers of exactly their sizes -- out of place, in place, op by op -- on
// chains that mix the op with all the others, the rule's functions, and the refusals.  Host code only; built and run by
// tests/test_photo_sharpness_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/photo_sharp_check.cpp llcomp_amd/csrc/photo_plan.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "photo_check.hpp"
#include "photo_plan.hpp"
#include "photo_rule.hpp"

using namespace llcomp_mi;

namespace {

llcomp_mi_photo_op random_op(std::mt19937& rng, bool sharp_only) {
    const float factors[6] = {0.0f, 1.0f, 0.37f, 2.75f, 7.5f, 256.0f};
    const uint32_t kind = sharp_only ? 0 : rng() % 5;
    if (kind == 0) return llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, factors[rng() % 6]};
    if (kind == 1) return llcomp_mi_photo_op{LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, float(rng() % 5) * 0.75f};
    if (kind == 2) return llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_HUE, float(int(rng() % 11) - 5) * 0.1f};
    llcomp_mi_photo_op o;
    o.op = rng() % LLCOMP_MI_PHOTO_OP_COUNT;
    o.param = o.op == LLCOMP_MI_PHOTO_SOLARIZE ? float(rng() % 257) : o.op == LLCOMP_MI_PHOTO_POSTERIZE ? float(1 + rng() % 8) : factors[rng() % 4];
    return o;
}

std::unique_ptr<llcomp_mi_photo_chain[]> random_chains(uint32_t n, std::mt19937& rng) {
    return heap_chains(n, rng, [](std::mt19937& r) { return random_op(r, false); });
}

// The plan of one group against its bound: what the driver and the kernels will address lies inside stage_bytes, and stage_bytes
// inside the bound wherever the group's view fits it at all.
int check_group(const PhotoGroup& pg, const PhotoTail& t, uint32_t c, uint64_t samples) {
    const uint64_t pitch = uint64_t(pg.ow) * c, view = pitch * pg.oh;
    CHECK(pg.chunk >= 1 && pg.chunk <= pg.n);  // (a single view is always planned)
    if (!std::any_of(pg.step, pg.step + pg.steps, [](const PhotoStepInfo& s) { return s.has(PhotoKind::kSharp); })) {
        CHECK(pg.sharp_rows == 0 && pg.halo_at == kPhotoNoHalo);
        CHECK(pg.chunk * view <= t.stage_bytes && (pg.chunk == 1 || pg.chunk * view <= samples));
        return 0;
    }
    const uint32_t rows = pg.sharp_rows;
    CHECK(rows >= 1 && rows <= pg.oh);
    const uint32_t bands = photo_sharp_bands(pg.oh, rows);
    CHECK(uint64_t(bands) * rows >= pg.oh && uint64_t(bands - 1) * rows < pg.oh);  // every row in one band, no band empty
    const uint64_t halo = photo_sharp_halo_bytes(pg.ow, pg.oh, c, rows);
    CHECK(halo == 2 * uint64_t(bands - 1) * pitch);
    if (pg.ow < 3 || pg.oh < 3) CHECK(bands == 1);
    const bool pieces = pitch > kSharpRowBytes;
    if (pieces) CHECK(rows <= kSharpKeepRows);
    // the chunk, halo areas included, within the bound -- but for the one view that does not fit it by itself, and the view in
    // pieces whose bands are capped
    const uint64_t chunk_bytes = pg.chunk * (view + halo);
    CHECK(chunk_bytes <= t.stage_bytes);
    if (pg.chunk > 1) CHECK(chunk_bytes <= samples);
    if (view <= samples && !(pieces && pg.oh > kSharpKeepRows)) CHECK(chunk_bytes <= samples);
    if (view >= samples && !(pieces && pg.oh > kSharpKeepRows)) CHECK(bands == 1 && halo == 0);  // the worst case needs no byte beyond the view
    if (pg.ow >= 3 && pg.oh >= 3 && view + photo_sharp_halo_bytes(pg.ow, pg.oh, c, std::min(pg.oh, kSharpBandRows)) <= samples) CHECK(rows == std::min(pg.oh, kSharpBandRows));
    // the addresses: view i of a chunk at i * view, its halo area at chunk * view + i * halo, pair j of rows there at j * 2 * pitch,
    // copied from rows (j + 1) * rows - 1 and (j + 1) * rows of the view
    const uint64_t halo_at = uint64_t(pg.chunk) * view;
    CHECK(pg.halo_at == (halo ? halo_at : kPhotoNoHalo));  // (the planner's offset is this sum, or none where nothing is saved)
    for (uint32_t i : {0u, pg.chunk - 1}) {
        for (uint32_t j : {0u, bands > 1 ? bands - 2 : 0u}) {
            if (bands < 2) break;
            const uint64_t first_row = uint64_t(j + 1) * rows - 1;
            CHECK(first_row + 1 < pg.oh);
            CHECK(i * view + (first_row + 2) * pitch <= halo_at);
            CHECK(halo_at + i * halo + (uint64_t(j) + 1) * 2 * pitch <= t.stage_bytes);
        }
    }
    return 0;
}

int check_setup(uint32_t c, std::mt19937& rng) {
    const uint32_t n_groups = 1 + rng() % 3;
    std::vector<uint32_t> n(n_groups), ow(n_groups), oh(n_groups);
    std::vector<std::unique_ptr<llcomp_mi_photo_chain[]>> chains(n_groups);
    std::vector<llcomp_mi_photo_group> photo(n_groups);
    uint64_t largest = 1;
    for (uint32_t g = 0; g < n_groups; ++g) {
        n[g] = 1 + rng() % 20;
        const uint32_t small = rng() % 4;  // a quarter of the groups small, so that chunks of several views with halos come up
        ow[g] = 1 + rng() % (small ? 5000 : 120);
        oh[g] = 1 + rng() % (small ? 5000 : 120);
        chains[g] = random_chains(n[g], rng);
        photo[g] = llcomp_mi_photo_group{uint32_t(sizeof(llcomp_mi_photo_group)), chains[g].get()};
        largest = std::max<uint64_t>(largest, uint64_t(ow[g]) * oh[g] * c);
    }
    // bounds below, at and above the largest view, and far above it
    const uint64_t bounds[6] = {largest / 3 + 1, largest, largest + 1 + rng() % (largest / 8 + 1), largest + largest / 4, 3 * largest, 50 * largest};
    const uint64_t samples = bounds[rng() % 6];
    PhotoTail t;
    CHECK(photo_setup(c, samples, photo.data(), n_groups, n.data(), ow.data(), oh.data(), t) == LLCOMP_MI_OK);
    for (uint32_t g = 0; g < n_groups; ++g) {
        uint32_t steps = 0, sharp = 0, area = 0;
        for (uint32_t i = 0; i < n[g]; ++i) {
            steps = std::max(steps, chains[g][i].n_ops);
            for (uint32_t k = 0; k < chains[g][i].n_ops; ++k) {
                if (chains[g][i].ops[k].op == LLCOMP_MI_PHOTO_ADJUST_SHARPNESS) sharp |= 1u << k;
                if (chains[g][i].ops[k].op == LLCOMP_MI_PHOTO_GAUSSIAN_BLUR) area |= 1u << k;
            }
        }
        const PhotoGroup& pg = t.groups[g];
        CHECK(pg.active == (steps > 0));
        if (!pg.active) continue;
        CHECK(pg.steps == steps);
        for (uint32_t k = 0; k < LLCOMP_MI_PHOTO_MAX_OPS; ++k)
            CHECK(pg.step[k].has(PhotoKind::kSharp) == ((sharp >> k) & 1u) && pg.step[k].has(PhotoKind::kBlur) == ((area >> k) & 1u));
        CHECK(pg.n == n[g] && pg.ow == ow[g] && pg.oh == oh[g]);
        if (check_group(pg, t, c, samples)) return 1;
    }
    return 0;
}

// the worst cases by name: one view the size of the bound; a long row in pieces; the band rows' limits
int check_corners() {
    for (uint32_t c : {1u, 3u}) {
        llcomp_mi_photo_chain ch[40];
        std::memset(ch, 0, sizeof ch);
        for (auto& one : ch) {
            one.n_ops = 3;
            one.ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_INVERT, 0.0f};
            one.ops[1] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 1.7f};
            one.ops[2] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_INVERT, 0.0f};
        }
        const llcomp_mi_photo_group photo[1] = {{uint32_t(sizeof(llcomp_mi_photo_group)), ch}};
        const uint32_t ow[1] = {100}, oh[1] = {44};
        for (uint32_t frames : {1u, 2u, 3u}) {
            for (uint32_t views : {1u, 40u}) {
                const uint32_t n[1] = {views};
                const uint64_t samples = uint64_t(frames) * 100 * 44 * c;
                PhotoTail t;
                CHECK(photo_setup(c, samples, photo, 1, n, ow, oh, t) == LLCOMP_MI_OK);
                CHECK(t.stage_bytes <= samples);
                for (uint32_t k = 0; k < LLCOMP_MI_PHOTO_MAX_OPS; ++k) CHECK(t.groups[0].step[k].has(PhotoKind::kSharp) == (k == 1));
                if (check_group(t.groups[0], t, c, samples)) return 1;
                if (frames == 1) CHECK(t.groups[0].chunk == 1 && t.groups[0].sharp_rows == 44);
                if (frames == 3) CHECK(t.groups[0].sharp_rows == kSharpBandRows && t.groups[0].chunk == std::min(views, 2u));
            }
        }
        // rows of more than kSharpRowBytes: the band is capped, whatever the bound
        const uint32_t wide = kSharpRowBytes / c + 1;
        CHECK(photo_sharp_band_rows(wide, 3 * kSharpKeepRows, c, 1) == kSharpKeepRows);
        CHECK(photo_sharp_band_rows(wide - 1, 3 * kSharpKeepRows, c, 1) == 3 * kSharpKeepRows);
        CHECK(photo_sharp_band_rows(wide, 100, c, 1) == 100 && photo_sharp_band_rows(wide, 100, c, ~0ull) == kSharpBandRows);
        CHECK(photo_sharp_band_rows(2, 5000, c, ~0ull) == 5000 && photo_sharp_band_rows(5000, 2, c, ~0ull) == 2);
        CHECK(photo_sharp_band_rows(1000000u, 1000000u, c, ~0ull) == kSharpBandRows);
        CHECK(photo_sharp_band_rows(1000000u, 1000000u, c, 7) == kSharpKeepRows);
    }
    return 0;
}

int check_reference(uint32_t w, uint32_t h, uint32_t c, std::mt19937& rng) {
    const size_t bytes = size_t(w) * h * c;
    std::unique_ptr<uint8_t[]> img(new uint8_t[bytes]), out(new uint8_t[bytes]), twice(new uint8_t[bytes]);
    const uint32_t kind = rng() % 3;  // noise, a constant, black and white
    for (size_t i = 0; i < bytes; ++i) img[i] = kind == 0 ? uint8_t(rng()) : kind == 1 ? uint8_t(77) : uint8_t((i / c + i / c / w) % 2 ? 0 : 255);
    const std::unique_ptr<llcomp_mi_photo_chain[]> ch = random_chains(1, rng);
    if (ch[0].n_ops) ch[0].ops[rng() % ch[0].n_ops] = random_op(rng, true);
    CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, ch[0].ops, ch[0].n_ops, out.get()) == LLCOMP_MI_OK);
    std::memcpy(twice.get(), img.get(), bytes);
    CHECK(llcomp_mi_photo_reference(twice.get(), w, h, c, ch[0].ops, ch[0].n_ops, twice.get()) == LLCOMP_MI_OK);  // in place
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    std::memcpy(twice.get(), img.get(), bytes);  // op by op is the chain
    for (uint32_t k = 0; k < ch[0].n_ops; ++k) CHECK(llcomp_mi_photo_reference(twice.get(), w, h, c, ch[0].ops + k, 1, twice.get()) == LLCOMP_MI_OK);
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    // a factor of 1, a constant image and a view with a side below 3 come back as they are; a factor of 0 is the smooth value itself
    const llcomp_mi_photo_op one = {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 1.0f}, zero = {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 0.0f}, big = {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 256.0f};
    CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, &one, 1, out.get()) == LLCOMP_MI_OK && !std::memcmp(out.get(), img.get(), bytes));
    CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, &big, 1, out.get()) == LLCOMP_MI_OK);
    if (kind == 1 || w < 3 || h < 3) CHECK(!std::memcmp(out.get(), img.get(), bytes));
    CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, &zero, 1, out.get()) == LLCOMP_MI_OK);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            for (uint32_t k = 0; k < c; ++k) {
                const size_t at = (size_t(y) * w + x) * c + k;
                uint32_t want = img[at];
                if (photo_smooth_interior(x, y, w, h)) {
                    uint32_t sum9 = 0;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) sum9 += img[(size_t(int64_t(y) + dy) * w + size_t(int64_t(x) + dx)) * c + k];
                    want = photo_smooth(sum9, img[at]);
                }
                CHECK(out[at] == want);
            }
    return 0;
}

int check_rule() {
    for (uint32_t v = 0; v < 256; ++v) CHECK(photo_smooth(9 * v, v) == v);  // a constant window stays
    CHECK(photo_smooth(0, 0) == 0 && photo_smooth(9 * 255, 255) == 255 && photo_smooth(8 * 255, 0) == 157 && photo_smooth(255, 255) == 98);
    // the float form is never nearer than 1 / 26 to an integer: (S + 6.5) / 13 over every S
    for (uint32_t s = 0; s <= 13 * 255; ++s) {
        const double q = (double(s) + 6.5) / 13.0, fl = std::floor(q);
        CHECK(uint32_t(fl) == (s + 6) / 13 && q - fl >= 1.0 / 26.0 - 1e-12 && fl + 1.0 - q >= 1.0 / 26.0 - 1e-12);
    }
    CHECK(photo_smooth_interior(1, 1, 3, 3) && !photo_smooth_interior(0, 1, 3, 3) && !photo_smooth_interior(2, 1, 3, 3) && !photo_smooth_interior(1, 0, 3, 3) &&
          !photo_smooth_interior(1, 2, 3, 3) && !photo_smooth_interior(0, 0, 1, 1) && !photo_smooth_interior(1, 1, 2, 9) && !photo_smooth_interior(1, 1, 9, 2));
    CHECK(photo_kind(LLCOMP_MI_PHOTO_ADJUST_SHARPNESS) == PhotoKind::kSharp && !photo_needs_stats(LLCOMP_MI_PHOTO_ADJUST_SHARPNESS) &&
          photo_kind(LLCOMP_MI_PHOTO_GAUSSIAN_BLUR) == PhotoKind::kBlur && photo_kind(18) == PhotoKind::kPixel);
    return 0;
}

int check_refusals() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const llcomp_mi_photo_op bad[7] = {{LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, -1e-3f}, {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 256.5f}, {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, nan},
                                       {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, inf},    {LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, -inf},   {18u, 1.0f},
                                       {20u, 1.0f}};
    const uint32_t n[1] = {2}, ow[1] = {8}, oh[1] = {8};
    std::unique_ptr<uint8_t[]> img(new uint8_t[8 * 8 * 3]), out(new uint8_t[8 * 8 * 3]);
    std::memset(img.get(), 9, 8 * 8 * 3);
    for (const llcomp_mi_photo_op& b : bad) {
        llcomp_mi_photo_chain ch[2] = {};
        ch[0].n_ops = 1;
        ch[0].ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 1.5f};
        ch[1].n_ops = 2;
        ch[1].ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_INVERT, 0.0f};
        ch[1].ops[1] = b;
        const llcomp_mi_photo_group photo[1] = {{uint32_t(sizeof(llcomp_mi_photo_group)), ch}};
        PhotoTail t;
        CHECK(photo_setup(3, 1000, photo, 1, n, ow, oh, t) == LLCOMP_MI_BAD_ARGS);
        CHECK(!photo_op_ok(b.op, b.param));
        std::memset(out.get(), 0x5A, 8 * 8 * 3);
        CHECK(llcomp_mi_photo_reference(img.get(), 8, 8, 3, ch[1].ops, 2, out.get()) == LLCOMP_MI_BAD_ARGS);
        for (size_t i = 0; i < 8 * 8 * 3; ++i) CHECK(out[i] == 0x5A);
    }
    CHECK(photo_op_ok(LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 0.0f) && photo_op_ok(LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 256.0f));
    llcomp_mi_photo_chain ok = {};
    ok.n_ops = 1;
    ok.ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_SHARPNESS, 2.0f};
    CHECK(photo_check_chain(ok, 1) == LLCOMP_MI_OK && photo_check_chain(ok, 3) == LLCOMP_MI_OK && photo_check_chain(ok, 4) == LLCOMP_MI_BAD_ARGS);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20241019);
    unsigned rounds = 0;
    for (uint32_t c : {1u, 3u})
        for (int i = 0; i < 400; ++i, ++rounds)
            if (check_setup(c, rng)) return 1;
    for (uint32_t c : {1u, 3u})
        for (int i = 0; i < 150; ++i, ++rounds)
            if (check_reference(1 + rng() % 80, 1 + rng() % 40, c, rng)) return 1;
    if (check_corners() || check_rule() || check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
