// photo_area_check.cpp -- GAUSSIAN_BLUR and ADJUST_HUE of the photometric chains on the host under a sanitizer: the planner
// (llcomp_amd/csrc/photo_plan.hpp: photo_setup, with the blur in its record of every step) over seeded groups whose chains lie in heap arrays of exactly
// n_views chains, llcomp_mi_photo_reference with image and output in heap buffers of exactly their sizes -- out of place, in place, op by
// op -- on chains that mix the two ops with the pointwise family, the rule's functions at the ends of their domains, and the
// refusals.  Host code only; built and run by tests/test_photo_area_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/photo_area_check.cpp llcomp_amd/csrc/photo_plan.cpp
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

llcomp_mi_photo_op random_op(std::mt19937& rng) {
    llcomp_mi_photo_op o;
    const uint32_t kind = rng() % 4;
    if (kind == 0) {
        const float radii[7] = {0.0f, 1e-4f, 0.1f, 1.0f, 2.0f, 11.5f, 32.0f};
        return llcomp_mi_photo_op{LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, radii[rng() % 7]};
    }
    if (kind == 1) {
        const float factors[7] = {0.0f, 0.5f, -0.5f, 0.1f, -0.1f, 1.0f / 255.0f, -1.0f / 255.0f};
        return llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_HUE, factors[rng() % 7]};
    }
    o.op = rng() % LLCOMP_MI_PHOTO_OP_COUNT;
    const float factors[4] = {0.0f, 1.0f, 0.37f, 2.75f};
    o.param = o.op == LLCOMP_MI_PHOTO_SOLARIZE ? float(rng() % 257) : o.op == LLCOMP_MI_PHOTO_POSTERIZE ? float(1 + rng() % 8) : factors[rng() % 4];
    return o;
}

int check_setup(uint32_t c, std::mt19937& rng) {
    const uint32_t n_groups = 1 + rng() % 3;
    std::vector<uint32_t> n(n_groups), ow(n_groups), oh(n_groups);
    std::vector<std::unique_ptr<llcomp_mi_photo_chain[]>> chains(n_groups);
    std::vector<llcomp_mi_photo_group> photo(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) {
        n[g] = 1 + rng() % 20;
        ow[g] = 1 + rng() % 5000;  // (no side limit: any width and height is taken)
        oh[g] = 1 + rng() % 5000;
        chains[g] = heap_chains(n[g], rng, random_op);
        photo[g] = llcomp_mi_photo_group{uint32_t(sizeof(llcomp_mi_photo_group)), chains[g].get()};
    }
    PhotoTail t;
    CHECK(photo_setup(c, 3 * 100 * 44 * 3, photo.data(), n_groups, n.data(), ow.data(), oh.data(), t) == LLCOMP_MI_OK);
    for (uint32_t g = 0; g < n_groups; ++g) {
        uint32_t steps = 0, stats = 0, table = 0, area = 0;
        for (uint32_t i = 0; i < n[g]; ++i) {
            steps = std::max(steps, chains[g][i].n_ops);
            for (uint32_t k = 0; k < chains[g][i].n_ops; ++k) {
                const uint32_t op = chains[g][i].ops[k].op;
                if (op == LLCOMP_MI_PHOTO_CONTRAST || op == LLCOMP_MI_PHOTO_AUTOCONTRAST || op == LLCOMP_MI_PHOTO_EQUALIZE) stats |= 1u << k;
                if (op < LLCOMP_MI_PHOTO_OP_COUNT && op != LLCOMP_MI_PHOTO_COLOR && op != LLCOMP_MI_PHOTO_GRAYSCALE) table |= 1u << k;
                if (op == LLCOMP_MI_PHOTO_GAUSSIAN_BLUR) area |= 1u << k;
            }
        }
        const PhotoGroup& pg = t.groups[g];
        CHECK(pg.active == (steps > 0));
        if (!pg.active) continue;
        CHECK(pg.steps == steps);
        for (uint32_t k = 0; k < LLCOMP_MI_PHOTO_MAX_OPS; ++k) {
            const PhotoStepInfo& st = pg.step[k];
            CHECK(st.stats == ((stats >> k) & 1u) && st.has(PhotoKind::kTable) == ((table >> k) & 1u) && st.has(PhotoKind::kBlur) == ((area >> k) & 1u));
            CHECK(!st.has(PhotoKind::kSharp));
        }
        CHECK(pg.n == n[g] && pg.ow == ow[g] && pg.oh == oh[g] && pg.chunk >= 1 && pg.chunk <= pg.n);
    }
    return 0;
}

int check_reference(uint32_t w, uint32_t h, uint32_t c, std::mt19937& rng) {
    const size_t bytes = size_t(w) * h * c;
    std::unique_ptr<uint8_t[]> img(new uint8_t[bytes]), out(new uint8_t[bytes]), twice(new uint8_t[bytes]);
    const uint32_t kind = rng() % 3;  // noise, a constant, two values
    for (size_t i = 0; i < bytes; ++i) img[i] = kind == 0 ? uint8_t(rng()) : kind == 1 ? uint8_t(77) : uint8_t(i % 7 ? 10 : 200);
    const std::unique_ptr<llcomp_mi_photo_chain[]> ch = heap_chains(1, rng, random_op);
    CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, ch[0].ops, ch[0].n_ops, out.get()) == LLCOMP_MI_OK);
    std::memcpy(twice.get(), img.get(), bytes);
    CHECK(llcomp_mi_photo_reference(twice.get(), w, h, c, ch[0].ops, ch[0].n_ops, twice.get()) == LLCOMP_MI_OK);  // in place
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    std::memcpy(twice.get(), img.get(), bytes);  // op by op is the chain
    for (uint32_t k = 0; k < ch[0].n_ops; ++k) CHECK(llcomp_mi_photo_reference(twice.get(), w, h, c, ch[0].ops + k, 1, twice.get()) == LLCOMP_MI_OK);
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    if (kind == 1) {  // a constant image: the blur and, its channels being equal, the hue leave it as it is
        const llcomp_mi_photo_op two[2] = {{LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 7.5f}, {LLCOMP_MI_PHOTO_ADJUST_HUE, 0.3f}};
        CHECK(llcomp_mi_photo_reference(img.get(), w, h, c, two, 2, out.get()) == LLCOMP_MI_OK && !std::memcmp(out.get(), img.get(), bytes));
    }
    return 0;
}

int check_rule() {
    uint32_t r, ww, fw;
    photo_blur_weights(0.0f, r, ww, fw);
    CHECK(r == 0 && ww == (1u << 24) && fw == 0);
    for (uint32_t v = 0; v < 256; ++v) CHECK(photo_blur_tap(v, 2 * v, ww, fw) == v);  // radius 0: the identity
    photo_blur_weights(1.0f, r, ww, fw);
    CHECK(r == 0 && ww == 11184811u && fw == 2796202u);
    photo_blur_weights(2.0f, r, ww, fw);
    CHECK(r == 1 && ww == 4473924u && fw == 1677722u);
    photo_blur_weights(float(LLCOMP_MI_PHOTO_MAX_RADIUS), r, ww, fw);
    CHECK(r <= LLCOMP_MI_PHOTO_MAX_RADIUS && photo_blur_reach(r) <= 3 * (LLCOMP_MI_PHOTO_MAX_RADIUS + 1));
    for (uint32_t v = 0; v < 256; ++v) CHECK(photo_blur_tap((2 * r + 1) * v, 2 * v, ww, fw) == v);  // a constant line stays constant
    CHECK(photo_hue_shift(0.5f) == 127 && photo_hue_shift(-0.5f) == 129 && photo_hue_shift(0.0f) == 0 && photo_hue_shift(-1.0f / 255.0f) == 255);
    // every gray survives the round trip under any shift; a seventh of all 2^24 triples, as RGB and as HSV, give bytes
    for (uint32_t v = 0; v < 256; ++v) {
        uint32_t a = v, b = v, d = v;
        photo_hue(a, b, d, 77);
        CHECK(a == v && b == v && d == v);
    }
    for (uint32_t rgb = 0; rgb < (1u << 24); rgb += 7) {
        uint32_t a = rgb >> 16, b = (rgb >> 8) & 255u, d = rgb & 255u, hh, ss, vv;
        photo_rgb2hsv(a, b, d, hh, ss, vv);
        CHECK(hh < 256 && ss < 256 && vv < 256);
        photo_hsv2rgb(a, b, d, hh, ss, vv);  // (the triple read as HSV)
        CHECK(hh < 256 && ss < 256 && vv < 256);
    }
    return 0;
}

int check_refusals() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<llcomp_mi_photo_op> bad = {{LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, -1e-3f}, {LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 32.5f}, {LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, nan},
                                           {LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, inf},    {LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, -inf},  {LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 3e9f},
                                           {LLCOMP_MI_PHOTO_ADJUST_HUE, 0.5001f},   {LLCOMP_MI_PHOTO_ADJUST_HUE, -0.5001f}, {LLCOMP_MI_PHOTO_ADJUST_HUE, nan},
                                           {LLCOMP_MI_PHOTO_ADJUST_HUE, inf},       {LLCOMP_MI_PHOTO_ADJUST_HUE, -inf},     {18u, 0.0f}};
    for (uint32_t code = LLCOMP_MI_PHOTO_OP_COUNT; code < LLCOMP_MI_PHOTO_GAUSSIAN_BLUR; ++code) bad.push_back(llcomp_mi_photo_op{code, 0.0f});
    const uint32_t n[1] = {2}, ow[1] = {8}, oh[1] = {8};
    std::unique_ptr<uint8_t[]> img(new uint8_t[8 * 8 * 3]), out(new uint8_t[8 * 8 * 3]);
    std::memset(img.get(), 9, 8 * 8 * 3);
    for (const llcomp_mi_photo_op& b : bad) {
        llcomp_mi_photo_chain ch[2] = {};
        ch[0].n_ops = 1;
        ch[0].ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 1.0f};
        ch[1].n_ops = 2;
        ch[1].ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_ADJUST_HUE, 0.25f};
        ch[1].ops[1] = b;
        const llcomp_mi_photo_group photo[1] = {{uint32_t(sizeof(llcomp_mi_photo_group)), ch}};
        PhotoTail t;
        CHECK(photo_setup(3, 1000, photo, 1, n, ow, oh, t) == LLCOMP_MI_BAD_ARGS);
        CHECK(!photo_op_ok(b.op, b.param));
        std::memset(out.get(), 0x5A, 8 * 8 * 3);
        CHECK(llcomp_mi_photo_reference(img.get(), 8, 8, 3, ch[1].ops, 2, out.get()) == LLCOMP_MI_BAD_ARGS);
        for (size_t i = 0; i < 8 * 8 * 3; ++i) CHECK(out[i] == 0x5A);
    }
    CHECK(photo_kind(LLCOMP_MI_PHOTO_GAUSSIAN_BLUR) == PhotoKind::kBlur && photo_kind(LLCOMP_MI_PHOTO_ADJUST_HUE) == PhotoKind::kPixel);
    for (uint32_t op : {uint32_t(LLCOMP_MI_PHOTO_GAUSSIAN_BLUR), uint32_t(LLCOMP_MI_PHOTO_ADJUST_HUE)}) CHECK(!photo_needs_stats(op));
    CHECK(photo_op_ok(LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 0.0f) && photo_op_ok(LLCOMP_MI_PHOTO_GAUSSIAN_BLUR, 32.0f));
    CHECK(photo_op_ok(LLCOMP_MI_PHOTO_ADJUST_HUE, 0.5f) && photo_op_ok(LLCOMP_MI_PHOTO_ADJUST_HUE, -0.5f));
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20240917);
    unsigned rounds = 0;
    for (uint32_t c : {1u, 3u})
        for (int i = 0; i < 100; ++i, ++rounds)
            if (check_setup(c, rng)) return 1;
    for (uint32_t c : {1u, 3u})
        for (int i = 0; i < 150; ++i, ++rounds)
            if (check_reference(1 + rng() % 80, 1 + rng() % 40, c, rng)) return 1;
    if (check_rule() || check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
