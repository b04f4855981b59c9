// photo_plan_check.cpp -- the host planner of the photometric chains (llcomp_amd/csrc/photo_plan.hpp) and the rule's host functions
// (photo_rule.hpp, llcomp_mi_photo_reference) under a sanitizer: seeded random groups with chains read from heap arrays of exactly
// n_views chains -- the block put into a heap buffer of exactly its size and within the bound the codec sizes its staging buffer by,
// every chunk within the staging bound and within what the statistics and tables are allocated for, the record of every step that of
// the chains' ops, kind by kind -- the reference with image and output in heap buffers of exactly their sizes, in place too, and the refusals.  Host code
// only; built and run by tests/test_photo_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/photo_plan_check.cpp llcomp_amd/csrc/photo_plan.cpp
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
    o.op = rng() % LLCOMP_MI_PHOTO_OP_COUNT;
    const float factors[5] = {0.0f, 1.0f, 0.37f, 2.75f, 256.0f};
    o.param = o.op == LLCOMP_MI_PHOTO_SOLARIZE ? float(rng() % 257) : o.op == LLCOMP_MI_PHOTO_POSTERIZE ? float(1 + rng() % 8) : factors[rng() % 5];
    return o;
}

int check_setup(uint32_t c, uint64_t samples, std::mt19937& rng) {
    const uint32_t n_groups = 1 + rng() % 4;
    std::vector<uint32_t> n(n_groups), ow(n_groups), oh(n_groups);
    std::vector<std::unique_ptr<llcomp_mi_photo_chain[]>> chains(n_groups);
    std::vector<llcomp_mi_photo_group> photo(n_groups);
    uint64_t total = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        n[g] = 1 + rng() % 40;
        ow[g] = 1 + rng() % 64;
        oh[g] = 1 + rng() % 48;
        total += n[g];
        const uint32_t kind = rng() % 4;  // no chains, all empty, or chains
        if (kind) chains[g] = heap_chains(n[g], rng, random_op, kind == 1);
        photo[g] = llcomp_mi_photo_group{uint32_t(sizeof(llcomp_mi_photo_group)), chains[g].get()};
    }
    PhotoTail t;
    CHECK(photo_setup(c, samples, photo.data(), n_groups, n.data(), ow.data(), oh.data(), t) == LLCOMP_MI_OK);
    CHECK(t.groups.size() == n_groups && t.bytes() <= photo_tables_bound(total));
    std::unique_ptr<uint8_t[]> block(new uint8_t[t.bytes() ? t.bytes() : 1]);
    t.put(block.get());
    uint64_t at = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const PhotoGroup& pg = t.groups[g];
        uint32_t steps = 0, stats = 0, kinds[4] = {};  // bit k: some view's op k reads statistics / is of the kind
        if (chains[g])
            for (uint32_t i = 0; i < n[g]; ++i) {
                steps = std::max(steps, chains[g][i].n_ops);
                for (uint32_t k = 0; k < chains[g][i].n_ops; ++k) {
                    if (photo_needs_stats(chains[g][i].ops[k].op)) stats |= 1u << k;
                    kinds[uint32_t(photo_kind(chains[g][i].ops[k].op))] |= 1u << k;
                }
            }
        CHECK(pg.active == (steps > 0));
        if (!pg.active) continue;
        CHECK(pg.steps == steps && pg.n == n[g] && pg.ow == ow[g] && pg.oh == oh[g]);
        for (uint32_t k = 0; k < LLCOMP_MI_PHOTO_MAX_OPS; ++k) {  // (beyond the longest chain: nothing)
            CHECK(pg.step[k].stats == ((stats >> k) & 1u));
            for (PhotoKind kind : {PhotoKind::kPixel, PhotoKind::kTable, PhotoKind::kBlur, PhotoKind::kSharp})
                CHECK(pg.step[k].has(kind) == ((kinds[uint32_t(kind)] >> k) & 1u));
        }
        CHECK(pg.sharp_rows == 0 && pg.halo_at == kPhotoNoHalo);  // (this program's ops are the pointwise family)
        CHECK(pg.first == at && pg.chunk >= 1 && pg.chunk <= pg.n && pg.chunk <= t.tab_views);
        const uint64_t per_view = uint64_t(oh[g]) * ow[g] * c;
        CHECK(pg.chunk * per_view <= t.stage_bytes && (pg.chunk == 1 || pg.chunk * per_view <= samples));
        CHECK(pg.chunk == pg.n || (pg.chunk + 1) * per_view > samples);  // (as many views as fit)
        for (uint32_t i = 0; i < n[g]; ++i) {  // the block: every chain where the kernels look for it, nothing of the 0xEE behind its ops
            llcomp_mi_photo_chain got;
            std::memcpy(&got, block.get() + (at + i) * sizeof got, sizeof got);
            CHECK(got.n_ops == chains[g][i].n_ops && !std::memcmp(got.ops, chains[g][i].ops, got.n_ops * sizeof(llcomp_mi_photo_op)));
            for (uint32_t k = got.n_ops; k < LLCOMP_MI_PHOTO_MAX_OPS; ++k) CHECK(got.ops[k].op == 0);
        }
        at += n[g];
    }
    CHECK(at * sizeof(llcomp_mi_photo_chain) == t.bytes());
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
    // op by op is the chain
    std::memcpy(twice.get(), img.get(), bytes);
    for (uint32_t k = 0; k < ch[0].n_ops; ++k) CHECK(llcomp_mi_photo_reference(twice.get(), w, h, c, ch[0].ops + k, 1, twice.get()) == LLCOMP_MI_OK);
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    return 0;
}

int check_refusals() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const llcomp_mi_photo_op bad[] = {{LLCOMP_MI_PHOTO_BRIGHTNESS, nan}, {LLCOMP_MI_PHOTO_CONTRAST, inf}, {LLCOMP_MI_PHOTO_COLOR, -0.5f},
                                      {LLCOMP_MI_PHOTO_BRIGHTNESS, 256.5f}, {LLCOMP_MI_PHOTO_SOLARIZE, 1.5f}, {LLCOMP_MI_PHOTO_SOLARIZE, 257.0f},
                                      {LLCOMP_MI_PHOTO_SOLARIZE, -1.0f}, {LLCOMP_MI_PHOTO_POSTERIZE, 0.0f}, {LLCOMP_MI_PHOTO_POSTERIZE, 9.0f},
                                      {LLCOMP_MI_PHOTO_POSTERIZE, 2.5f}, {LLCOMP_MI_PHOTO_POSTERIZE, nan}, {LLCOMP_MI_PHOTO_OP_COUNT, 1.0f},
                                      {0xFFFFFFFFu, 1.0f}, {LLCOMP_MI_PHOTO_SOLARIZE, 3e9f}, {LLCOMP_MI_PHOTO_POSTERIZE, -3e9f}};
    const uint32_t n[2] = {2, 1}, ow[2] = {8, 8}, oh[2] = {8, 8};
    for (const llcomp_mi_photo_op& b : bad) {
        llcomp_mi_photo_chain good{}, ch[2] = {};
        good.n_ops = 1;
        good.ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_INVERT, 0.0f};
        ch[0] = good;
        ch[1].n_ops = 3;
        ch[1].ops[0] = ch[1].ops[1] = good.ops[0];
        ch[1].ops[2] = b;
        const llcomp_mi_photo_group photo[2] = {{uint32_t(sizeof(llcomp_mi_photo_group)), ch}, {uint32_t(sizeof(llcomp_mi_photo_group)), &good}};
        PhotoTail t;
        CHECK(photo_setup(3, 1000, photo, 2, n, ow, oh, t) == LLCOMP_MI_BAD_ARGS);
        CHECK(!photo_op_ok(b.op, b.param));
    }
    llcomp_mi_photo_chain nine{}, inv{};
    nine.n_ops = LLCOMP_MI_PHOTO_MAX_OPS + 1;
    inv.n_ops = 1;
    inv.ops[0] = llcomp_mi_photo_op{LLCOMP_MI_PHOTO_INVERT, 0.0f};
    CHECK(photo_check_chain(nine, 3) == LLCOMP_MI_BAD_ARGS && photo_check_chain(inv, 3) == LLCOMP_MI_OK && photo_check_chain(inv, 1) == LLCOMP_MI_OK);
    CHECK(photo_check_chain(inv, 2) == LLCOMP_MI_BAD_ARGS && photo_check_chain(inv, 4) == LLCOMP_MI_BAD_ARGS);
    CHECK(photo_check_chain(llcomp_mi_photo_chain{}, 4) == LLCOMP_MI_OK);  // (an empty chain on any c)
    PhotoTail t;
    const llcomp_mi_photo_group wrong[1] = {{uint32_t(sizeof(llcomp_mi_photo_group)) + 8, &inv}};
    CHECK(photo_setup(3, 1000, wrong, 1, n + 1, ow, oh, t) == LLCOMP_MI_BAD_ARGS);
    CHECK(photo_setup(3, 1000, nullptr, 2, n, ow, oh, t) == LLCOMP_MI_OK && !t.any() && t.groups.size() == 2 && !t.bytes());
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    unsigned rounds = 0;
    for (uint32_t c : {1u, 3u})
        for (uint64_t samples : {uint64_t(1), uint64_t(3 * 100 * 44 * 3), uint64_t(1) << 40})
            for (int i = 0; i < 100; ++i, ++rounds)
                if (check_setup(c, samples, rng)) return 1;
    for (uint32_t c : {1u, 3u})
        for (int i = 0; i < 100; ++i, ++rounds)
            if (check_reference(1 + rng() % 40, 1 + rng() % 40, c, rng)) return 1;
    if (check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
