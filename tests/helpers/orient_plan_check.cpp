// orient_plan_check.cpp -- the host half of the batch orientation (llcomp_amd/csrc/orient_plan.hpp) and the rule's host functions
// (orient_rule.hpp, llcomp_mi_orient_reference) under a sanitizer: the table of seeded codes read from heap arrays of exactly n bytes,
// the reference with batch and output in heap buffers of exactly their sizes, out of place and in place, on arbitrary bit patterns,
// against the rule applied pixel by pixel here; the fundamental domains, whose pixels and their images have to be every pixel that
// moves, each once; and the refusals.  Host code only; built and run by tests/test_orient_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/orient_plan_check.cpp llcomp_amd/csrc/orient_plan.cpp
// Prints "ok <rounds>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "orient_plan.hpp"
#include "orient_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace {

// n codes on the heap, exactly: kind 0 all zeros, 1 all of one code, 2 drawn (among the shape-keeping codes where square is false)
std::unique_ptr<uint8_t[]> heap_codes(uint32_t n, uint32_t kind, bool square, std::mt19937& rng) {
    static const uint8_t keeps[4] = {0, 1, 2, 4};
    std::unique_ptr<uint8_t[]> codes(new uint8_t[n]);
    const uint8_t one = square ? uint8_t(1 + rng() % 7) : keeps[1 + rng() % 3];
    for (uint32_t i = 0; i < n; ++i) codes[i] = kind == 0 ? 0 : kind == 1 ? one : square ? uint8_t(rng() % 8) : keeps[rng() % 4];
    return codes;
}

int check_table(uint32_t n, uint32_t kind, std::mt19937& rng) {
    const std::unique_ptr<uint8_t[]> codes = heap_codes(n, kind, true, rng);
    CHECK(orient_check_call(n, 3, 8, 8, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, codes.get()) == LLCOMP_MI_OK);
    std::vector<OrientEntry> table;
    orient_table(n, codes.get(), table);
    CHECK(table.size() * sizeof(OrientEntry) <= orient_table_bound(n));
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!codes[i]) continue;
        CHECK(at < table.size() && table[at].sample == i && table[at].code == codes[i]);
        ++at;
    }
    CHECK(at == table.size() && (kind != 0 || table.empty()) && (kind != 1 || table.size() == n));
    return 0;
}

int check_reference(uint32_t dtype, uint32_t layout, std::mt19937& rng) {
    const bool square = rng() % 2;
    const uint32_t n = 1 + rng() % 9, c = rng() % 2 ? 3 : 1, ow = 1 + rng() % 9, oh = square ? ow : 1 + rng() % 7, es = batch_esize(dtype);
    const size_t bytes = size_t(n) * c * ow * oh * es;
    const std::unique_ptr<uint8_t[]> codes = heap_codes(n, 2, ow == oh, rng);
    std::unique_ptr<uint8_t[]> batch(new uint8_t[bytes]), out(new uint8_t[bytes]), twice(new uint8_t[bytes]);
    for (size_t i = 0; i < bytes; ++i) batch[i] = uint8_t(rng());  // (any bit pattern: NaNs, infinities and subnormals among them)
    CHECK(llcomp_mi_orient_reference(batch.get(), n, c, ow, oh, dtype, layout, codes.get(), out.get()) == LLCOMP_MI_OK);
    std::memcpy(twice.get(), batch.get(), bytes);
    CHECK(llcomp_mi_orient_reference(twice.get(), n, c, ow, oh, dtype, layout, codes.get(), twice.get()) == LLCOMP_MI_OK);  // in place
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t ch = 0; ch < c; ++ch)
            for (uint32_t y = 0; y < oh; ++y)
                for (uint32_t x = 0; x < ow; ++x) {
                    const OrientXY s = orient_src(codes[i], ow, oh, x, y);
                    CHECK(s.x < ow && s.y < oh);
                    const size_t to = chw ? ((size_t(i) * c + ch) * oh + y) * ow + x : ((size_t(i) * oh + y) * ow + x) * c + ch;
                    const size_t from = chw ? ((size_t(i) * c + ch) * oh + s.y) * ow + s.x : ((size_t(i) * oh + s.y) * ow + s.x) * c + ch;
                    CHECK(!std::memcmp(out.get() + to * es, batch.get() + from * es, es));
                }
    return 0;
}

// The domain's pixels and their images under the powers of the map: every pixel that moves, once; no pixel that is its own image; and
// what orient_rect_in_domain and orient_rect_src say of every rectangle of a small box is what their pixels say
int check_domains() {
    for (uint32_t code = 1; code < kOrientCodes; ++code)
        for (uint32_t ow = 1; ow <= 9; ++ow)
            for (uint32_t oh = 1; oh <= 9; ++oh) {
                if (orient_transposes(code) && ow != oh) continue;
                std::unique_ptr<uint8_t[]> hits(new uint8_t[ow * oh]);
                std::memset(hits.get(), 0, ow * oh);
                const OrientXY box = orient_domain_box(code, ow, oh);
                const uint32_t order = orient_order(code);
                CHECK(box.x <= ow && box.y <= oh);
                for (uint32_t y = 0; y < box.y; ++y)
                    for (uint32_t x = 0; x < box.x; ++x) {
                        if (!orient_in_domain(code, ow, oh, x, y)) continue;
                        OrientXY p = {x, y};
                        for (uint32_t k = 0; k < order; ++k) {
                            const OrientXY q = orient_src(orient_power(code, k), ow, oh, x, y);
                            CHECK(q.x == p.x && q.y == p.y);  // the k-th power is the map applied k times
                            ++hits[p.y * ow + p.x];
                            p = orient_src(code, ow, oh, p.x, p.y);
                        }
                        CHECK(p.x == x && p.y == y);
                    }
                for (uint32_t y = 0; y < oh; ++y)
                    for (uint32_t x = 0; x < ow; ++x) {
                        const OrientXY s = orient_src(code, ow, oh, x, y);
                        CHECK(hits[y * ow + x] == ((s.x == x && s.y == y) ? 0 : 1));
                    }
                if (ow > 6 || oh > 6) continue;
                for (uint32_t y0 = 0; y0 < box.y; ++y0)
                    for (uint32_t y1 = y0 + 1; y1 <= box.y; ++y1)
                        for (uint32_t x0 = 0; x0 < box.x; ++x0)
                            for (uint32_t x1 = x0 + 1; x1 <= box.x; ++x1) {
                                const OrientRect r = {x0, y0, x1, y1};
                                const OrientRect im = orient_rect_src(code, ow, oh, r);
                                uint32_t in = 0, all = 0;
                                for (uint32_t y = y0; y < y1; ++y)
                                    for (uint32_t x = x0; x < x1; ++x, ++all) {
                                        in += orient_in_domain(code, ow, oh, x, y);
                                        const OrientXY s = orient_src(code, ow, oh, x, y);
                                        CHECK(s.x >= im.x0 && s.x < im.x1 && s.y >= im.y0 && s.y < im.y1);
                                    }
                                CHECK((im.x1 - im.x0) * (im.y1 - im.y0) == all);
                                const uint32_t says = orient_rect_in_domain(code, ow, oh, r);
                                CHECK(says == (in == all ? 2u : in ? 1u : 0u));
                            }
            }
    return 0;
}

int check_refusals() {
    std::mt19937 rng(3);
    const uint32_t n = 5, ow = 6, oh = 6;
    const size_t el = size_t(n) * 3 * ow * oh;
    std::unique_ptr<float[]> out(new float[el]), batch(new float[el]);
    std::fill(batch.get(), batch.get() + el, 1.0f);
    std::fill(out.get(), out.get() + el, 7.0f);
    const std::unique_ptr<uint8_t[]> ok = heap_codes(n, 2, true, rng);
    auto ref = [&](uint32_t n_, uint32_t c, uint32_t w, uint32_t h, uint32_t dtype, uint32_t layout, const uint8_t* codes) {
        return llcomp_mi_orient_reference(batch.get(), n_, c, w, h, dtype, layout, codes, out.get());
    };
    CHECK(ref(n, 3, ow, oh, 1, 1, nullptr) == LLCOMP_MI_BAD_ARGS);
    CHECK(ref(0, 3, ow, oh, 1, 1, ok.get()) == LLCOMP_MI_BAD_ARGS && ref(65536, 3, ow, oh, 1, 1, ok.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(ref(n, 0, ow, oh, 1, 1, ok.get()) == LLCOMP_MI_BAD_ARGS && ref(n, 3, 0, oh, 1, 1, ok.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(ref(n, 3, ow, 0, 1, 1, ok.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(ref(n, 3, ow, oh, 4, 1, ok.get()) == LLCOMP_MI_BAD_ARGS && ref(n, 3, ow, oh, 1, 2, ok.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_orient_reference(nullptr, n, 3, ow, oh, 1, 1, ok.get(), out.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_orient_reference(batch.get(), n, 3, ow, oh, 1, 1, ok.get(), nullptr) == LLCOMP_MI_BAD_ARGS);
    for (uint32_t bad : {8u, 9u, 255u}) {
        std::unique_ptr<uint8_t[]> codes = heap_codes(n, 2, true, rng);
        codes[n - 1] = uint8_t(bad);
        CHECK(ref(n, 3, ow, oh, 1, 1, codes.get()) == LLCOMP_MI_BAD_ARGS);
    }
    for (uint32_t code : {3u, 5u, 6u, 7u}) {  // 6 x 5 and 5 x 6: not square (the buffers are larger than that)
        std::unique_ptr<uint8_t[]> codes = heap_codes(n, 0, false, rng);
        codes[2] = uint8_t(code);
        CHECK(ref(n, 3, ow, oh - 1, 1, 1, codes.get()) == LLCOMP_MI_BAD_ARGS && ref(n, 3, ow - 1, oh, 1, 0, codes.get()) == LLCOMP_MI_BAD_ARGS);
    }
    for (size_t i = 0; i < el; ++i) CHECK(out[i] == 7.0f);
    CHECK(ref(n, 3, ow, oh, 1, 1, ok.get()) == LLCOMP_MI_OK);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20241020);
    unsigned rounds = 0;
    CHECK(llcomp_mi_orient_tile() == kOrientTile && kOrientTile >= 8);
    for (uint32_t kind = 0; kind < 3; ++kind) {
        for (uint32_t n : {1u, 2u, 65535u}) {
            if (check_table(n, kind, rng)) return 1;
            ++rounds;
        }
        for (int i = 0; i < 50; ++i, ++rounds)
            if (check_table(1 + rng() % 300, kind, rng)) return 1;
    }
    for (uint32_t dtype = 0; dtype < 4; ++dtype)
        for (uint32_t layout = 0; layout < 2; ++layout)
            for (int i = 0; i < 50; ++i, ++rounds)
                if (check_reference(dtype, layout, rng)) return 1;
    if (check_domains() || check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
