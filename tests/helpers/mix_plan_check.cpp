// mix_plan_check.cpp -- the host planner of the batch mixing (llcomp_amd/csrc/mix_plan.hpp) and the rule's host functions
// (mix_rule.hpp, llcomp_mi_mix_reference) under a sanitizer: seeded random permutations with records read from heap arrays of exactly n
// records -- the plan's order and segments written into heap arrays of exactly n and n + 1 entries, every segment within
// kMixSegment, every saved head where the segment in front of it looks for it, the table put into a heap buffer of exactly its size
// and within the bound the codec sizes its buffer by -- the reference with batch and output in heap buffers of exactly their sizes,
// in place too, and the refusals.  Host code only; built and run by tests/test_mix_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/mix_plan_check.cpp llcomp_amd/csrc/mix_plan.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "mix_plan.hpp"
#include "mix_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace {

// n records on the heap, exactly: a permutation of `kind` (0 roll, 1 flip, 2 random, 3 the identity), blends and rectangles drawn
std::unique_ptr<llcomp_mi_mix_sample[]> heap_records(uint32_t n, uint32_t kind, uint32_t ow, uint32_t oh, bool blend, std::mt19937& rng) {
    std::unique_ptr<llcomp_mi_mix_sample[]> s(new llcomp_mi_mix_sample[n]);
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    if (kind == 2) std::shuffle(perm.begin(), perm.end(), rng);
    for (uint32_t i = 0; i < n; ++i) {
        std::memset(&s[i], 0, sizeof s[i]);
        s[i].partner = kind == 0 ? (i + n - 1) % n : kind == 1 ? n - 1 - i : perm[i];
        if (blend && rng() % 3) {
            s[i].flags = LLCOMP_MI_MIX_BLEND;
            const double lam = double(rng() % 1001) / 1000.0;
            s[i].w_own = float(lam), s[i].w_partner = float(1.0 - lam);
        }
        for (uint32_t* r : {s[i].box, s[i].erase}) {
            if (rng() % 2) continue;
            r[0] = rng() % ow, r[1] = rng() % oh;
            r[2] = rng() % (ow - r[0] + 1), r[3] = rng() % (oh - r[1] + 1);
        }
    }
    return s;
}

int check_plan(uint32_t n, uint32_t kind, std::mt19937& rng) {
    const std::unique_ptr<llcomp_mi_mix_sample[]> s = heap_records(n, kind, 8, 8, true, rng);
    std::unique_ptr<uint32_t[]> order(new uint32_t[n]), seg_first(new uint32_t[n + 1]);
    uint32_t n_segments = 0, n_saved = 0;
    CHECK(llcomp_mi_mix_plan(n, s.get(), order.get(), seg_first.get(), &n_segments, &n_saved) == LLCOMP_MI_OK);
    CHECK(n_segments >= 1 && n_segments <= n && seg_first[0] == 0 && seg_first[n_segments] == n && n_saved <= mix_saved_bound(n));
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t j = 0; j < n; ++j) {
        CHECK(order[j] < n && !seen[order[j]]);
        seen[order[j]] = 1;
    }
    MixPlan p;
    mix_plan(n, s.get(), p);
    CHECK(p.segs.size() == n_segments && p.n_saved == n_saved && !std::memcmp(p.order.data(), order.get(), size_t(n) * 4));
    uint32_t saved = 0;
    for (uint32_t k = 0; k < n_segments; ++k) {
        const MixSeg& g = p.segs[k];
        CHECK(g.first == seg_first[k] && g.count == seg_first[k + 1] - seg_first[k] && g.count >= 1 && g.count <= kMixSegment);
        for (uint32_t j = g.first; j + 1 < g.first + g.count; ++j) CHECK(s[order[j]].partner == order[j + 1]);
        const uint32_t tail_partner = s[order[g.first + g.count - 1]].partner;
        if (g.tail_slot == kMixNoSlot) {
            CHECK(tail_partner == order[g.first]);  // a whole cycle
        } else {
            ++saved;
            CHECK(g.tail_slot < n_saved && p.segs[g.tail_slot].slot_sample == tail_partner);
        }
    }
    CHECK(saved == n_saved);
    std::vector<uint32_t> ev = {1, 2, 3};
    const MixTable t(n, n_segments, 3);
    CHECK(t.bytes <= mix_table_bound(n, 3));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes]);
    mix_table_put(n, s.get(), p, ev, table.get());
    CHECK(!std::memcmp(table.get() + t.recs_at, s.get(), size_t(n) * sizeof(llcomp_mi_mix_sample)));
    CHECK(!std::memcmp(table.get() + t.order_at, order.get(), size_t(n) * 4) && !std::memcmp(table.get() + t.erase_at, ev.data(), 12));
    return 0;
}

int check_reference(uint32_t dtype, uint32_t layout, std::mt19937& rng) {
    const uint32_t n = 1 + rng() % 12, c = rng() % 2 ? 3 : 1, ow = 1 + rng() % 9, oh = 1 + rng() % 7, es = batch_esize(dtype);
    const size_t bytes = size_t(n) * c * ow * oh * es;
    const std::unique_ptr<llcomp_mi_mix_sample[]> s = heap_records(n, rng() % 4, ow, oh, dtype != LLCOMP_MI_DTYPE_U8, rng);
    std::unique_ptr<uint8_t[]> batch(new uint8_t[bytes]), out(new uint8_t[bytes]), twice(new uint8_t[bytes]);
    for (size_t i = 0; i < bytes; ++i) batch[i] = uint8_t(rng());  // (any bit pattern: NaNs, infinities and subnormals among them)
    std::unique_ptr<float[]> ev(new float[c]);
    for (uint32_t ch = 0; ch < c; ++ch) ev[ch] = float(rng() % 256);
    const float* evp = rng() % 4 ? ev.get() : nullptr;
    CHECK(llcomp_mi_mix_reference(batch.get(), n, c, ow, oh, dtype, layout, s.get(), evp, out.get()) == LLCOMP_MI_OK);
    std::memcpy(twice.get(), batch.get(), bytes);
    CHECK(llcomp_mi_mix_reference(twice.get(), n, c, ow, oh, dtype, layout, s.get(), evp, twice.get()) == LLCOMP_MI_OK);  // in place
    CHECK(!std::memcmp(out.get(), twice.get(), bytes));
    return 0;
}

int check_rounding() {
    // every binary16 value widens and narrows to itself (a NaN to some NaN), and halfway cases go to even
    for (uint32_t h = 0; h < 0x10000; ++h) {
        const float f = mix_widen<LLCOMP_MI_DTYPE_F16>(h);
        const uint32_t back = mix_narrow<LLCOMP_MI_DTYPE_F16>(f);
        if ((h & 0x7FFFu) > 0x7C00u) CHECK((back & 0x7FFFu) > 0x7C00u);
        else CHECK(back == h);
        const uint32_t b = mix_narrow<LLCOMP_MI_DTYPE_BF16>(mix_widen<LLCOMP_MI_DTYPE_BF16>(h));
        if ((h & 0x7FFFu) > 0x7F80u) CHECK((b & 0x7FFFu) > 0x7F80u);
        else CHECK(b == h);
    }
    CHECK(mix_narrow<LLCOMP_MI_DTYPE_F16>(65520.0f) == 0x7C00u && mix_narrow<LLCOMP_MI_DTYPE_F16>(65519.996f) == 0x7BFFu);
    CHECK(mix_narrow<LLCOMP_MI_DTYPE_F16>(1.00048828125f) == 0x3C00u && mix_narrow<LLCOMP_MI_DTYPE_F16>(1.00146484375f) == 0x3C02u);  // ties to even
    CHECK(mix_narrow<LLCOMP_MI_DTYPE_F16>(2.98023223876953125e-08f) == 0u && mix_narrow<LLCOMP_MI_DTYPE_F16>(8.94069671630859375e-08f) == 2u);  // 0.5 and 1.5 steps
    CHECK(mix_narrow<LLCOMP_MI_DTYPE_BF16>(mix_f32_of(0x3F808000u)) == 0x3F80u && mix_narrow<LLCOMP_MI_DTYPE_BF16>(mix_f32_of(0x3F818000u)) == 0x3F82u);
    CHECK(mix_narrow<LLCOMP_MI_DTYPE_BF16>(mix_f32_of(0x7F7FFFFFu)) == 0x7F80u);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(mix_round<LLCOMP_MI_DTYPE_F32>(-nan) == 0x7FC00000u && mix_round<LLCOMP_MI_DTYPE_F16>(-nan) == 0x7E00u && mix_round<LLCOMP_MI_DTYPE_BF16>(nan) == 0x7FC0u);
    return 0;
}

int check_refusals() {
    std::mt19937 rng(3);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const uint32_t n = 5, ow = 6, oh = 4;
    std::unique_ptr<float[]> out(new float[n * 3 * ow * oh]), batch(new float[n * 3 * ow * oh]);
    std::fill(batch.get(), batch.get() + n * 3 * ow * oh, 1.0f);
    std::fill(out.get(), out.get() + n * 3 * ow * oh, 7.0f);
    auto ref = [&](const llcomp_mi_mix_sample* s, uint32_t dtype, const float* ev) {
        return llcomp_mi_mix_reference(batch.get(), n, 3, ow, oh, dtype, LLCOMP_MI_LAYOUT_CHW, s, ev, out.get());
    };
    for (int what = 0; what < 12; ++what) {
        std::unique_ptr<llcomp_mi_mix_sample[]> s = heap_records(n, 0, ow, oh, true, rng);
        uint32_t dtype = LLCOMP_MI_DTYPE_F32;
        float ev[3] = {0.0f, 1.0f, 2.0f};
        switch (what) {
            case 0: s[2].partner = n; break;
            case 1: s[2].partner = s[3].partner; break;
            case 2: s[0].flags |= 2u; break;
            case 3: s[1].flags = LLCOMP_MI_MIX_BLEND, s[1].w_own = nan; break;
            case 4: s[1].flags = 0, s[1].w_partner = -inf; break;
            case 5: s[4].box[0] = ow - 1, s[4].box[1] = 0, s[4].box[2] = 2, s[4].box[3] = 1; break;
            case 6: s[4].erase[0] = 0, s[4].erase[1] = oh, s[4].erase[2] = 1, s[4].erase[3] = 1; break;
            case 7: s[4].erase[0] = 1, s[4].erase[1] = 1, s[4].erase[2] = 0xFFFFFFFFu, s[4].erase[3] = 1; break;
            case 8: ev[1] = inf; break;
            case 9: s[0].flags = LLCOMP_MI_MIX_BLEND, dtype = LLCOMP_MI_DTYPE_U8; break;
            case 10: dtype = LLCOMP_MI_DTYPE_U8, ev[2] = 2.5f; break;
            default: dtype = 4; break;
        }
        if (what == 10)
            for (uint32_t i = 0; i < n; ++i) s[i].flags = 0;
        CHECK(ref(s.get(), dtype, ev) == LLCOMP_MI_BAD_ARGS);
        if (what < 5) {
            uint32_t ns = 77, nv = 77;
            CHECK(llcomp_mi_mix_plan(n, s.get(), nullptr, nullptr, &ns, &nv) == LLCOMP_MI_BAD_ARGS && ns == 77 && nv == 77);
        }
    }
    for (uint32_t i = 0; i < n * 3 * ow * oh; ++i) CHECK(out[i] == 7.0f);
    const std::unique_ptr<llcomp_mi_mix_sample[]> s = heap_records(n, 1, ow, oh, true, rng);
    CHECK(ref(nullptr, LLCOMP_MI_DTYPE_F32, nullptr) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_mix_reference(batch.get(), 0, 3, ow, oh, LLCOMP_MI_DTYPE_F32, 0, s.get(), nullptr, out.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_mix_reference(batch.get(), n, 3, ow, oh, LLCOMP_MI_DTYPE_F32, 2, s.get(), nullptr, out.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_mix_reference(batch.get(), n, 3, 0, oh, LLCOMP_MI_DTYPE_F32, 0, s.get(), nullptr, out.get()) == LLCOMP_MI_BAD_ARGS);
    CHECK(ref(s.get(), LLCOMP_MI_DTYPE_F32, nullptr) == LLCOMP_MI_OK);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20240923);
    unsigned rounds = 0;
    const uint32_t S = llcomp_mi_mix_segment();
    for (uint32_t kind = 0; kind < 4; ++kind) {
        for (uint32_t n : {1u, 2u, S - 1, S, S + 1, 2 * S + 1, 65535u}) {
            if (check_plan(n, kind, rng)) return 1;
            ++rounds;
        }
        for (int i = 0; i < 100; ++i, ++rounds)
            if (check_plan(1 + rng() % 300, kind, rng)) return 1;
    }
    for (uint32_t dtype = 0; dtype < 4; ++dtype)
        for (uint32_t layout = 0; layout < 2; ++layout)
            for (int i = 0; i < 50; ++i, ++rounds)
                if (check_reference(dtype, layout, rng)) return 1;
    if (check_rounding() || check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
