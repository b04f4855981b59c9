// compose_plan_check.cpp -- the host half of the batch composition (llcomp_amd/csrc/compose_plan.hpp) and the KERNEL'S OWN decisions
// (compose_rule.hpp: the tiles, the units a tile owns, the filter, compose_decide and compose_finish with the shifted copy) walked on the host under a
// sanitizer, workgroup by workgroup and thread by thread as k_compose does, through a memory that checks every access: an address read
// lies in the src batch, an address written in the dst batch, a 16-byte access is aligned, and every dst element is written exactly
// once without KEEP -- at most once, and exactly the covered ones, with it.  The result is compared with llcomp_mi_compose_reference
// bit for bit.  Batches stand at every byte offset 0..15 (that the element allows) of src and of dst, independently.  Host code only;
// built and run by tests/test_compose_plan_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/compose_plan_check.cpp llcomp_amd/csrc/compose_plan.cpp
// Prints "ok <rounds>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "compose_plan.hpp"
#include "compose_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace {

// the memory of compose_rule.hpp's functions on the host: real addresses, every access checked and every written byte counted
struct HostMem {
    uint64_t src, src_bytes, dst, dst_bytes;
    uint32_t es;
    std::vector<uint8_t> written;  // per byte of dst
    bool bad = false;

    bool in_src(uint64_t a, uint64_t n) { return a >= src && a + n <= src + src_bytes; }
    bool in_dst(uint64_t a, uint64_t n) { return a >= dst && a + n <= dst + dst_bytes; }
    void count(uint64_t a, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) ++written[size_t(a - dst + i)];
    }
    ComposeChunk load16(uint64_t a) {
        ComposeChunk c{{0, 0, 0, 0}};
        if ((a & 15) || !in_src(a, 16)) return bad = true, c;
        std::memcpy(&c, reinterpret_cast<const void*>(uintptr_t(a)), 16);
        return c;
    }
    void store16(uint64_t a, const ComposeChunk& c) {
        if ((a & 15) || !in_dst(a, 16)) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &c, 16);
        count(a, 16);
    }
    uint32_t load_el(uint64_t a) {
        uint32_t v = 0;
        if ((a & (es - 1)) || !in_src(a, es)) return bad = true, v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), es);
        return v;
    }
    void store_el(uint64_t a, uint32_t bits) {
        if ((a & (es - 1)) || !in_dst(a, es)) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &bits, es);
        count(a, es);
    }
};

struct Call {
    uint32_t n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, flags;
    std::vector<llcomp_mi_compose_piece> pieces;
    std::vector<float> fill;
    uint32_t src_off, dst_off;  // bytes past a multiple of 16
};

template <uint32_t ES>
void walk(const ComposeGeom& g, const ComposeSample* samples, uint32_t n_samples, const ComposeRec* recs, const uint32_t* fill_bits, HostMem& mem,
          bool& cap_ok) {
    for (uint32_t z = 0; z < n_samples; ++z)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t tile = 0; tile < g.tiles_x * g.tiles_y; ++tile) {  // one workgroup
                const ComposeTileBox box = compose_tile_box(g, ES, tile);
                std::vector<ComposeRec> list;  // the short list, or the sample's whole run where that has no room for it
                const bool filtered = samples[z].count <= kComposeListCap;
                for (uint32_t i = 0; i < samples[z].count; ++i)
                    if (!filtered || compose_hits(recs[samples[z].first + i], box)) list.push_back(recs[samples[z].first + i]);
                if (samples[z].count > kComposeMaxPiecesPerSample) cap_ok = false;
                const uint32_t* fill = fill_bits + (g.planes > 1 ? pl : 0u);
                std::vector<ComposeChunk> patterns;
                for (uint32_t ph = 0; g.cs <= kComposePatterns && ph < g.cs; ++ph) patterns.push_back(compose_pattern<ES>(fill, g.cs, ph));
                ComposeWork k;
                k.list = list.data(), k.n_list = uint32_t(list.size()), k.fill = fill, k.cmod = g.cs, k.patterns = patterns.data();
                k.d = samples[z].dst, k.pl = pl;
                if (!k.n_list && g.keep) continue;
                k.solo = filtered && compose_solo(k.list, k.n_list, box);
                for (uint32_t tid = 0; tid < 256; ++tid) compose_tile_pass<ES>(g, k, box, tid, 256, mem);
            }
}

int run(const Call& c, std::mt19937& rng) {
    const uint32_t es = batch_esize(c.dtype);
    const bool chw = c.layout == LLCOMP_MI_LAYOUT_CHW, keep = c.flags & LLCOMP_MI_COMPOSE_KEEP;
    const size_t src_bytes = size_t(c.n_src) * c.c * c.iw * c.ih * es, dst_bytes = size_t(c.n_dst) * c.c * c.ow * c.oh * es;
    // operator new[] aligns to 16: the batches begin src_off / dst_off bytes behind that and end where their arrays end
    std::unique_ptr<uint8_t[]> src_buf(new uint8_t[c.src_off + src_bytes]), dst_buf(new uint8_t[c.dst_off + dst_bytes]), ref(new uint8_t[dst_bytes]);
    CHECK(reinterpret_cast<uintptr_t>(src_buf.get()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_buf.get()) % 16 == 0);
    uint8_t* src = c.n_src ? src_buf.get() + c.src_off : nullptr;
    uint8_t* dst = dst_buf.get() + c.dst_off;
    for (size_t i = 0; i < src_bytes; ++i) src[i] = uint8_t(rng());
    for (size_t i = 0; i < dst_bytes; ++i) dst[i] = uint8_t(rng());
    const llcomp_mi_compose_piece* pieces = c.pieces.empty() ? nullptr : c.pieces.data();
    const uint32_t n_pieces = uint32_t(c.pieces.size());
    const float* fill_value = c.fill.empty() ? nullptr : c.fill.data();
    CHECK(compose_reference(src, c.n_src, c.iw, c.ih, dst, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, fill_value, c.flags,
                            ref.get()) == LLCOMP_MI_OK);

    std::vector<uint32_t> fill_bits;
    CHECK(compose_check_call(c.n_src, c.iw, c.ih, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, fill_value, c.flags, fill_bits) ==
          LLCOMP_MI_OK);
    CHECK(compose_check_memory(src, src_bytes, dst, dst_bytes, es) == LLCOMP_MI_OK);
    ComposePlan p;
    compose_plan(c.n_dst, pieces, n_pieces, c.flags, p);
    // the plan: the samples ascending, their runs a partition of the pieces that are not empty, each run in the call's order
    size_t at = 0, live = 0;
    for (const llcomp_mi_compose_piece& q : c.pieces) live += !compose_empty(q);
    CHECK(p.order.size() == live);
    for (size_t j = 0; j < p.samples.size(); ++j) {
        const ComposeSample& s = p.samples[j];
        CHECK(s.dst < c.n_dst && (!j || p.samples[j - 1].dst < s.dst) && s.first == at && (s.count || !keep));
        for (uint32_t i = 0; i < s.count; ++i) {
            const uint32_t pi = p.order[s.first + i];
            CHECK(pi < n_pieces && c.pieces[pi].dst == s.dst && !compose_empty(c.pieces[pi]) && (!i || p.order[s.first + i - 1] < pi));
        }
        at += s.count;
    }
    CHECK(at == live && (keep || p.samples.size() == c.n_dst));
    const ComposeTable t(p.samples.size(), p.order.size(), c.c);
    CHECK(t.bytes <= compose_table_bound(c.n_dst, n_pieces, c.c));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes]);
    compose_table_put(pieces, p, fill_bits, c.layout, table.get());
    std::vector<ComposeSample> samples(p.samples.size());
    std::vector<ComposeRec> recs(p.order.size());
    std::vector<uint32_t> fb(c.c);
    if (!samples.empty()) std::memcpy(samples.data(), table.get() + t.samples_at, samples.size() * sizeof(ComposeSample));
    if (!recs.empty()) std::memcpy(recs.data(), table.get() + t.recs_at, recs.size() * sizeof(ComposeRec));
    std::memcpy(fb.data(), table.get() + t.fill_at, size_t(c.c) * 4);

    const ComposeGeom g = compose_geom(reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(src), c.n_src, c.iw, c.ih, c.ow, c.oh, c.c, es,
                                       chw, keep);
    CHECK(compose_workgroups(p, c.ow, c.oh, c.c, c.dtype, c.layout) == uint64_t(samples.size()) * g.planes * g.tiles_x * g.tiles_y);
    HostMem mem{g.src, g.src_bytes, g.dst, dst_bytes, es, std::vector<uint8_t>(dst_bytes, 0), false};
    bool cap_ok = true;
    if (es == 1) walk<1>(g, samples.data(), uint32_t(samples.size()), recs.data(), fb.data(), mem, cap_ok);
    else if (es == 2) walk<2>(g, samples.data(), uint32_t(samples.size()), recs.data(), fb.data(), mem, cap_ok);
    else walk<4>(g, samples.data(), uint32_t(samples.size()), recs.data(), fb.data(), mem, cap_ok);
    CHECK(!mem.bad && cap_ok);
    CHECK(std::memcmp(dst, ref.get(), dst_bytes) == 0);
    // every element once; under KEEP the covered ones once and the others never
    const uint32_t cs = chw ? 1u : c.c, planes = chw ? c.c : 1u;
    size_t byte = 0;
    for (uint32_t d = 0; d < c.n_dst; ++d)
        for (uint32_t pl = 0; pl < planes; ++pl)
            for (uint32_t y = 0; y < c.oh; ++y)
                for (uint32_t x = 0; x < c.ow; ++x) {
                    bool covered = !keep;
                    for (size_t i = 0; i < c.pieces.size() && !covered; ++i) covered = c.pieces[i].dst == d && compose_covers(c.pieces[i], x, y);
                    for (uint32_t b = 0; b < cs * es; ++b, ++byte) CHECK(mem.written[byte] == (covered ? 1 : 0));
                }
    CHECK(byte == dst_bytes);
    return 0;
}

const uint32_t kDtypes[4] = {LLCOMP_MI_DTYPE_U8, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_DTYPE_BF16, LLCOMP_MI_DTYPE_F32};
const uint32_t kLayouts[2] = {LLCOMP_MI_LAYOUT_CHW, LLCOMP_MI_LAYOUT_HWC};

// a drawn call: pieces that overlap, hide each other, are empty or FILL; big: shapes that cross the tile's borders
Call draw(uint32_t dtype, uint32_t layout, uint32_t src_off, uint32_t dst_off, bool big, std::mt19937& rng) {
    static const uint32_t cs[3] = {1, 3, 5};
    Call c{};
    c.dtype = dtype, c.layout = layout, c.src_off = src_off, c.dst_off = dst_off;
    c.c = cs[rng() % 3];
    const uint32_t rows = compose_tile_rows(batch_esize(dtype) * (layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c.c));
    c.n_src = rng() % 8 ? 1 + rng() % 3 : 0, c.n_dst = 1 + rng() % 3;
    c.iw = 1 + rng() % (big ? 160 : 40), c.ih = 1 + rng() % (big ? 24 : 9);
    c.ow = big ? kComposeTile - 2 + rng() % (kComposeTile + 5) : 1 + rng() % 48;
    c.oh = big ? rows - 1 + rng() % (rows + 3) : 1 + rng() % 9;
    c.flags = rng() % 2 ? LLCOMP_MI_COMPOSE_KEEP : 0u;
    if (rng() % 4) {
        for (uint32_t ch = 0; ch < c.c; ++ch) c.fill.push_back(dtype == LLCOMP_MI_DTYPE_U8 ? float(rng() % 256) : float(int32_t(rng() % 2001) - 1000) / 8.0f);
    }
    const uint32_t n = rng() % 9;
    for (uint32_t i = 0; i < n; ++i) {
        llcomp_mi_compose_piece p{};
        p.dst = rng() % c.n_dst;
        const bool fill = !c.n_src || rng() % 4 == 0;
        const uint32_t mw = fill || c.iw > c.ow ? c.ow : c.iw, mh = fill || c.ih > c.oh ? c.oh : c.ih;
        p.w = rng() % 8 ? 1 + rng() % mw : 0, p.h = rng() % 8 ? 1 + rng() % mh : 0;
        p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1);
        if (fill) {
            p.flags = LLCOMP_MI_COMPOSE_FILL;
        } else {
            p.src = rng() % c.n_src, p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1);
        }
        c.pieces.push_back(p);
    }
    return c;
}

int check_refusals() {
    std::vector<uint32_t> bits(1, 77u);
    llcomp_mi_compose_piece ok{};
    ok.w = 4, ok.h = 4;
    auto call = [&](const llcomp_mi_compose_piece& p, uint32_t n_src = 2, uint32_t n_dst = 2, uint32_t c = 3, uint32_t dtype = LLCOMP_MI_DTYPE_F16,
                    uint32_t layout = LLCOMP_MI_LAYOUT_CHW, uint32_t flags = 0, const float* fill = nullptr, uint32_t n_pieces = 1) {
        return compose_check_call(n_src, 8, 8, n_dst, 8, 8, c, dtype, layout, &p, n_pieces, fill, flags, bits);
    };
    CHECK(call(ok) == LLCOMP_MI_OK && bits.size() == 3);
    bits.assign(1, 77u);
    llcomp_mi_compose_piece p = ok;
    p.dst = 2;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.src = 2;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.dx = 5;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.dy = 0xFFFFFFFFu;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.sx = 5;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.sy = 5;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.flags = 2;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.reserved = 1;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.flags = LLCOMP_MI_COMPOSE_FILL, p.sx = 1;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.flags = LLCOMP_MI_COMPOSE_FILL, p.src = 1;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 0) == LLCOMP_MI_BAD_ARGS && call(ok, 65536) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 0) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 65536) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 2, 0) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 2, 3, 4) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, 2) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, 2) == LLCOMP_MI_BAD_ARGS);
    const float inf[3] = {0.0f, 1.0f / 0.0f, 0.0f}, half[3] = {0.5f, 0.0f, 0.0f};
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, 0, inf) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_U8, LLCOMP_MI_LAYOUT_CHW, 0, half) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, 0, half) == LLCOMP_MI_OK);
    bits.assign(1, 77u);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, 0, nullptr, kComposeMaxPieces + 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(compose_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, nullptr, 1, nullptr, 0, bits) == LLCOMP_MI_BAD_ARGS);
    // the cap on one dst sample: empty pieces do not count
    std::vector<llcomp_mi_compose_piece> many(kComposeMaxPiecesPerSample + 1, ok);
    many[3].w = 0;
    CHECK(compose_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), nullptr, 0, bits) == LLCOMP_MI_OK);
    bits.assign(1, 77u);
    many[3].w = 4;
    CHECK(compose_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), nullptr, 0, bits) == LLCOMP_MI_BAD_ARGS);
    many[3].dst = 1;
    CHECK(compose_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), nullptr, 0, bits) == LLCOMP_MI_OK);
    // memory: NULL, alignment, overlap
    alignas(16) static uint8_t m[64];
    CHECK(compose_check_memory(m, 16, m + 16, 16, 2) == LLCOMP_MI_OK && compose_check_memory(m, 17, m + 16, 16, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(compose_check_memory(m + 16, 16, m, 17, 1) == LLCOMP_MI_BAD_ARGS && compose_check_memory(m + 32, 16, m, 32, 4) == LLCOMP_MI_OK);
    CHECK(compose_check_memory(nullptr, 16, m, 16, 1) == LLCOMP_MI_BAD_ARGS && compose_check_memory(nullptr, 0, m, 16, 1) == LLCOMP_MI_OK);
    CHECK(compose_check_memory(m, 16, nullptr, 16, 1) == LLCOMP_MI_BAD_ARGS && compose_check_memory(m + 1, 16, m + 32, 16, 2) == LLCOMP_MI_BAD_ARGS);
    CHECK(compose_check_memory(m, 16, m + 33, 16, 2) == LLCOMP_MI_BAD_ARGS && compose_check_memory(m, 64, m, 64, 1) == LLCOMP_MI_BAD_ARGS);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20251);
    uint32_t rounds = 0;
    // every byte offset of src against every byte offset of dst, small drawn calls
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts) {
            const uint32_t es = batch_esize(dtype);
            for (uint32_t so = 0; so < 16; so += es)
                for (uint32_t d0 = 0; d0 < 16; d0 += es, ++rounds)
                    if (run(draw(dtype, layout, so, d0, false, rng), rng)) return 1;
        }
    // shapes around the tile's borders, offsets drawn
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts) {
            const uint32_t es = batch_esize(dtype);
            for (uint32_t i = 0; i < 12; ++i, ++rounds)
                if (run(draw(dtype, layout, rng() % 16 / es * es, rng() % 16 / es * es, true, rng), rng)) return 1;
        }
    // all 16 shifts of the shifted copy: sx against dx, one-row pieces of 1, 15, 16, 17 and 33 pixels, for every element size and HWC c = 3
    static const uint32_t widths[5] = {1, 15, 16, 17, 33};
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t sx = 0; sx < 16; ++sx)
                for (uint32_t dx = 0; dx < 16; ++dx, ++rounds) {
                    Call c{};
                    c.dtype = dtype, c.layout = layout, c.c = layout == LLCOMP_MI_LAYOUT_HWC ? 3 : 1;
                    c.n_src = 1, c.iw = 52, c.ih = 3, c.n_dst = 5, c.ow = 50, c.oh = 2, c.flags = (sx ^ dx) & 1;
                    for (uint32_t i = 0; i < 5; ++i) {
                        llcomp_mi_compose_piece p{};
                        p.dst = i, p.dx = dx, p.sx = sx, p.dy = i & 1, p.sy = 1 + (i & 1), p.w = widths[i], p.h = 1;
                        c.pieces.push_back(p);
                    }
                    if (run(c, rng)) return 1;
                }
    // more pieces on one dst sample than the short list holds: the whole run, not filtered
    for (uint32_t layout : kLayouts) {
        Call c{};
        c.dtype = LLCOMP_MI_DTYPE_F16, c.layout = layout, c.c = 3, c.src_off = 2, c.dst_off = 6;
        c.n_src = 2, c.iw = 9, c.ih = 7, c.n_dst = 2, c.ow = kComposeTile + 3, c.oh = 5, c.flags = layout;
        for (uint32_t i = 0; i < kComposeListCap + 40; ++i) {
            llcomp_mi_compose_piece p{};
            p.dst = i % 7 == 0, p.src = rng() % 2, p.w = 1 + rng() % 9, p.h = 1 + rng() % 5;
            p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1), p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1);
            c.pieces.push_back(p);
        }
        if (run(c, rng)) return 1;
        ++rounds;
    }
    if (check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
