// wide_paste_check.cpp -- the batch copy-paste by ids of 3 and 4 bytes (llcomp_amd/csrc/paste_rule.hpp with MB 3 and 4, paste_plan.cpp)
// walked on the host under a sanitizer as tests/helpers/paste_check.cpp walks the 8- and 16-bit calls: k_paste<MB, ES>'s workgroups
// (a tile of a plane of a dst sample, its short list) and threads through a memory that checks every access -- reads inside the src
// or the mask batch, writes inside the dst batch, 16-byte accesses aligned, a 4-byte mask pixel read at a multiple of 4, a 3-byte one
// anywhere; the mask is never written; a selected dst element is written exactly once and any other never -- and compared with
// llcomp_mi_paste32_reference bit for bit.  Host code only; built and run by tests/test_wide_id_paste_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/wide_paste_check.cpp llcomp_amd/csrc/paste_plan.cpp
// Prints "ok <rounds>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "paste_plan.hpp"
#include "paste_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace {

struct HostMem {
    uint64_t src, src_bytes, mask, mask_bytes, dst, dst_bytes;
    uint32_t es;
    std::vector<uint8_t> written;  // per byte of dst
    bool bad = false;

    bool readable(uint64_t a, uint64_t n) { return (a >= src && a + n <= src + src_bytes) || (a >= mask && a + n <= mask + mask_bytes); }
    bool in_dst(uint64_t a, uint64_t n) { return a >= dst && a + n <= dst + dst_bytes; }
    void count(uint64_t a, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) ++written[size_t(a - dst + i)];
    }
    ComposeChunk load16(uint64_t a) {
        ComposeChunk c{{0, 0, 0, 0}};
        if ((a & 15) || !readable(a, 16)) return bad = true, c;
        std::memcpy(&c, reinterpret_cast<const void*>(uintptr_t(a)), 16);
        return c;
    }
    void store16(uint64_t a, const ComposeChunk& c) {
        if ((a & 15) || !in_dst(a, 16)) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &c, 16);
        count(a, 16);
    }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) {
        uint32_t v = 0;
        if ((N != 3 && (a & (N - 1))) || !readable(a, N)) return bad = true, v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);
        return v;
    }
    template <uint32_t N>
    void store_el(uint64_t a, uint32_t bits) {
        if (N != es || (a & (es - 1)) || !in_dst(a, es)) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &bits, es);
        count(a, es);
    }
};

template <class P>
struct Call {
    uint32_t n_src, iw, ih, n_dst, ow, oh, c, dtype, layout;
    std::vector<P> pieces;
    uint32_t src_off, dst_off, mask_off;  // bytes past a multiple of 16
    bool alias;                           // the mask batch IS the src batch
};

// ids that differ only in byte 2 or byte 3 while bytes 0-1 agree, and the ends of the range
const uint32_t kPool[8] = {0x000001, 0x010001, 0xFF0001, 0x01000001, 0x000000, 0xFFFFFFFF, 0x000002, 0x010002};
template <uint32_t MB>
uint32_t pool_id(std::mt19937& rng) { return kPool[rng() % 8] & (MB == 3 ? 0xFFFFFFu : 0xFFFFFFFFu); }

template <uint32_t MB, uint32_t ES>
void walk(const PasteGeom& pg, const ComposeSample* samples, uint32_t n_samples, const PasteRec<MB>* recs, HostMem& mem, bool& cap_ok) {
    const ComposeGeom& g = pg.g;
    for (uint32_t z = 0; z < n_samples; ++z)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t tile = 0; tile < g.tiles_x * g.tiles_y; ++tile) {  // one workgroup
                const ComposeTileBox box = compose_tile_box(g, ES, tile);
                std::vector<PasteRec<MB>> list;  // the short list
                if (samples[z].count > kPasteMaxPiecesPerSample) cap_ok = false;
                for (uint32_t i = 0; i < samples[z].count; ++i)
                    if (compose_hits(recs[samples[z].first + i].r, box)) list.push_back(recs[samples[z].first + i]);
                PasteWork<MB> k;
                k.list = list.data(), k.n_list = uint32_t(list.size()), k.d = samples[z].dst, k.pl = pl;
                if (!k.n_list) continue;
                for (uint32_t tid = 0; tid < 256; ++tid) paste_tile_pass<MB, ES>(pg, k, box, tid, 256, mem);
            }
}

template <class P>
int run(const Call<P>& c, std::mt19937& rng) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    const uint32_t es = batch_esize(c.dtype);
    const bool chw = c.layout == LLCOMP_MI_LAYOUT_CHW;
    const size_t src_bytes = size_t(c.n_src) * c.c * c.iw * c.ih * es, dst_bytes = size_t(c.n_dst) * c.c * c.ow * c.oh * es;
    const size_t mask_bytes = MB * size_t(c.n_src) * c.iw * c.ih;
    // operator new[] aligns to 16: the batches begin their offsets behind that and end where their arrays end
    std::unique_ptr<uint8_t[]> src_buf(new uint8_t[c.src_off + src_bytes]), dst_buf(new uint8_t[c.dst_off + dst_bytes]), ref(new uint8_t[dst_bytes]);
    std::unique_ptr<uint8_t[]> mask_buf(new uint8_t[c.mask_off + mask_bytes]), mask_copy(new uint8_t[mask_bytes]);
    CHECK(reinterpret_cast<uintptr_t>(src_buf.get()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_buf.get()) % 16 == 0);
    CHECK(reinterpret_cast<uintptr_t>(mask_buf.get()) % 16 == 0 && (MB == 3 || c.mask_off % 4 == 0));
    uint8_t* src = src_buf.get() + c.src_off;
    uint8_t* dst = dst_buf.get() + c.dst_off;
    uint8_t* mask = c.alias ? src : mask_buf.get() + c.mask_off;
    CHECK(!c.alias || src_bytes == mask_bytes);
    for (size_t i = 0; i < src_bytes; ++i) src[i] = uint8_t(rng());
    for (size_t i = 0; i < mask_bytes; i += MB) {  // (an aliased src becomes the map)
        const uint32_t id = pool_id<MB>(rng);
        std::memcpy(mask + i, &id, MB);
    }
    std::memcpy(mask_copy.get(), mask, mask_bytes);
    for (size_t i = 0; i < dst_bytes; ++i) dst[i] = uint8_t(rng());
    const P* pieces = c.pieces.empty() ? nullptr : c.pieces.data();
    const uint32_t n_pieces = uint32_t(c.pieces.size());
    CHECK(llcomp_mi_paste32_reference(src, mask, MB, c.n_src, c.iw, c.ih, dst, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, ref.get()) == LLCOMP_MI_OK);

    std::vector<uint32_t> value_bits;
    CHECK(paste_check_call(c.n_src, c.iw, c.ih, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, value_bits) == LLCOMP_MI_OK);
    CHECK(paste_check_memory(src, src_bytes, mask, mask_bytes, dst, dst_bytes, es, paste_mask_align(MB), n_pieces) == LLCOMP_MI_OK);
    PastePlan p;
    paste_plan(c.n_dst, pieces, n_pieces, p);
    size_t live = 0;
    for (const P& q : c.pieces) live += !paste_idle(q);
    CHECK(p.order.size() == live);
    const PasteTable<MB> t(p.samples.size(), p.order.size());
    CHECK(t.bytes <= paste_table_bound<MB>(c.n_dst, n_pieces) && paste_table_bound<MB>(c.n_dst, n_pieces) == paste_table_bound<2>(c.n_dst, n_pieces));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes + 1]);
    paste_table_put(pieces, p, value_bits, c.c, c.layout, table.get());
    std::vector<ComposeSample> samples(p.samples.size());
    std::vector<PasteRec<MB>> recs(p.order.size());
    if (!samples.empty()) std::memcpy(static_cast<void*>(samples.data()), table.get() + t.samples_at, samples.size() * sizeof(ComposeSample));
    if (!recs.empty()) std::memcpy(static_cast<void*>(recs.data()), table.get() + t.recs_at, recs.size() * sizeof(PasteRec<MB>));

    const PasteGeom pg = paste_geom<MB>(reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(mask), c.n_src,
                                        c.iw, c.ih, c.ow, c.oh, c.c, es, chw);
    CHECK(pg.mask_bytes == mask_bytes);
    HostMem mem{pg.g.src, src_bytes, pg.mask, mask_bytes, pg.g.dst, dst_bytes, es, std::vector<uint8_t>(dst_bytes, 0)};
    bool cap_ok = true;
    if (es == 1) walk<MB, 1>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    else if (es == 2) walk<MB, 2>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    else walk<MB, 4>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    CHECK(!mem.bad && cap_ok);
    CHECK(std::memcmp(dst, ref.get(), dst_bytes) == 0);
    CHECK(c.alias || std::memcmp(mask, mask_copy.get(), mask_bytes) == 0);
    // the selected elements once, the others never
    const uint32_t cs = chw ? 1u : c.c, planes = chw ? c.c : 1u;
    PlainMem plain;
    size_t byte = 0;
    for (uint32_t d = 0; d < c.n_dst; ++d)
        for (uint32_t pl = 0; pl < planes; ++pl)
            for (uint32_t y = 0; y < c.oh; ++y)
                for (uint32_t x = 0; x < c.ow; ++x) {
                    bool selected = false;
                    for (size_t i = 0; i < c.pieces.size() && !selected; ++i) selected = c.pieces[i].dst == d && paste_selects<MB>(pg, c.pieces[i], x, y, plain);
                    for (uint32_t b = 0; b < cs * es; ++b, ++byte) CHECK(mem.written[byte] == (selected ? 1 : 0));
                }
    CHECK(byte == dst_bytes);
    return 0;
}

// a drawn window over the pool's ids: mostly one id or a base near one with drawn bits, now and then all bits, none, or a window that
// passes the top id
template <class P>
void draw_ids(P& p, std::mt19937& rng) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>, kTop = MB == 3 ? 0xFFFFFFu : 0xFFFFFFFFu;
    const uint32_t kind = rng() % 16;
    if (kind == 0) {
        p.id_base = rng() % 2 ? 0 : kTop - 10;  // all bits; the second passes the top id
        for (uint32_t i = 0; i < 8; ++i) p.ids[i] = 0xFFFFFFFFu;
    } else if (kind == 1) {
        p.id_base = kTop, p.ids[0] = 0xFFFFFFFEu;  // above the top altogether: ignored
    } else if (kind != 2) {                       // (2: no bit at all)
        const uint32_t around = pool_id<MB>(rng), back = rng() % 3;
        p.id_base = around >= back ? around - back : 0;
        p.ids[0] = 1u << back | (rng() & 0x7u);
        if (rng() % 4 == 0) p.ids[1 + rng() % 7] |= rng();
    }
}
template <class P>
void draw_value(P& p, uint32_t dtype, uint32_t layout, uint32_t c, std::mt19937& rng) {
    const uint32_t es = batch_esize(dtype);
    if (rng() % 3) return;
    p.flags = LLCOMP_MI_PASTE_VALUE;
    p.value_bits = es == 4 ? uint32_t(rng()) : uint32_t(rng()) & ((1u << (8 * es)) - 1u);
    if (dtype == LLCOMP_MI_DTYPE_U8 && layout == LLCOMP_MI_LAYOUT_HWC && c <= 4 && rng() % 2) {
        p.flags |= LLCOMP_MI_PASTE_VALUE_PIXEL;
        p.value_bits = c == 4 ? uint32_t(rng()) : uint32_t(rng()) & ((1u << (8 * c)) - 1u);
    }
}

const uint32_t kDtypes[4] = {LLCOMP_MI_DTYPE_U8, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_DTYPE_BF16, LLCOMP_MI_DTYPE_F32};
const uint32_t kLayouts[2] = {LLCOMP_MI_LAYOUT_CHW, LLCOMP_MI_LAYOUT_HWC};

// a drawn call: pieces that overlap, hide each other, are empty or VALUE; the maps their own source half the time where the shapes allow
template <class P>
Call<P> draw(uint32_t dtype, uint32_t layout, uint32_t mask_off, uint32_t dst_off, std::mt19937& rng) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    static const uint32_t cs[5] = {1, 2, 3, 4, 5};
    const uint32_t es = batch_esize(dtype);
    Call<P> c{};
    c.dtype = dtype, c.layout = layout, c.dst_off = dst_off, c.mask_off = mask_off, c.src_off = rng() % 16 / es * es;
    c.c = cs[rng() % 5];
    const bool can = (es == 1 && layout == LLCOMP_MI_LAYOUT_HWC) || (MB == 4 && dtype == LLCOMP_MI_DTYPE_F32);
    if (can && rng() % 2) c.alias = true, c.c = es == 1 ? MB : 1, c.src_off = mask_off;
    c.n_src = 1 + rng() % 2, c.n_dst = 1 + rng() % 2;
    c.iw = 1 + rng() % 40, c.ih = 1 + rng() % 5, c.ow = 1 + rng() % 40, c.oh = 1 + rng() % 5;
    const uint32_t n = rng() % 7;
    for (uint32_t i = 0; i < n; ++i) {
        P p{};
        p.dst = rng() % c.n_dst, p.src = rng() % c.n_src;
        p.w = rng() % 8 == 0 ? 0 : 1 + rng() % (c.iw < c.ow ? c.iw : c.ow), p.h = 1 + rng() % (c.ih < c.oh ? c.ih : c.oh);
        p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1), p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1);
        draw_ids(p, rng);
        draw_value(p, dtype, layout, c.c, rng);
        c.pieces.push_back(p);
    }
    return c;
}

template <class P>
int rounds_of(std::mt19937& rng, uint32_t& rounds) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    // every byte offset of the mask (MB 4: every multiple of 4) against every dst offset the element allows
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t mask_off = 0; mask_off < 16; mask_off += MB == 3 ? 1 : 4)
                for (uint32_t dst_off = 0; dst_off < 16; dst_off += batch_esize(dtype)) {
                    if (run(draw<P>(dtype, layout, mask_off, dst_off, rng), rng)) return 1;
                    ++rounds;
                }
    // all 16 x 16 pairs of sx and dx with one-row pieces of 1, 5, 6, 7, 15, 16, 17 and 33 pixels: where one to four (five) mask units
    // are decided
    static const uint32_t widths[8] = {1, 5, 6, 7, 15, 16, 17, 33};
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t sx = 0; sx < 16; ++sx)
                for (uint32_t dx = 0; dx < 16; ++dx) {
                    Call<P> c{};
                    c.dtype = dtype, c.layout = layout, c.c = layout == LLCOMP_MI_LAYOUT_HWC && (sx ^ dx) & 4 ? 3 : 1;
                    c.n_src = c.n_dst = 1, c.iw = c.ow = 16 + 33, c.ih = c.oh = 8;
                    c.mask_off = MB == 3 ? (sx * 5 + dx * 3) % 16 : (sx + dx) % 4 * 4, c.dst_off = (dx * 7 + sx) % 16 / batch_esize(dtype) * batch_esize(dtype);
                    for (uint32_t r = 0; r < 8; ++r) {
                        P p{};
                        p.dx = dx, p.sx = sx, p.dy = p.sy = r, p.w = widths[r], p.h = 1;
                        p.id_base = (sx ^ dx) & 1 ? 0 : 0x010000, p.ids[0] = (sx ^ dx) & 2 ? 0x7u : 0x2u;
                        if (r == 3) p.flags = LLCOMP_MI_PASTE_VALUE, p.value_bits = 0x5A;
                        c.pieces.push_back(p);
                    }
                    if (run(c, rng)) return 1;
                    ++rounds;
                }
    // 256 pieces on one dst sample
    for (uint32_t k = 0; k < 2; ++k) {
        Call<P> c{};
        c.dtype = k ? LLCOMP_MI_DTYPE_U8 : LLCOMP_MI_DTYPE_F16, c.layout = k ? LLCOMP_MI_LAYOUT_HWC : LLCOMP_MI_LAYOUT_CHW, c.c = 3;
        c.n_src = 2, c.n_dst = 2, c.iw = 37, c.ih = 9, c.ow = 41, c.oh = 9, c.mask_off = MB == 3 ? 7 : 12, c.dst_off = 2;
        for (uint32_t i = 0; i < 256; ++i) {
            P p{};
            p.dst = 1, p.src = rng() % 2, p.w = 1 + rng() % 20, p.h = 1 + rng() % 4;
            p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1), p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1);
            p.id_base = pool_id<MB>(rng), p.ids[0] = 1u | 1u << (rng() % 8);
            c.pieces.push_back(p);
        }
        if (run(c, rng)) return 1;
        ++rounds;
    }
    return 0;
}

int check_refusals() {
    alignas(16) static uint8_t src[4 * 6 * 4 * 4 + 16], dst[4 * 6 * 4 * 4 + 16], mask[6 * 4 * 4 + 16], out[4 * 6 * 4 * 4 + 16];
    llcomp_mi_paste_piece32 ok{};
    ok.w = 3, ok.h = 2, ok.id_base = 0, ok.ids[0] = 1;
    auto call = [&](const llcomp_mi_paste_piece32& p, uint32_t mb, uint32_t c, uint32_t dtype, uint32_t layout, const uint8_t* m = nullptr) {
        return llcomp_mi_paste32_reference(src, m ? m : mask, mb, 1, 6, 4, dst, 1, 6, 4, c, dtype, layout, &p, 1, out);
    };
    const uint32_t U8 = LLCOMP_MI_DTYPE_U8, HWC = LLCOMP_MI_LAYOUT_HWC, CHW = LLCOMP_MI_LAYOUT_CHW;
    CHECK(call(ok, 3, 3, U8, HWC) == LLCOMP_MI_OK && call(ok, 4, 3, U8, HWC) == LLCOMP_MI_OK && call(ok, 3, 3, U8, HWC, mask + 1) == LLCOMP_MI_OK);
    for (uint32_t mb : {0u, 1u, 2u, 5u}) CHECK(call(ok, mb, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);
    for (uint32_t off : {1u, 2u, 3u, 6u}) CHECK(call(ok, 4, 3, U8, HWC, mask + off) == LLCOMP_MI_BAD_ARGS);  // a 4-byte mask off its alignment
    auto with = [&](auto&& change) {
        llcomp_mi_paste_piece32 p = ok;
        change(p);
        return p;
    };
    CHECK(call(with([](auto& p) { p.id_base = 0x1000000; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);  // above 0xFFFFFF with map_bytes 3
    CHECK(call(with([](auto& p) { p.id_base = 0xFFFFFFFF; }), 4, 3, U8, HWC) == LLCOMP_MI_OK && call(with([](auto& p) { p.id_base = 0xFFFFFF; }), 3, 3, U8, HWC) == LLCOMP_MI_OK);
    CHECK(call(with([](auto& p) { p.flags = 4; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS && call(with([](auto& p) { p.value_bits = 1; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);
    const uint32_t VP = LLCOMP_MI_PASTE_VALUE | LLCOMP_MI_PASTE_VALUE_PIXEL;
    CHECK(call(with([](auto& p) { p.flags = LLCOMP_MI_PASTE_VALUE_PIXEL; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);  // without VALUE
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 0x030201; }), 3, 3, U8, HWC) == LLCOMP_MI_OK);
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 0x04030201; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);  // a byte at c
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 0x04030201; }), 3, 4, U8, HWC) == LLCOMP_MI_OK);
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 1; }), 3, 3, U8, CHW) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 1; }), 3, 1, LLCOMP_MI_DTYPE_F32, HWC) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(with([&](auto& p) { p.flags = VP, p.value_bits = 1; }), 3, 5, U8, HWC) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(with([&](auto& p) { p.flags = LLCOMP_MI_PASTE_VALUE, p.value_bits = 0x100; }), 3, 3, U8, HWC) == LLCOMP_MI_BAD_ARGS);
    // the 8- and 16-bit calls go on refusing flag bits above bit 0
    llcomp_mi_paste_piece16 p16{};
    p16.w = 3, p16.h = 2, p16.ids[0] = 1, p16.flags = VP;
    alignas(16) static uint16_t mask16[6 * 4];
    CHECK(llcomp_mi_paste16_reference(src, mask16, 1, 6, 4, dst, 1, 6, 4, 3, U8, HWC, &p16, 1, out) == LLCOMP_MI_BAD_ARGS);
    llcomp_mi_paste_piece p8{};
    p8.w = 3, p8.h = 2, p8.ids[0] = 1, p8.flags = VP;
    CHECK(llcomp_mi_paste_reference(src, mask, 1, 6, 4, dst, 1, 6, 4, 3, U8, HWC, &p8, 1, out) == LLCOMP_MI_BAD_ARGS);
    // a window that passes the top id selects nothing there; a piece with no other bit set is ignored
    PastePiece4 top{};
    top.w = 1, top.h = 1, top.id_base = 0xFFFFFFF0u, top.ids[0] = 0xFFFF0000u;
    CHECK(paste_idle(top) && !paste_id_set<4>(top, 0u) && !paste_id_set<4>(top, 5u));
    top.ids[0] = 0x8000u;
    CHECK(!paste_idle(top) && paste_id_set<4>(top, 0xFFFFFFFFu));
    PastePiece3 top3{};
    top3.w = 1, top3.h = 1, top3.id_base = 0xFFFFF0u, top3.ids[0] = 0xFFFF0000u;
    CHECK(paste_idle(top3));
    top3.ids[0] = 0x8000u;
    CHECK(!paste_idle(top3) && paste_id_set<3>(top3, 0xFFFFFFu));
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(3232);
    uint32_t rounds = 0;
    if (rounds_of<PastePiece3>(rng, rounds) || rounds_of<PastePiece4>(rng, rounds) || check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
