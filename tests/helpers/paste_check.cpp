// paste_check.cpp -- the host half of the batch copy-paste of either width of id map (llcomp_amd/csrc/paste_plan.hpp) and the KERNEL'S
// OWN decisions (paste_rule.hpp on compose_rule.hpp: the tiles, the units a tile owns, the filter, paste_decide and paste_finish with
// the fetch of one to three mask units and the shifted copies) walked on the host under a sanitizer, workgroup by workgroup and thread
// by thread as k_paste<MB, ES> does, through a memory that checks every access: an address read lies in the src or in the mask batch,
// an address written in the dst batch, a 16-byte access is aligned, an element or a mask pixel is read at an address aligned to it (a
// 16-bit mask pixel at an even one), a selected dst element is written exactly once and one that no piece selects never.  The result is
// compared with llcomp_mi_paste_reference or llcomp_mi_paste16_reference bit for bit.  The walk, the memory and a round exist once,
// templated on MB; what a width draws -- its ids, its values, its offsets, its refusals -- is its Width<MB>.
//   paste_check 8    batches at every byte offset 0..15 (that the element allows) of src and of dst, independently, the mask at a drawn one
//   paste_check 16   the mask at every even byte offset against every offset of dst; batches end where their arrays end
// Host code only; built by tests/test_paste_plan_sanitizers.py (8) and tests/test_paste16_sanitizers.py (16):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/paste_check.cpp llcomp_amd/csrc/paste_plan.cpp
// Prints "ok <rounds>".
#include <cstdio>
#include <cstdlib>
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

// the memory of paste_rule.hpp's functions on the host: real addresses, every access checked and every written byte counted
struct HostMem {
    uint64_t src, src_bytes, mask, mask_bytes, dst, dst_bytes;
    uint32_t es;
    std::vector<uint8_t> written;  // per byte of dst
    bool bad = false;
    uint32_t mask_units = 0;  // 16-byte loads inside the mask batch

    bool in_mask(uint64_t a, uint64_t n) { return a >= mask && a + n <= mask + mask_bytes; }
    bool readable(uint64_t a, uint64_t n) { return (a >= src && a + n <= src + src_bytes) || in_mask(a, n); }
    bool in_dst(uint64_t a, uint64_t n) { return a >= dst && a + n <= dst + dst_bytes; }
    void count(uint64_t a, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) ++written[size_t(a - dst + i)];
    }
    ComposeChunk load16(uint64_t a) {
        ComposeChunk c{{0, 0, 0, 0}};
        if ((a & 15) || !readable(a, 16)) return bad = true, c;
        mask_units += in_mask(a, 16);
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
        if ((a & (N - 1)) || !readable(a, N)) return bad = true, v;
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

// the ids of the 16-bit maps: they share low bytes and differ in the high byte
const uint16_t kPool[8] = {0x0001, 0x0101, 0x0201, 0xFF01, 0x0002, 0x0102, 0x0000, 0xFF00};

// What a width's rounds draw
template <uint32_t MB>
struct Width;
template <>
struct Width<1> {
    using Piece = llcomp_mi_paste_piece;
    static constexpr uint32_t kSeed = 20252, kNWidths = 5, kManyMaskOff = 5;
    static constexpr uint32_t kWidths[5] = {1, 15, 16, 17, 33};  // one-row pieces of the shift rounds
    // the call's channels and offsets: first_off is src's, the mask's is drawn; the mask as its own src for U8, c == 1
    static void begin(Call<Piece>& c, uint32_t first_off, std::mt19937& rng) {
        static const uint32_t cs[3] = {1, 3, 5};
        c.src_off = first_off, c.mask_off = rng() % 16;
        c.c = cs[rng() % 3];
        c.alias = c.dtype == LLCOMP_MI_DTYPE_U8 && c.c == 1 && rng() % 2;
    }
    static bool alias_ok(const Call<Piece>& c, uint32_t es, bool) { return es == 1 && c.c == 1; }
    static void fill(uint8_t* src, size_t src_bytes, uint8_t* mask, size_t mask_bytes, bool alias, std::mt19937& rng) {
        for (size_t i = 0; i < src_bytes; ++i) src[i] = alias ? uint8_t(rng() % 8) : uint8_t(rng());
        for (size_t i = 0; i < mask_bytes && !alias; ++i) mask[i] = uint8_t(rng() % 8);
    }
    // a drawn id set over the mask's bytes 0..7: mostly half of them, now and then all 256 bits, none, or bits the mask does not use
    static void draw_ids(Piece& p, std::mt19937& rng) {
        const uint32_t kind = rng() % 16;
        if (kind == 0) {
            for (uint32_t i = 0; i < 8; ++i) p.ids[i] = 0xFFFFFFFFu;
        } else if (kind == 1) {
            p.ids[7] = 0x80000000u;  // id 255 only: selects nothing here
        } else if (kind != 2) {     // (2: no bit at all)
            p.ids[0] = rng() & 0xFFu;
            p.ids[1 + rng() % 7] |= rng();
        }
    }
    static void draw_value(Piece& p, uint32_t dtype, std::mt19937& rng) {
        if (rng() % 4) return;
        p.flags = LLCOMP_MI_PASTE_VALUE;
        p.value = dtype == LLCOMP_MI_DTYPE_U8 ? float(rng() % 8) : float(int32_t(rng() % 2001) - 1000) / 8.0f;
    }
    static uint32_t shift_mask_off(uint32_t sx, uint32_t dx) { return (sx * 5 + dx * 3) % 16; }
    static void shift_ids(Piece& p, uint32_t sx, uint32_t dx) { p.ids[0] = (sx ^ dx) & 1 ? 0xFFu : 0x5Au; }
    static void many_ids(Piece& p, std::mt19937& rng) { p.ids[0] = 1u << (rng() % 8) | 1u << (rng() % 8); }
};
template <>
struct Width<2> {
    using Piece = llcomp_mi_paste_piece16;
    static constexpr uint32_t kSeed = 16161, kNWidths = 8, kManyMaskOff = 10;
    static constexpr uint32_t kWidths[8] = {1, 7, 8, 9, 15, 16, 17, 33};  // where one, two or three mask units are decided
    // first_off is the mask's, src's is drawn; the maps as their own src for U8 HWC c == 2, or a 2-byte dtype with c == 1
    static void begin(Call<Piece>& c, uint32_t first_off, std::mt19937& rng) {
        static const uint32_t cs[4] = {1, 2, 3, 5};
        const uint32_t es = batch_esize(c.dtype);
        c.mask_off = first_off, c.src_off = rng() % 16 / es * es;
        c.c = cs[rng() % 4];
        c.alias = (es == 2 ? c.c == 1 : es == 1 && c.c == 2 && c.layout == LLCOMP_MI_LAYOUT_HWC) && rng() % 2;
        if (c.alias) c.src_off = first_off;
    }
    static bool alias_ok(const Call<Piece>& c, uint32_t es, bool chw) { return c.src_off % 2 == 0 && (es == 2 ? c.c == 1 : es == 1 && c.c == 2 && !chw); }
    static void fill(uint8_t* src, size_t src_bytes, uint8_t* mask, size_t mask_bytes, bool, std::mt19937& rng) {
        for (size_t i = 0; i < src_bytes; ++i) src[i] = uint8_t(rng());
        for (size_t i = 0; i < mask_bytes; i += 2) {
            const uint16_t id = kPool[rng() % 8];
            std::memcpy(mask + i, &id, 2);
        }
    }
    // a drawn window over the pool's ids: mostly a base near one of them with drawn bits, now and then all bits, none, a window that
    // passes 65535, or bits that the maps do not use
    static void draw_ids(Piece& p, std::mt19937& rng) {
        const uint32_t kind = rng() % 16;
        if (kind == 0) {
            p.id_base = rng() % 2 ? 0 : 0xFF00;
            for (uint32_t i = 0; i < 8; ++i) p.ids[i] = 0xFFFFFFFFu;
        } else if (kind == 1) {
            p.id_base = 0x4000, p.ids[7] = 0x80000000u;  // selects nothing here
        } else if (kind == 2) {
            p.id_base = 65535, p.ids[0] = 0xFFFFFFFEu;  // above 65535 altogether: ignored
        } else if (kind != 3) {                         // (3: no bit at all)
            const uint32_t around = kPool[rng() % 8], back = rng() % 3;
            p.id_base = around >= back ? around - back : 0;
            p.ids[0] = rng() & 0xFFu;
            p.ids[1 + rng() % 7] |= rng();
            if (rng() % 2) p.ids[0] |= 1u << back;
        }
    }
    static void draw_value(Piece& p, uint32_t dtype, std::mt19937& rng) {
        const uint32_t es = batch_esize(dtype);
        if (rng() % 4) return;
        p.flags = LLCOMP_MI_PASTE_VALUE;
        p.value_bits = es == 4 ? uint32_t(rng()) : uint32_t(rng()) & ((1u << (8 * es)) - 1u);
    }
    static uint32_t shift_mask_off(uint32_t sx, uint32_t dx) { return (sx * 5 + dx * 3) % 8 * 2; }
    static void shift_ids(Piece& p, uint32_t sx, uint32_t dx) { p.id_base = (sx ^ dx) & 1 ? 0 : 0x0100, p.ids[0] = (sx ^ dx) & 2 ? 0x7u : 0x2u; }
    static void many_ids(Piece& p, std::mt19937& rng) { p.id_base = kPool[rng() % 8], p.ids[0] = 1u | 1u << (rng() % 8); }
};

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

uint32_t g_mask_units = 0;

template <uint32_t MB>
int run(const Call<typename Width<MB>::Piece>& c, std::mt19937& rng) {
    using P = typename Width<MB>::Piece;
    const uint32_t es = batch_esize(c.dtype);
    const bool chw = c.layout == LLCOMP_MI_LAYOUT_CHW;
    const size_t src_bytes = size_t(c.n_src) * c.c * c.iw * c.ih * es, dst_bytes = size_t(c.n_dst) * c.c * c.ow * c.oh * es;
    const size_t mask_bytes = MB * size_t(c.n_src) * c.iw * c.ih;
    // operator new[] aligns to 16: the batches begin their offsets behind that and end where their arrays end
    std::unique_ptr<uint8_t[]> src_buf(new uint8_t[c.src_off + src_bytes]), dst_buf(new uint8_t[c.dst_off + dst_bytes]), ref(new uint8_t[dst_bytes]);
    std::unique_ptr<uint8_t[]> mask_buf(new uint8_t[c.mask_off + mask_bytes]);
    CHECK(reinterpret_cast<uintptr_t>(src_buf.get()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_buf.get()) % 16 == 0);
    CHECK(reinterpret_cast<uintptr_t>(mask_buf.get()) % 16 == 0 && c.mask_off % MB == 0);
    uint8_t* src = src_buf.get() + c.src_off;
    uint8_t* dst = dst_buf.get() + c.dst_off;
    uint8_t* mask = c.alias ? src : mask_buf.get() + c.mask_off;
    CHECK(!c.alias || (src_bytes == mask_bytes && Width<MB>::alias_ok(c, es, chw)));
    Width<MB>::fill(src, src_bytes, mask, mask_bytes, c.alias, rng);
    for (size_t i = 0; i < dst_bytes; ++i) dst[i] = uint8_t(rng());
    const P* pieces = c.pieces.empty() ? nullptr : c.pieces.data();
    const uint32_t n_pieces = uint32_t(c.pieces.size());
    CHECK(paste_reference(src, mask, c.n_src, c.iw, c.ih, dst, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, ref.get()) == LLCOMP_MI_OK);

    std::vector<uint32_t> value_bits;
    CHECK(paste_check_call(c.n_src, c.iw, c.ih, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, value_bits) == LLCOMP_MI_OK);
    CHECK(paste_check_memory(src, src_bytes, mask, mask_bytes, dst, dst_bytes, es, MB, n_pieces) == LLCOMP_MI_OK);
    PastePlan p;
    paste_plan(c.n_dst, pieces, n_pieces, p);
    // the plan: the samples ascending, their runs a partition of the pieces that are not ignored, each run in the call's order
    size_t at = 0, live = 0;
    for (const P& q : c.pieces) live += !paste_idle(q);
    CHECK(p.order.size() == live);
    for (size_t j = 0; j < p.samples.size(); ++j) {
        const ComposeSample& s = p.samples[j];
        CHECK(s.dst < c.n_dst && (!j || p.samples[j - 1].dst < s.dst) && s.first == at && s.count);
        for (uint32_t i = 0; i < s.count; ++i) {
            const uint32_t pi = p.order[s.first + i];
            CHECK(pi < n_pieces && c.pieces[pi].dst == s.dst && !paste_idle(c.pieces[pi]) && (!i || p.order[s.first + i - 1] < pi));
        }
        at += s.count;
    }
    CHECK(at == live);
    const PasteTable<MB> t(p.samples.size(), p.order.size());
    CHECK(t.bytes <= paste_table_bound<MB>(c.n_dst, n_pieces));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes + 1]);
    paste_table_put(pieces, p, value_bits, c.c, c.layout, table.get());
    std::vector<ComposeSample> samples(p.samples.size());
    std::vector<PasteRec<MB>> recs(p.order.size());
    if (!samples.empty()) std::memcpy(samples.data(), table.get() + t.samples_at, samples.size() * sizeof(ComposeSample));
    if (!recs.empty()) std::memcpy(recs.data(), table.get() + t.recs_at, recs.size() * sizeof(PasteRec<MB>));

    const PasteGeom pg = paste_geom<MB>(reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(mask), c.n_src,
                                        c.iw, c.ih, c.ow, c.oh, c.c, es, chw);
    CHECK(pg.mask_bytes == mask_bytes);
    CHECK(paste_workgroups(p, c.ow, c.oh, c.c, c.dtype, c.layout) == uint64_t(samples.size()) * pg.g.planes * pg.g.tiles_x * pg.g.tiles_y);
    HostMem mem{pg.g.src, src_bytes, pg.mask, mask_bytes, pg.g.dst, dst_bytes, es, std::vector<uint8_t>(dst_bytes, 0)};
    bool cap_ok = true;
    if (es == 1) walk<MB, 1>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    else if (es == 2) walk<MB, 2>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    else walk<MB, 4>(pg, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    CHECK(!mem.bad && cap_ok);
    g_mask_units += mem.mask_units;
    CHECK(std::memcmp(dst, ref.get(), dst_bytes) == 0);
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

const uint32_t kDtypes[4] = {LLCOMP_MI_DTYPE_U8, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_DTYPE_BF16, LLCOMP_MI_DTYPE_F32};
const uint32_t kLayouts[2] = {LLCOMP_MI_LAYOUT_CHW, LLCOMP_MI_LAYOUT_HWC};

// a drawn call: pieces that overlap, hide each other, are empty or VALUE; big: shapes that cross the tile's borders
template <uint32_t MB>
Call<typename Width<MB>::Piece> draw(uint32_t dtype, uint32_t layout, uint32_t first_off, uint32_t dst_off, bool big, std::mt19937& rng) {
    using P = typename Width<MB>::Piece;
    Call<P> c{};
    c.dtype = dtype, c.layout = layout, c.dst_off = dst_off;
    Width<MB>::begin(c, first_off, rng);
    const uint32_t rows = compose_tile_rows(batch_esize(dtype) * (layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c.c));
    c.n_src = 1 + rng() % 3, c.n_dst = 1 + rng() % 3;
    c.iw = 1 + rng() % (big ? 160 : 40), c.ih = 1 + rng() % (big ? 24 : 9);
    c.ow = big ? kComposeTile - 2 + rng() % (kComposeTile + 5) : 1 + rng() % 48;
    c.oh = big ? rows - 1 + rng() % (rows + 3) : 1 + rng() % 9;
    const uint32_t n = rng() % 9;
    for (uint32_t i = 0; i < n; ++i) {
        P p{};
        p.dst = rng() % c.n_dst;
        const uint32_t mw = c.iw > c.ow ? c.ow : c.iw, mh = c.ih > c.oh ? c.oh : c.ih;
        p.w = rng() % 8 ? 1 + rng() % mw : 0, p.h = rng() % 8 ? 1 + rng() % mh : 0;
        p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1);
        p.src = rng() % c.n_src, p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1);
        Width<MB>::draw_ids(p, rng);
        Width<MB>::draw_value(p, dtype, rng);
        c.pieces.push_back(p);
    }
    return c;
}

// the refusals of either piece type: the shapes, the rectangles, the flags, the counts, the cap on one dst sample
template <class P>
int check_shared_refusals() {
    std::vector<uint32_t> bits(1, 77u);
    P ok{};
    ok.w = 4, ok.h = 4, ok.ids[0] = 2;
    auto call = [&](const P& p, uint32_t n_src = 2, uint32_t n_dst = 2, uint32_t c = 3, uint32_t dtype = LLCOMP_MI_DTYPE_F16,
                    uint32_t layout = LLCOMP_MI_LAYOUT_CHW, uint32_t n_pieces = 1) {
        return paste_check_call(n_src, 8, 8, n_dst, 8, 8, c, dtype, layout, &p, n_pieces, bits);
    };
    CHECK(call(ok) == LLCOMP_MI_OK && bits.size() == 1 && bits[0] == 0);
    bits.assign(1, 77u);
    P p = ok;
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
    CHECK(call(ok, 0) == LLCOMP_MI_BAD_ARGS && call(ok, 65536) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 0) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 65536) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 2, 0) == LLCOMP_MI_BAD_ARGS && call(ok, 2, 2, 3, 4) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, 2) == LLCOMP_MI_BAD_ARGS);
    CHECK(call(ok, 2, 2, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, kPasteMaxPieces + 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(bits.size() == 1 && bits[0] == 77u);  // (a refused call leaves value_bits alone)
    const P* none = nullptr;
    CHECK(paste_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, none, 1, bits) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_call(0, 0, 0, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, none, 0, bits) == LLCOMP_MI_OK && bits.empty());
    bits.assign(1, 77u);
    CHECK(paste_check_call(2, 1u << 31, 1, 2, 8, 8, 1, LLCOMP_MI_DTYPE_U8, LLCOMP_MI_LAYOUT_CHW, none, 0, bits) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_call(2, 8, 8, 2, 1u << 30, 1, 3, LLCOMP_MI_DTYPE_U8, LLCOMP_MI_LAYOUT_HWC, none, 0, bits) == LLCOMP_MI_BAD_ARGS);
    // the cap on one dst sample: empty pieces do not count, pieces without an id bit do
    std::vector<P> many(kPasteMaxPiecesPerSample + 1, ok);
    many[3].w = 0;
    CHECK(paste_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), bits) == LLCOMP_MI_OK);
    bits.assign(1, 77u);
    many[3].w = 4, many[3].ids[0] = 0;
    CHECK(paste_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), bits) == LLCOMP_MI_BAD_ARGS);
    many[3].dst = 1;
    CHECK(paste_check_call(2, 8, 8, 2, 8, 8, 3, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_CHW, many.data(), uint32_t(many.size()), bits) == LLCOMP_MI_OK);
    return 0;
}

// ... and a width's own: its values, its window, its mask's alignment
int check_refusals(Width<1>) {
    if (check_shared_refusals<llcomp_mi_paste_piece>()) return 1;
    std::vector<uint32_t> bits(1, 77u);
    llcomp_mi_paste_piece ok{};
    ok.w = 4, ok.h = 4, ok.ids[0] = 2;
    auto call = [&](const llcomp_mi_paste_piece& p, uint32_t dtype = LLCOMP_MI_DTYPE_F16) {
        return paste_check_call(2, 8, 8, 2, 8, 8, 3, dtype, LLCOMP_MI_LAYOUT_CHW, &p, 1, bits);
    };
    llcomp_mi_paste_piece p = ok;
    p.value = 1.0f;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.flags = LLCOMP_MI_PASTE_VALUE, p.value = 1.0f / 0.0f;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.flags = LLCOMP_MI_PASTE_VALUE, p.value = 0.5f;
    CHECK(call(p, LLCOMP_MI_DTYPE_U8) == LLCOMP_MI_BAD_ARGS && call(p, LLCOMP_MI_DTYPE_F16) == LLCOMP_MI_OK && bits[0] == 0x3800u);
    p.value = 256.0f;
    CHECK(call(p, LLCOMP_MI_DTYPE_U8) == LLCOMP_MI_BAD_ARGS);
    p.value = 255.0f;
    CHECK(call(p, LLCOMP_MI_DTYPE_U8) == LLCOMP_MI_OK && bits[0] == 255u);
    // memory: NULL, alignment, overlap of dst with src or mask; src and mask may be one buffer
    alignas(16) static uint8_t m[96];
    CHECK(paste_check_memory(m, 16, m + 3, 8, m + 16, 16, 2, 1, 1) == LLCOMP_MI_OK && paste_check_memory(m, 17, m, 8, m + 16, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_memory(m, 16, m + 31, 2, m + 16, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS && paste_check_memory(m, 16, m + 32, 2, m + 16, 16, 1, 1, 1) == LLCOMP_MI_OK);
    CHECK(paste_check_memory(m, 16, m + 15, 2, m + 16, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS && paste_check_memory(m, 16, m, 16, m + 16, 16, 1, 1, 1) == LLCOMP_MI_OK);
    CHECK(paste_check_memory(nullptr, 16, m, 8, m + 16, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS && paste_check_memory(m, 16, nullptr, 8, m + 16, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_memory(nullptr, 0, nullptr, 0, m + 16, 16, 1, 1, 0) == LLCOMP_MI_OK && paste_check_memory(m, 16, m, 8, nullptr, 16, 1, 1, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_memory(m + 1, 16, m, 8, m + 32, 16, 2, 1, 1) == LLCOMP_MI_BAD_ARGS && paste_check_memory(m, 16, m, 8, m + 33, 16, 2, 1, 1) == LLCOMP_MI_BAD_ARGS);
    return 0;
}
int check_refusals(Width<2>) {
    if (check_shared_refusals<llcomp_mi_paste_piece16>()) return 1;
    std::vector<uint32_t> bits;
    llcomp_mi_paste_piece16 ok{};
    ok.w = 4, ok.h = 4, ok.ids[0] = 2;
    auto call = [&](const llcomp_mi_paste_piece16& p, uint32_t dtype = LLCOMP_MI_DTYPE_F16) {
        return paste_check_call(2, 8, 8, 2, 8, 8, 3, dtype, LLCOMP_MI_LAYOUT_CHW, &p, 1, bits);
    };
    llcomp_mi_paste_piece16 p = ok;
    p.value_bits = 1;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.id_base = 65536;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS);
    p = ok, p.id_base = 65535;
    CHECK(call(p) == LLCOMP_MI_OK && paste_idle(p));
    p.ids[0] = 1;
    CHECK(!paste_idle(p));
    p = ok, p.flags = LLCOMP_MI_PASTE_VALUE, p.value_bits = 0x10000;
    CHECK(call(p) == LLCOMP_MI_BAD_ARGS && call(p, LLCOMP_MI_DTYPE_F32) == LLCOMP_MI_OK && bits[0] == 0x10000u);
    p.value_bits = 0xFFFF;
    CHECK(call(p) == LLCOMP_MI_OK && call(p, LLCOMP_MI_DTYPE_U8) == LLCOMP_MI_BAD_ARGS);
    p.value_bits = 0xFF;
    CHECK(call(p, LLCOMP_MI_DTYPE_U8) == LLCOMP_MI_OK && bits[0] == 0xFFu);
    // memory: the 8-bit call's cases, and a mask at an odd address
    alignas(16) static uint8_t m[96];
    CHECK(paste_check_memory(m, 16, m + 4, 8, m + 16, 16, 2, 2, 1) == LLCOMP_MI_OK && paste_check_memory(m, 16, m + 3, 8, m + 16, 16, 2, 2, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_memory(m, 16, m, 16, m + 16, 16, 2, 2, 1) == LLCOMP_MI_OK && paste_check_memory(m, 16, m + 10, 8, m + 16, 16, 1, 2, 1) == LLCOMP_MI_BAD_ARGS);
    CHECK(paste_check_memory(nullptr, 0, nullptr, 0, m + 16, 16, 1, 2, 0) == LLCOMP_MI_OK && paste_check_memory(m, 16, nullptr, 8, m + 16, 16, 1, 2, 1) == LLCOMP_MI_BAD_ARGS);
    return 0;
}

template <uint32_t MB>
int rounds_of() {
    using W = Width<MB>;
    using P = typename W::Piece;
    std::mt19937 rng(W::kSeed);
    uint32_t rounds = 0;
    // every byte offset of src (MB 1) or every even byte offset of the mask (MB 2) against every byte offset of dst that the element
    // allows: small drawn calls.  The batches end where their arrays end, so a mask at an offset begins and ends inside an aligned unit at
    // the batch's first and last bytes
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts) {
            const uint32_t es = batch_esize(dtype), step = MB == 1 ? es : 2;
            for (uint32_t fo = 0; fo < 16; fo += step)
                for (uint32_t d0 = 0; d0 < 16; d0 += es, ++rounds)
                    if (run<MB>(draw<MB>(dtype, layout, fo, d0, false, rng), rng)) return 1;
        }
    // shapes around the tile's borders, offsets drawn
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts) {
            const uint32_t es = batch_esize(dtype), step = MB == 1 ? es : 2;
            for (uint32_t i = 0; i < 12; ++i, ++rounds) {
                const uint32_t fo = rng() % 16 / step * step, d0 = rng() % 16 / es * es;
                if (run<MB>(draw<MB>(dtype, layout, fo, d0, true, rng), rng)) return 1;
            }
        }
    // all 16 x 16 pairs of sx and dx -- all 16 shifts of the shifted copies -- with one-row pieces of the width's lengths, for every element
    // size and HWC c = 3
    const uint32_t units_before = g_mask_units;
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t sx = 0; sx < 16; ++sx)
                for (uint32_t dx = 0; dx < 16; ++dx, ++rounds) {
                    Call<P> c{};
                    c.dtype = dtype, c.layout = layout, c.c = layout == LLCOMP_MI_LAYOUT_HWC ? 3 : 1;
                    c.n_src = 1, c.iw = 52, c.ih = 3, c.n_dst = W::kNWidths, c.ow = 50, c.oh = 2, c.mask_off = W::shift_mask_off(sx, dx);
                    for (uint32_t i = 0; i < W::kNWidths; ++i) {
                        P p{};
                        p.dst = i, p.dx = dx, p.sx = sx, p.dy = i & 1, p.sy = 1 + (i & 1), p.w = W::kWidths[i], p.h = 1;
                        W::shift_ids(p, sx, dx);
                        c.pieces.push_back(p);
                    }
                    if (run<MB>(c, rng)) return 1;
                }
    CHECK(g_mask_units > units_before);
    // one dst sample with as many pieces as the list holds
    for (uint32_t layout : kLayouts) {
        Call<P> c{};
        c.dtype = LLCOMP_MI_DTYPE_F16, c.layout = layout, c.c = 3, c.src_off = 2, c.dst_off = 6, c.mask_off = W::kManyMaskOff;
        c.n_src = 2, c.iw = 9, c.ih = 7, c.n_dst = 2, c.ow = kComposeTile + 3, c.oh = 5;
        for (uint32_t i = 0; i < kPasteMaxPiecesPerSample + 30; ++i) {
            P p{};
            p.dst = i < kPasteMaxPiecesPerSample ? 1 : 0, p.src = rng() % 2, p.w = 1 + rng() % 9, p.h = 1 + rng() % 5;
            p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1), p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1);
            W::many_ids(p, rng);
            W::draw_value(p, c.dtype, rng);
            c.pieces.push_back(p);
        }
        if (run<MB>(c, rng)) return 1;
        ++rounds;
    }
    if (check_refusals(W{})) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const int bits = argc == 2 ? std::atoi(argv[1]) : 0;
    if (bits == 8) return rounds_of<1>();
    if (bits == 16) return rounds_of<2>();
    std::printf("usage: paste_check 8|16\n");
    return 2;
}
