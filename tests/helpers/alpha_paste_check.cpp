// alpha_paste_check.cpp -- the batch alpha paste (llcomp_amd/csrc/alpha_rule.hpp, alpha_plan.cpp) walked on the host under a sanitizer
// as tests/helpers/paste_check.cpp walks the copy-paste: k_alpha_paste<AB, DT>'s workgroups (a tile of a plane of a dst sample, its
// short list) and threads through a memory that checks every access -- reads inside the src, the alpha or the dst batch, writes inside
// the dst batch, 16-byte accesses aligned and elements at multiples of their size; src and alpha are never written; every byte of dst
// is written at most once, and only by the one thread of the one workgroup that owns its (row, unit), which alone reads it as an element; an
// element no piece reaches is never written -- and compared with llcomp_mi_alpha_paste_reference bit for bit.  Host code only; built
// and run by tests/test_alpha_paste_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/alpha_paste_check.cpp llcomp_amd/csrc/alpha_plan.cpp llcomp_amd/csrc/paste_plan.cpp
// Prints "ok <rounds>".
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "alpha_plan.hpp"
#include "alpha_rule.hpp"

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
    uint64_t src, src_bytes, alpha, alpha_bytes, dst, dst_bytes;
    uint32_t es;
    std::vector<uint8_t> written;  // per byte of dst
    std::vector<uint32_t> owner;   // per byte of dst: the thread that read it as an element or wrote it, 0 for none
    uint32_t who = 0;              // the thread at work: 1 + workgroup * 256 + tid
    bool bad = false;
    int why = 0;  // the line of the first refusal
    void flag(int line) { bad = true, why = why ? why : line; }

    bool readable(uint64_t a, uint64_t n) { return (src && a >= src && a + n <= src + src_bytes) || (alpha && a >= alpha && a + n <= alpha + alpha_bytes); }
    bool in_dst(uint64_t a, uint64_t n) { return a >= dst && a + n <= dst + dst_bytes; }
    bool own(uint64_t a, uint64_t n) {  // the bytes of dst belong to the thread at work: nobody else read them as elements or wrote them
        bool mine = true;
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t& o = owner[size_t(a - dst + i)];
            if (!o) o = who;
            mine = mine && o == who;
        }
        return mine;
    }
    void count(uint64_t a, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) ++written[size_t(a - dst + i)];
    }
    ComposeChunk load16(uint64_t a) {
        ComposeChunk c{{0, 0, 0, 0}};
        if (a & 15) return flag(__LINE__), c;
        if (!in_dst(a, 16) && !readable(a, 16)) {  // (a unit of dst read whole holds the neighbouring rows' elements too, which are dropped)
            return flag(__LINE__), c;
        }
        std::memcpy(&c, reinterpret_cast<const void*>(uintptr_t(a)), 16);
        return c;
    }
    void store16(uint64_t a, const ComposeChunk& c) {
        if ((a & 15) || !in_dst(a, 16) || !own(a, 16)) return flag(__LINE__);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &c, 16);
        count(a, 16);
    }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) {
        uint32_t v = 0;
        if (a & (N - 1)) return flag(__LINE__), v;
        if (in_dst(a, N)) {
            if (N != es || !own(a, N)) return flag(__LINE__), v;
        } else if (!readable(a, N)) {
            return flag(__LINE__), v;
        }
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);
        return v;
    }
    template <uint32_t N>
    void store_el(uint64_t a, uint32_t bits) {
        if (N != es || (a & (es - 1)) || !in_dst(a, es) || !own(a, es)) return flag(__LINE__);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &bits, es);
        count(a, es);
    }
};

struct Call {
    uint32_t n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, apx, ab;
    std::vector<llcomp_mi_alpha_piece> pieces;
    uint32_t src_off, dst_off, alpha_off;  // bytes past a multiple of 16
    bool alias;                            // the alpha batch IS the src batch
};

template <uint32_t AB, uint32_t DT, bool OVER>
void walk(const AlphaGeom& ag, const ComposeSample* samples, uint32_t n_samples, const AlphaRec* recs, HostMem& mem, bool& cap_ok) {
    constexpr uint32_t ES = batch_esize(DT);
    const ComposeGeom& g = ag.pg.g;
    uint32_t wg = 0;
    for (uint32_t z = 0; z < n_samples; ++z)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t tile = 0; tile < g.tiles_x * g.tiles_y; ++tile, ++wg) {  // one workgroup
                const ComposeTileBox box = compose_tile_box(g, ES, tile);
                std::vector<AlphaRec> list;  // the short list
                if (samples[z].count > kPasteMaxPiecesPerSample) cap_ok = false;
                for (uint32_t i = 0; i < samples[z].count; ++i)
                    if (compose_hits(recs[samples[z].first + i].r, box)) list.push_back(recs[samples[z].first + i]);
                AlphaWork k;
                k.list = list.data(), k.n_list = uint32_t(list.size()), k.d = samples[z].dst, k.pl = pl, k.w = kAlphaWeights.w;
                if (!k.n_list) continue;
                for (uint32_t tid = 0; tid < 256; ++tid) {
                    mem.who = 1 + wg * 256 + tid;
                    alpha_tile_pass<AB, DT, OVER>(ag, k, box, tid, 256, mem);
                }
            }
}
template <uint32_t AB>
void walk_of(uint32_t dtype, bool over, const AlphaGeom& ag, const ComposeSample* samples, uint32_t n_samples, const AlphaRec* recs, HostMem& mem, bool& cap_ok) {
    switch (dtype) {  // (the launcher's switch: alpha_kernels.hip)
        case LLCOMP_MI_DTYPE_U8:
            if (over) walk<AB, LLCOMP_MI_DTYPE_U8, true>(ag, samples, n_samples, recs, mem, cap_ok);
            else walk<AB, LLCOMP_MI_DTYPE_U8, false>(ag, samples, n_samples, recs, mem, cap_ok);
            break;
        case LLCOMP_MI_DTYPE_F32: walk<AB, LLCOMP_MI_DTYPE_F32, false>(ag, samples, n_samples, recs, mem, cap_ok); break;
        case LLCOMP_MI_DTYPE_F16: walk<AB, LLCOMP_MI_DTYPE_F16, false>(ag, samples, n_samples, recs, mem, cap_ok); break;
        default: walk<AB, LLCOMP_MI_DTYPE_BF16, false>(ag, samples, n_samples, recs, mem, cap_ok); break;
    }
}

template <uint32_t AB>
int run_width(const Call& c, std::mt19937& rng) {
    const uint32_t es = batch_esize(c.dtype);
    const bool chw = c.layout == LLCOMP_MI_LAYOUT_CHW;
    const size_t src_bytes = size_t(c.n_src) * c.c * c.iw * c.ih * es, dst_bytes = size_t(c.n_dst) * c.c * c.ow * c.oh * es;
    const size_t alpha_bytes = AB * size_t(c.n_src) * c.iw * c.ih;
    // operator new[] aligns to 16: the batches begin their offsets behind that and end where their arrays end
    std::unique_ptr<uint8_t[]> src_buf(new uint8_t[c.src_off + src_bytes]), dst_buf(new uint8_t[c.dst_off + dst_bytes]), ref(new uint8_t[dst_bytes]);
    std::unique_ptr<uint8_t[]> alpha_buf(new uint8_t[c.alpha_off + alpha_bytes]), src_copy(new uint8_t[src_bytes]), alpha_copy(new uint8_t[alpha_bytes]);
    CHECK(reinterpret_cast<uintptr_t>(src_buf.get()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_buf.get()) % 16 == 0);
    CHECK(reinterpret_cast<uintptr_t>(alpha_buf.get()) % 16 == 0 && reinterpret_cast<uintptr_t>(ref.get()) % 4 == 0);
    uint8_t* src = src_buf.get() + c.src_off;
    uint8_t* dst = dst_buf.get() + c.dst_off;
    uint8_t* alpha = c.alias ? src : alpha_buf.get() + c.alpha_off;
    CHECK(!c.alias || src_bytes == alpha_bytes);
    for (size_t i = 0; i < src_bytes; ++i) src[i] = uint8_t(rng());
    if (!c.alias)
        for (size_t i = 0; i < alpha_bytes; ++i) alpha[i] = uint8_t(rng());
    for (size_t i = c.ab; i < alpha_bytes; i += AB) {  // a soft matte: runs of 0 and 255 between noise
        const uint32_t kind = rng() % 4;
        if (kind < 2) alpha[i] = kind ? 255 : 0;
    }
    std::memcpy(src_copy.get(), src, src_bytes);
    std::memcpy(alpha_copy.get(), alpha, alpha_bytes);
    for (size_t i = 0; i < dst_bytes; ++i) dst[i] = uint8_t(rng());
    const llcomp_mi_alpha_piece* pieces = c.pieces.empty() ? nullptr : c.pieces.data();
    const uint32_t n_pieces = uint32_t(c.pieces.size());
    CHECK(llcomp_mi_alpha_paste_reference(src, alpha, AB, c.ab, c.n_src, c.iw, c.ih, dst, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, ref.get()) ==
          LLCOMP_MI_OK);

    AlphaUses uses;
    CHECK(alpha_check_call(AB, c.ab, c.n_src, c.iw, c.ih, c.n_dst, c.ow, c.oh, c.c, c.dtype, c.layout, pieces, n_pieces, uses) == LLCOMP_MI_OK);
    CHECK(alpha_check_memory(src, src_bytes, alpha, alpha_bytes, dst, dst_bytes, es, uses) == LLCOMP_MI_OK);
    PastePlan p;
    alpha_plan(c.n_dst, pieces, n_pieces, p);
    size_t live = 0;
    for (const llcomp_mi_alpha_piece& q : c.pieces) live += !alpha_idle(q);
    CHECK(p.order.size() == live);
    const AlphaTable t(p.samples.size(), p.order.size());
    CHECK(t.bytes <= alpha_table_bound(c.n_dst, n_pieces));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes + 1]);
    alpha_table_put(pieces, p, c.c, c.layout, table.get());
    std::vector<ComposeSample> samples(p.samples.size());
    std::vector<AlphaRec> recs(p.order.size());
    if (!samples.empty()) std::memcpy(static_cast<void*>(samples.data()), table.get() + t.samples_at, samples.size() * sizeof(ComposeSample));
    if (!recs.empty()) std::memcpy(static_cast<void*>(recs.data()), table.get() + t.recs_at, recs.size() * sizeof(AlphaRec));

    const AlphaGeom ag = alpha_geom<AB>(reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(alpha), c.ab, c.n_src, c.iw,
                                        c.ih, c.n_dst, c.ow, c.oh, c.c, es, chw);
    CHECK(ag.pg.mask_bytes == alpha_bytes && ag.dst_bytes == dst_bytes && ag.pg.g.src_bytes == src_bytes);
    HostMem mem{ag.pg.g.src, src_bytes, ag.pg.mask, alpha_bytes, ag.pg.g.dst, dst_bytes, es, std::vector<uint8_t>(dst_bytes, 0),
                std::vector<uint32_t>(dst_bytes, 0u)};
    bool cap_ok = true;
    walk_of<AB>(c.dtype, uses.over, ag, samples.data(), uint32_t(samples.size()), recs.data(), mem, cap_ok);
    if (mem.bad) std::printf("refused at line %d: dtype %u layout %u c %u apx %u ab %u offsets %u %u %u alias %d\n", mem.why, c.dtype, c.layout, c.c, c.apx, c.ab, c.src_off, c.dst_off, c.alpha_off, int(c.alias));
    CHECK(!mem.bad && cap_ok);
    CHECK(std::memcmp(dst, ref.get(), dst_bytes) == 0);
    CHECK(std::memcmp(src, src_copy.get(), src_bytes) == 0 && std::memcmp(alpha, alpha_copy.get(), alpha_bytes) == 0);
    // every byte at most once; an element no piece reaches never
    const uint32_t cs = chw ? 1u : c.c, planes = chw ? c.c : 1u;
    size_t byte = 0;
    for (uint32_t d = 0; d < c.n_dst; ++d)
        for (uint32_t pl = 0; pl < planes; ++pl)
            for (uint32_t y = 0; y < c.oh; ++y)
                for (uint32_t x = 0; x < c.ow; ++x) {
                    bool reached = false;
                    for (size_t i = 0; i < c.pieces.size() && !reached; ++i) reached = c.pieces[i].dst == d && alpha_covers(c.pieces[i], x, y);
                    for (uint32_t b = 0; b < cs * es; ++b, ++byte) CHECK(mem.written[byte] <= (reached ? 1 : 0));
                }
    CHECK(byte == dst_bytes);
    return 0;
}
int run(const Call& c, std::mt19937& rng) {
    return c.apx == 1 ? run_width<1>(c, rng) : c.apx == 2 ? run_width<2>(c, rng) : c.apx == 3 ? run_width<3>(c, rng) : run_width<4>(c, rng);
}

void draw_value(llcomp_mi_alpha_piece& p, const Call& c, std::mt19937& rng) {
    const uint32_t es = batch_esize(c.dtype), kind = rng() % 6;
    const bool u8_hwc = c.dtype == LLCOMP_MI_DTYPE_U8 && c.layout == LLCOMP_MI_LAYOUT_HWC;
    if (kind == 0) {
        p.flags = LLCOMP_MI_ALPHA_VALUE, p.value_bits = es == 4 ? uint32_t(rng()) : uint32_t(rng()) & ((1u << (8 * es)) - 1u);
    } else if (kind == 1 && u8_hwc && c.c <= 4) {
        p.flags = LLCOMP_MI_ALPHA_VALUE | LLCOMP_MI_ALPHA_VALUE_PIXEL, p.value_bits = c.c == 4 ? uint32_t(rng()) : uint32_t(rng()) & ((1u << (8 * c.c)) - 1u);
    }
}
llcomp_mi_alpha_piece draw_piece(const Call& c, std::mt19937& rng, uint32_t max_w = 0) {
    llcomp_mi_alpha_piece p{};
    const uint32_t mw = c.iw < c.ow ? c.iw : c.ow, mh = c.ih < c.oh ? c.ih : c.oh;
    p.dst = rng() % c.n_dst, p.src = rng() % c.n_src;
    p.w = rng() % 8 == 0 ? 0 : 1 + rng() % (max_w && max_w < mw ? max_w : mw), p.h = 1 + rng() % mh;
    p.sx = rng() % (c.iw - p.w + 1), p.sy = rng() % (c.ih - p.h + 1), p.dx = rng() % (c.ow - p.w + 1), p.dy = rng() % (c.oh - p.h + 1);
    return p;
}

const uint32_t kDtypes[4] = {LLCOMP_MI_DTYPE_U8, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_DTYPE_BF16, LLCOMP_MI_DTYPE_F32};
const uint32_t kLayouts[2] = {LLCOMP_MI_LAYOUT_CHW, LLCOMP_MI_LAYOUT_HWC};
// every alpha_px_bytes with every alpha_byte
const uint32_t kAlphas[10][2] = {{1, 0}, {2, 0}, {2, 1}, {3, 0}, {3, 1}, {3, 2}, {4, 0}, {4, 1}, {4, 2}, {4, 3}};

// a drawn call: pieces that overlap, are empty or VALUE; the alpha batch is the src batch half the time where the shapes allow
Call draw(uint32_t dtype, uint32_t layout, uint32_t src_off, uint32_t dst_off, uint32_t round, std::mt19937& rng) {
    const uint32_t es = batch_esize(dtype);
    Call c{};
    c.dtype = dtype, c.layout = layout, c.src_off = src_off, c.dst_off = dst_off, c.alpha_off = rng() % 16;
    c.apx = kAlphas[round % 10][0], c.ab = kAlphas[round % 10][1];
    c.c = 1 + rng() % 5;
    if (es == 1 && layout == LLCOMP_MI_LAYOUT_HWC && rng() % 2) c.alias = true, c.c = c.apx;
    c.n_src = 1 + rng() % 2, c.n_dst = 1 + rng() % 2;
    c.iw = 1 + rng() % 40, c.ih = 1 + rng() % 5, c.ow = 1 + rng() % 40, c.oh = 1 + rng() % 5;
    const uint32_t n = rng() % 7;
    for (uint32_t i = 0; i < n; ++i) {
        llcomp_mi_alpha_piece p = draw_piece(c, rng);
        draw_value(p, c, rng);
        c.pieces.push_back(p);
    }
    return c;
}

int rounds_of(std::mt19937& rng, uint32_t& rounds) {
    // 4 dtypes x 2 layouts x every byte offset of src and of dst that the element allows; alpha_px_bytes and alpha_byte in turn
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t src_off = 0; src_off < 16; src_off += batch_esize(dtype))
                for (uint32_t dst_off = 0; dst_off < 16; dst_off += batch_esize(dtype)) {
                    if (run(draw(dtype, layout, src_off, dst_off, rounds, rng), rng)) return 1;
                    ++rounds;
                }
    // shapes around the tile's borders: a tile and five pixels across, the tile's rows and three down, pieces across every border
    for (uint32_t dtype : kDtypes)
        for (uint32_t layout : kLayouts)
            for (uint32_t k = 0; k < 10; ++k) {
                Call c{};
                c.dtype = dtype, c.layout = layout, c.c = 3, c.apx = kAlphas[k][0], c.ab = kAlphas[k][1];
                c.src_off = rng() % 16 / batch_esize(dtype) * batch_esize(dtype), c.dst_off = rng() % 16 / batch_esize(dtype) * batch_esize(dtype), c.alpha_off = rng() % 16;
                const uint32_t rows = compose_tile_rows((layout == LLCOMP_MI_LAYOUT_CHW ? 1 : c.c) * batch_esize(dtype));
                c.n_src = 2, c.n_dst = 2, c.ow = kComposeTile + 5, c.oh = rows + 3, c.iw = kComposeTile + 9, c.ih = rows + 4;
                for (uint32_t i = 0; i < 6; ++i) {
                    llcomp_mi_alpha_piece p{};
                    p.dst = i & 1, p.src = (i >> 1) & 1;
                    p.dx = kComposeTile - 9 + i, p.w = c.ow - p.dx - (i % 3), p.sx = i, p.dy = rows - 2 - (i % 2), p.h = c.oh - p.dy - (i % 2), p.sy = i % 4;
                    if (i == 2) p.dx = 0, p.w = c.ow, p.sx = 3, p.dy = rows - 1, p.h = 2;
                    if (i == 3) p.dy = 0, p.h = c.oh, p.sy = 1, p.dx = kComposeTile - 1, p.w = 2;
                    draw_value(p, c, rng);
                    c.pieces.push_back(p);
                }
                if (run(c, rng)) return 1;
                ++rounds;
            }
    // 256 pieces on one dst sample
    for (uint32_t k = 0; k < 2; ++k) {
        Call c{};
        c.dtype = k ? LLCOMP_MI_DTYPE_U8 : LLCOMP_MI_DTYPE_F16, c.layout = k ? LLCOMP_MI_LAYOUT_HWC : LLCOMP_MI_LAYOUT_CHW, c.c = 3;
        c.n_src = 2, c.n_dst = 2, c.iw = 37, c.ih = 9, c.ow = 41, c.oh = 9, c.alpha_off = 7, c.dst_off = 2, c.apx = k ? 3 : 1, c.ab = k ? 2 : 0;
        for (uint32_t i = 0; i < 256; ++i) {
            llcomp_mi_alpha_piece p = draw_piece(c, rng, 20);
            p.dst = 1;
            if (!p.w) p.w = 1, p.sx = p.dx = 0;
            c.pieces.push_back(p);
        }
        if (run(c, rng)) return 1;
        ++rounds;
    }
    // OVER at every 4-byte offset of src and of dst, among PASTE and VALUE pieces, the RGBA batch its own alpha half the time
    for (uint32_t src_off = 0; src_off < 16; src_off += 4)
        for (uint32_t dst_off = 0; dst_off < 16; dst_off += 4)
            for (uint32_t k = 0; k < 2; ++k) {
                Call c{};
                c.dtype = LLCOMP_MI_DTYPE_U8, c.layout = LLCOMP_MI_LAYOUT_HWC, c.c = 4, c.src_off = src_off, c.dst_off = dst_off, c.alpha_off = rng() % 16;
                c.alias = k == 1, c.apx = k ? 4 : 1 + rng() % 4, c.ab = k ? 3 : rng() % c.apx;
                c.n_src = 2, c.n_dst = 2;
                c.iw = k ? kComposeTile + 7 : 1 + rng() % 40, c.ow = k ? kComposeTile + 3 : 1 + rng() % 40, c.ih = 1 + rng() % 5, c.oh = 1 + rng() % 5;
                const uint32_t n = 1 + rng() % 7;
                for (uint32_t i = 0; i < n; ++i) {
                    llcomp_mi_alpha_piece p = draw_piece(c, rng);
                    if (i == 0 || rng() % 2) p.flags = LLCOMP_MI_ALPHA_OVER;
                    else draw_value(p, c, rng);
                    c.pieces.push_back(p);
                }
                if (run(c, rng)) return 1;
                ++rounds;
            }
    return 0;
}

// the two rules at their ends, and the weights
int check_rules() {
    for (uint32_t m = 0; m < 256; ++m) CHECK(kAlphaWeights.w[m] == float(m) / 255.0f);
    for (uint32_t d = 0; d < 256; ++d)
        for (uint32_t s = 0; s < 256; ++s) {
            CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_U8>(d, s, 0, nullptr) == d && alpha_paste_el<LLCOMP_MI_DTYPE_U8>(d, s, 255, nullptr) == s);
            const uint32_t t = d * 127u + s * 128u + 128u;
            CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_U8>(d, s, 128, nullptr) == (((t >> 8) + t) >> 8));
        }
    CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_F32>(0x7FA55555u, 0x3F800000u, 255, kAlphaWeights.w) == 0x3F800000u);  // a NaN under an opaque pixel
    CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_F32>(0x7FA55555u, 0x3F800000u, 0, kAlphaWeights.w) == 0x7FA55555u);    // ... keeps its payload under none
    CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_F32>(0x7FA55555u, 0x3F800000u, 1, kAlphaWeights.w) == 0x7FC00000u);
    CHECK(alpha_paste_el<LLCOMP_MI_DTYPE_F16>(0x7C00u, 0xFC00u, 128, kAlphaWeights.w) == 0x7E00u);              // inf - inf
    CHECK(alpha_over_px(0x12345678u, 0x00FFFFFFu) == 0x12345678u && alpha_over_px(0x12345678u, 0xFFABCDEFu) == 0xFFABCDEFu);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(2550);
    uint32_t rounds = 0;
    if (check_rules() || rounds_of(rng, rounds)) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
