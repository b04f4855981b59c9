// alpha_rule.hpp -- the rule of the batch alpha paste (include/llcomp_mi.h: "Batch alpha paste"), stated ONCE: these functions are
// compiled into the kernel (alpha_kernels.hip), into llcomp_mi_alpha_paste_reference and the planner's checks (alpha_plan.cpp) and into
// the host check that walks the kernel's own decisions without a GPU (tests/helpers/alpha_paste_check.cpp).
//
// The batches, the tiles and the 16-byte units of dst MEMORY a tile owns are the composition's (compose_rule.hpp); the aligned units
// that hold a unit's mask pixels, their shifted copies and a VALUE piece's unit are the copy-paste's (paste_rule.hpp: PasteFetch,
// paste_load_units, PasteUnits, paste_value_unit, paste_value_pixel_unit); the binary32 arithmetic without fused multiply-adds is the
// mixing's (mix_rule.hpp: mix_widen, mix_product, mix_round, and its contraction pragma).  What is the alpha paste's own: the two rules
// per element and pixel (alpha_paste_el, alpha_over_px), the record (ComposeRec and the value, 36 bytes), and a thread's walk of the
// short list FORWARDS: it reads the unit of dst once, every piece that reaches it blends onto what the pieces before it left, and the
// unit is stored once.
// AB: the alpha batch's bytes per pixel, 1..4; the alpha of a pixel is ONE byte of it (alpha_byte), so the fetch begins at that byte
// of the first pixel and pixel j's alpha is byte AB * j of the shifted copies -- a constant place after unrolling, at any byte address.
// DT: the dtype, because the arithmetic depends on it.  Mem: batch_chunk.hpp's.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "compose_rule.hpp"
#include "mix_rule.hpp"
#include "paste_rule.hpp"

namespace llcomp_mi {

constexpr uint32_t kAlphaFlagBits = LLCOMP_MI_ALPHA_VALUE | LLCOMP_MI_ALPHA_VALUE_PIXEL | LLCOMP_MI_ALPHA_OVER;
static_assert(LLCOMP_MI_ALPHA_VALUE == LLCOMP_MI_PASTE_VALUE && LLCOMP_MI_ALPHA_VALUE_PIXEL == LLCOMP_MI_PASTE_VALUE_PIXEL, "the copy-paste's value bits");

// The 256 weights float(m) / 255.0f, divided once by the compiler so that no device division is part of the rule
struct AlphaWeights {
    float w[256];
};
constexpr AlphaWeights alpha_weights() {
    AlphaWeights t{};
    for (uint32_t m = 0; m < 256; ++m) t.w[m] = float(m) / 255.0f;
    return t;
}
inline constexpr AlphaWeights kAlphaWeights = alpha_weights();

// THE PASTE rule for one element: d and s in the dtype's bits, m the pixel's alpha byte, w the weights
template <uint32_t DT>
LLMI_HD inline uint32_t alpha_paste_el(uint32_t d, uint32_t s, uint32_t m, const float* w) {
    if (m == 0) return d;
    if (m == 255) return s;
    if constexpr (DT == LLCOMP_MI_DTYPE_U8) {
        const uint32_t t = d * (255u - m) + s * m + 128u;
        return ((t >> 8) + t) >> 8;
    } else {
        const float a = w[m];
        const float pd = mix_product(mix_widen<DT>(d), 1.0f - a), ps = mix_product(mix_widen<DT>(s), a);
        return mix_round<DT>(pd + ps);
    }
}
// THE OVER rule for one U8 RGBA pixel, bytes R G B A from the low byte up
LLMI_HD inline uint32_t alpha_over_px(uint32_t d, uint32_t s) {
    const uint32_t sa = s >> 24, da = d >> 24;
    if (!sa) return d;
    const uint32_t outa255 = sa * 255u + da * (255u - sa);
    const uint32_t coef1 = sa * 255u * 255u * 128u / outa255, coef2 = 255u * 128u - coef1;
    uint32_t o = 0;
    LLMI_UNROLL
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const uint32_t t = ((s >> (8 * ch)) & 0xFFu) * coef1 + ((d >> (8 * ch)) & 0xFFu) * coef2 + (0x80u << 7);
        o |= (((((t >> 8) + t) >> 8) >> 7) & 0xFFu) << (8 * ch);
    }
    const uint32_t t = outa255 + 0x80u;
    return o | ((((t >> 8) + t) >> 8) << 24);
}

template <class P>
LLMI_HD inline bool alpha_covers(const P& p, uint32_t x, uint32_t y) { return x - p.dx < p.w && y - p.dy < p.h; }
// a piece with w or h of 0 is checked and ignored
LLMI_HD inline bool alpha_idle(const llcomp_mi_alpha_piece& p) { return !p.w || !p.h; }

// A piece as the kernel reads it: ComposeRec's eight words (columns in elements) and the value in the dtype's bits
struct AlphaRec {
    ComposeRec r;
    uint32_t value;
};
static_assert(sizeof(AlphaRec) == 36, "the table's records");
LLMI_HD inline AlphaRec alpha_rec(const llcomp_mi_alpha_piece& p, uint32_t cs) {
    return AlphaRec{ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags}, p.value_bits};
}

// One call as the kernel sees it: the copy-paste's geometry with the alpha batch as its mask, AB bytes per pixel, the byte of a pixel
// that is its alpha, and where dst ends
struct AlphaGeom {
    PasteGeom pg;
    uint64_t dst_bytes;
    uint32_t alpha_byte;
};
template <uint32_t AB>
LLMI_HD inline AlphaGeom alpha_geom(uint64_t dst, uint64_t src, uint64_t alpha, uint32_t alpha_byte, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst,
                                    uint32_t ow, uint32_t oh, uint32_t c, uint32_t esize, bool chw) {
    AlphaGeom ag;
    ag.pg = paste_geom<AB>(dst, src, alpha, n_src, iw, ih, ow, oh, c, esize, chw);
    if (!src) ag.pg.g.src_bytes = 0;
    if (!alpha) ag.pg.mask_bytes = 0;
    ag.dst_bytes = uint64_t(n_dst) * c * ow * oh * esize, ag.alpha_byte = alpha_byte;
    return ag;
}
// THE address of the alpha byte of pixel (s, y, x)
template <uint32_t AB>
LLMI_HD inline uint64_t alpha_at(const AlphaGeom& ag, uint32_t s, uint32_t y, uint32_t x) {
    return paste_mask_row<AB>(ag.pg, s, y) + AB * uint64_t(x) + ag.alpha_byte;
}

// The alpha bytes of the pixels of the elements [e0, e1) of the unit's row in piece r, as the copy-paste's fetch of its mask pixels:
// `at` is the alpha byte of pixel 0, pixel j's is AB * j bytes on, so the fetch spans AB * (npx - 1) + 1 bytes
template <uint32_t AB>
LLMI_HD inline PasteFetch alpha_fetch_of(const AlphaGeom& ag, const ComposeRec& r, uint32_t y, int32_t eu, uint32_t e0, uint32_t e1) {
    const PasteGeom& pg = ag.pg;
    const uint32_t cs = pg.g.cs, se0 = r.sxe + (e0 - r.dxe), spx0 = cs == 1 ? se0 : se0 / cs;
    PasteFetch f;
    f.ph0 = se0 - spx0 * cs, f.p0 = uint32_t(int32_t(e0) - eu), f.n_el = e1 - e0;
    f.npx = cs == 1 ? f.n_el : (f.ph0 + f.n_el + cs - 1) / cs;
    f.at = alpha_at<AB>(ag, r.src, r.sy + (y - r.dy), spx0);
    f.a = f.at & ~uint64_t(15), f.sh = uint32_t(f.at & 15u), f.units = (f.sh + AB * (f.npx - 1) + 1u + 15u) / 16u;
    f.inside = f.a >= pg.mask && f.a + 16u * f.units <= pg.mask + pg.mask_bytes;
    return f;
}

// What a workgroup knows beside its geometry, the same in every thread
struct AlphaWork {
    const AlphaRec* list;  // the pieces that matter to the tile, in order
    uint32_t n_list;
    uint32_t d, pl;    // the dst sample and the plane
    const float* w;    // the 256 weights (the kernel: its copy in LDS)
};

// What a thread does with one unit of dst memory at address u in row y, decided before anything is read: nothing where no piece of the
// list reaches the unit's elements of the row; otherwise the walk from piece `hit`, the first that does, up the list; f: that piece's
// alpha units, which the tile pass asks for ahead of the walk, with the unit of dst itself (whole: it lies inside the dst batch)
struct AlphaTodo {
    uint32_t work, whole;
    PasteTodo t;
};
template <uint32_t AB, uint32_t ES>
LLMI_HD inline AlphaTodo alpha_decide(const AlphaGeom& ag, const AlphaWork& k, uint32_t y, uint64_t row_addr, uint64_t u) {
    const ComposeGeom& g = ag.pg.g;
    const uint64_t row_end = row_addr + uint64_t(g.rwd) * ES;
    AlphaTodo a{};
    PasteTodo& t = a.t;
    t.y = y, t.u = u;
    t.eu = int32_t((int64_t(u) - int64_t(row_addr)) / int64_t(ES));
    t.e_lo = t.eu > 0 ? uint32_t(t.eu) : 0u;
    t.e_hi = u + 16 < row_end ? uint32_t((u + 16 - row_addr) / ES) : g.rwd;
    t.hit = -1;
    a.whole = u >= g.dst && u + 16 <= g.dst + ag.dst_bytes;
    for (uint32_t i = 0; i < k.n_list; ++i) {
        uint32_t e0, e1;
        if (!paste_reach(k.list[i].r, t, e0, e1)) continue;
        a.work = t.work = 1, t.hit = int32_t(i);
        if (!(k.list[i].r.flags & LLCOMP_MI_ALPHA_OVER)) t.f = alpha_fetch_of<AB>(ag, k.list[i].r, y, t.eu, e0, e1);
        break;
    }
    return a;
}
// does the walk's first piece have alpha units to ask for ahead?
LLMI_HD inline bool alpha_prefetch(const AlphaTodo& a, const AlphaWork& k) {
    return a.work && !(k.list[a.t.hit].r.flags & LLCOMP_MI_ALPHA_OVER) && a.t.f.inside;
}

// byte j of a chunk, j a variable: selects, no indexed register
LLMI_CHUNK_FN uint32_t alpha_byte_of(const ComposeChunk& c, uint32_t j) {
    const uint32_t lo = j & 8u ? c.w[2] : c.w[0], hi = j & 8u ? c.w[3] : c.w[1];
    return ((j & 4u ? hi : lo) >> (8 * (j & 3u))) & 0xFFu;
}

// The alphas of the unit's elements that fetch f names, byte p for the unit's element p (zeros elsewhere): the alpha bytes of their
// pixels from the shifted copies of the aligned units that hold them (pre: already loaded when `have`), single bytes only where such a
// unit sticks out of the alpha batch; a pixel's alpha to its elements (c of them in HWC, one in CHW)
template <uint32_t AB, uint32_t ES, class Mem>
LLMI_HD inline ComposeChunk alpha_of_unit(const AlphaGeom& ag, const PasteFetch& f, bool have, const PasteUnits<AB, ES>& pre, Mem& mem) {
    constexpr uint32_t PER = 16 / ES, COPIES = kPasteCopies<AB, ES>;
    const uint32_t cs = ag.pg.g.cs;
    ComposeChunk px{{0u, 0u, 0u, 0u}};  // byte j: the alpha of pixel j
    if (f.inside) {
        PasteUnits<AB, ES> m{};
        if (have) m = pre;
        else paste_load_units(f, m, mem);
        ComposeChunk mv[COPIES];
        LLMI_UNROLL
        for (uint32_t q = 0; q < COPIES; ++q) mv[q] = f.sh ? compose_shift(m.u[q], m.u[q + 1], f.sh) : m.u[q];
        LLMI_UNROLL
        for (uint32_t j = 0; j < PER; ++j) chunk_or<1>(px.w, j, chunk_get<1>(mv[(AB * j) >> 4].w, (AB * j) & 15u));
    } else {  // at the first or the last bytes of the alpha batch: the bytes that belong, one by one
        LLMI_UNROLL
        for (uint32_t j = 0; j < PER; ++j)
            if (j < f.npx) chunk_or<1>(px.w, j, mem.template load_el<1>(f.at + AB * uint64_t(j)));
    }
    ComposeChunk el{{0u, 0u, 0u, 0u}};
    uint32_t j = 0, ph = f.ph0;
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p) {
        if (p < f.p0 || p >= f.p0 + f.n_el) continue;
        chunk_or<1>(el.w, p, alpha_byte_of(px, j));
        if (++ph == cs) ph = 0, ++j;
    }
    return el;
}

// ... and the walk.  The unit of dst as read (whole, or the row's elements of it one by one where it sticks out of the batch); the list
// from `hit` on: every piece that reaches elements of the unit blends them -- PASTE: each element under its pixel's alpha with the
// piece's own shifted copy of the unit (compose_rule.hpp) or its value, a piece whose alphas there are all 0 reads no src; OVER
// (U8 HWC c == 4, aligned to 4: a word of the unit is a pixel): each pixel under src's own alpha.  Stored once: 16 bytes where the
// pieces reached all of the unit's elements, the elements some piece reached one by one otherwise; an element no piece reaches is
// never written.  (pre is piece `hit`'s alpha units.)
template <uint32_t AB, uint32_t DT, bool OVER, class Mem>
LLMI_HD inline void alpha_finish(const AlphaGeom& ag, const AlphaWork& k, const AlphaTodo& a, const ComposeChunk& dst_unit, const PasteUnits<AB, batch_esize(DT)>& pre,
                                 Mem& mem) {
    constexpr uint32_t ES = batch_esize(DT), PER = 16 / ES;
    if (!a.work) return;
    const PasteTodo& t = a.t;
    const ComposeGeom& g = ag.pg.g;
    const uint32_t need = compose_span(uint32_t(int32_t(t.e_lo) - t.eu), uint32_t(int32_t(t.e_hi) - t.eu));
    ComposeChunk acc = dst_unit;
    if (!a.whole) {
        acc = ComposeChunk{{0u, 0u, 0u, 0u}};
        LLMI_UNROLL
        for (uint32_t p = 0; p < PER; ++p)
            if ((need >> p) & 1u) chunk_or<ES>(acc.w, p, mem.template load_el<ES>(t.u + uint64_t(p) * ES));
    }
    uint32_t reached = 0;
    for (uint32_t i = uint32_t(t.hit); i < k.n_list; ++i) {
        const AlphaRec& r = k.list[i];
        uint32_t e0, e1;
        if (!paste_reach(r.r, t, e0, e1)) continue;
        const uint32_t m = compose_span(uint32_t(int32_t(e0) - t.eu), uint32_t(int32_t(e1) - t.eu));
        reached |= m;
        const bool over = OVER && (r.r.flags & LLCOMP_MI_ALPHA_OVER);
        ComposeChunk al{{0u, 0u, 0u, 0u}};
        if (!over) {
            const bool first = int32_t(i) == t.hit;
            al = alpha_of_unit<AB, ES>(ag, first ? t.f : alpha_fetch_of<AB>(ag, r.r, t.y, t.eu, e0, e1), first, pre, mem);
            if (!(al.w[0] | al.w[1] | al.w[2] | al.w[3])) continue;
        }
        ComposeChunk v{{0u, 0u, 0u, 0u}};
        if (r.r.flags & LLCOMP_MI_ALPHA_VALUE) {
            v = paste_value_unit<ES>(r.value);
            if constexpr (ES == 1)
                if (r.r.flags & LLCOMP_MI_ALPHA_VALUE_PIXEL) v = paste_value_pixel_unit(r.value, g.cs, t.eu);
        } else {
            const uint64_t s = compose_src_of_unit(g, ES, r.r, k.pl, t.y, t.eu);
            if (compose_src_units_inside(g, s)) {
                const ComposeChunk lo = mem.load16(s & ~uint64_t(15));
                v = (s & 15u) ? compose_shift(lo, mem.load16((s & ~uint64_t(15)) + 16), uint32_t(s & 15u)) : lo;
            } else {  // at the first or the last bytes of the src batch: the elements that belong, one by one
                LLMI_UNROLL
                for (uint32_t p = 0; p < PER; ++p)
                    if ((m >> p) & 1u) chunk_or<ES>(v.w, p, mem.template load_el<ES>(s + uint64_t(p) * ES));
            }
        }
        if constexpr (OVER) {
            if (over) {
                LLMI_UNROLL
                for (uint32_t q = 0; q < 4; ++q)
                    if ((m >> (4 * q)) & 1u) acc.w[q] = alpha_over_px(acc.w[q], v.w[q]);
                continue;
            }
        }
        ComposeChunk o = acc;
        LLMI_UNROLL
        for (uint32_t p = 0; p < PER; ++p)
            chunk_set<ES>(o.w, p, alpha_paste_el<DT>(chunk_get<ES>(acc.w, p), chunk_get<ES>(v.w, p), chunk_get<1>(al.w, p), k.w));
        acc = o;
    }
    if (reached == (1u << PER) - 1u) return mem.store16(t.u, acc);
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p)
        if ((reached >> p) & 1u) mem.template store_el<ES>(t.u + uint64_t(p) * ES, chunk_get<ES>(acc.w, p));
}

// One tile's rows and units, thread `tid` of `threads`, as paste_tile_pass: a thread decides kAlphaBatch units and asks for the dst
// unit and the first piece's alpha units of all of them before it walks the first, so that its loads are in flight together.
constexpr uint32_t kAlphaBatch = 2;
template <uint32_t AB, uint32_t DT, bool OVER, class Mem>
LLMI_HD inline void alpha_tile_pass(const AlphaGeom& ag, const AlphaWork& k, const ComposeTileBox& b, uint32_t tid, uint32_t threads, Mem& mem) {
    constexpr uint32_t ES = batch_esize(DT);
    const ComposeGeom& g = ag.pg.g;
    const uint32_t upr = compose_units_per_row(g.tile_w, ES), total = (b.y1 - b.y0) * upr;
    for (uint32_t i0 = tid; i0 < total; i0 += threads * kAlphaBatch) {
        AlphaTodo todo[kAlphaBatch];
        PasteUnits<AB, ES> pre[kAlphaBatch];
        ComposeChunk du[kAlphaBatch];
        LLMI_UNROLL
        for (uint32_t j = 0; j < kAlphaBatch; ++j) {
            const uint32_t i = i0 + j * threads;
            todo[j] = AlphaTodo{};
            pre[j] = PasteUnits<AB, ES>{};
            du[j] = ComposeChunk{{0u, 0u, 0u, 0u}};
            if (i >= total) continue;
            const uint32_t row = i / upr, col = i - row * upr, y = b.y0 + row;
            const uint64_t row_addr = compose_dst_row(g, ES, k.d, k.pl, y);
            const ComposeUnits un = compose_row_units(b, ES, row_addr);
            const uint64_t u = un.first + 16 * uint64_t(col);
            if (u >= un.end) continue;
            todo[j] = alpha_decide<AB, ES>(ag, k, y, row_addr, u);
            if (todo[j].work && todo[j].whole) du[j] = mem.load16(u);
            if (alpha_prefetch(todo[j], k)) paste_load_units(todo[j].t.f, pre[j], mem);
        }
        LLMI_UNROLL
        for (uint32_t j = 0; j < kAlphaBatch; ++j) alpha_finish<AB, DT, OVER>(ag, k, todo[j], du[j], pre[j], mem);
    }
}

}  // namespace llcomp_mi
