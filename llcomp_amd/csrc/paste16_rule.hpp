// paste16_rule.hpp -- the rule of the batch copy-paste selected by a 16-bit id map (include/llcomp_mi.h: "Batch copy-paste by 16-bit
// ids"), stated ONCE on top of paste_rule.hpp and compose_rule.hpp: these functions are compiled into the kernel (paste16_kernels.hip),
// into llcomp_mi_paste16_reference and the planner's checks (paste16_plan.cpp) and into the host check that walks the kernel's own
// decisions without a GPU (tests/helpers/paste16_check.cpp).
//
// The batches, the tiles, the 16-byte units of dst MEMORY a tile owns, the shifted copy, the merge, the reach of a piece in a unit and
// the value's unit are the 8-bit paste's and the composition's, by #include: ownership of units is exactly the composition's.  What is
// new: the record with its window of 256 ids from id_base on, the id test (one subtract, one compare, one bit test), and the mask fetch
// -- a unit's npx pixels have 2 * npx mask bytes, up to 32 for 1-byte CHW elements, so the fetch is of one, two or three aligned units
// of mask memory taken as two shifted copies (16 bytes for 2-byte elements, 8 for 4-byte ones: one copy of one or two units).  A mask
// is aligned to 2 bytes, so a pixel never straddles a unit.
// Mem: load16 / store16 of aligned 16-byte units, load_el<N> of an N-byte element (N = 2: a mask pixel), store_el of a dst element.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "paste_rule.hpp"

namespace llcomp_mi {

LLMI_HD inline bool paste16_covers(const llcomp_mi_paste_piece16& p, uint32_t x, uint32_t y) { return x - p.dx < p.w && y - p.dy < p.h; }
LLMI_HD inline bool paste16_empty(const llcomp_mi_paste_piece16& p) { return !p.w || !p.h; }
// THE id test: id m against the window of 256 ids from base on (32-bit unsigned arithmetic: ids below base wrap above 255)
LLMI_HD inline bool paste16_id_set(uint32_t base, const uint32_t* ids, uint32_t m) {
    const uint32_t d = m - base;
    return d < 256u && ((ids[d >> 5] >> (d & 31u)) & 1u);
}
// ... a piece with no id bit set below 65536 selects nothing: checked and ignored
LLMI_HD inline bool paste16_idle(const llcomp_mi_paste_piece16& p) {
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t lo = p.id_base + 32 * i;  // the id of the word's bit 0
        const uint32_t keep = lo > 65535u ? 0u : 65536u - lo >= 32u ? 0xFFFFFFFFu : (1u << (65536u - lo)) - 1u;
        any |= p.ids[i] & keep;
    }
    return paste16_empty(p) || !any;
}

// A piece as the kernel reads it: ComposeRec's eight words (columns in elements), the value's bits, the window's base, the id set.  72 bytes
struct PasteRec16 {
    ComposeRec r;
    uint32_t value;
    uint32_t id_base;
    uint32_t ids[8];
};
LLMI_HD inline PasteRec16 paste16_rec(const llcomp_mi_paste_piece16& p, uint32_t cs) {
    PasteRec16 o;
    o.r = ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags};
    o.value = p.value_bits, o.id_base = p.id_base;
    for (uint32_t i = 0; i < 8; ++i) o.ids[i] = p.ids[i];
    return o;
}

// One call as the kernel sees it: the 8-bit paste's geometry with a mask of 2 bytes per pixel (PasteGeom's mask_bytes says so)
LLMI_HD inline PasteGeom paste16_geom(uint64_t dst, uint64_t src, uint64_t mask, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh,
                                      uint32_t c, uint32_t esize, bool chw) {
    PasteGeom pg = paste_geom(dst, src, mask, n_src, iw, ih, ow, oh, c, esize, chw);
    pg.mask_bytes *= 2;
    return pg;
}
// THE address of mask16(s, y, 0)
LLMI_HD inline uint64_t paste16_mask_row(const PasteGeom& pg, uint32_t s, uint32_t y) { return pg.mask + 2 * (uint64_t(s) * pg.g.ih + y) * pg.iw; }

// THE rule, per pixel: does piece p select (x, y) of its dst sample?
template <class Mem>
LLMI_HD inline bool paste16_selects(const PasteGeom& pg, const llcomp_mi_paste_piece16& p, uint32_t x, uint32_t y, Mem& mem) {
    if (!paste16_covers(p, x, y)) return false;
    return paste16_id_set(p.id_base, p.ids, mem.template load_el<2>(paste16_mask_row(pg, p.src, p.sy + (y - p.dy)) + 2 * uint64_t(p.sx + (x - p.dx))));
}

struct PasteWork16 {
    const PasteRec16* list;  // the pieces that matter to the tile, in order
    uint32_t n_list;
    uint32_t d, pl;  // the dst sample and the plane
};

// The mask pixels of the elements [e0, e1) of the unit's row in piece r: pixel 0 is the pixel of e0, at `at`; the unit's element p0 is
// e0 and its channel is ph0 (HWC; CHW: 0).  Their 2 * npx bytes lie in the `units` (1..3) aligned units from a on, from byte sh (even)
// on; inside: those units lie whole in the mask batch.
struct PasteFetch16 {
    uint64_t at, a;
    uint32_t sh, units, inside;
    uint32_t p0, n_el, ph0, npx;
};
LLMI_HD inline PasteFetch16 paste16_fetch_of(const PasteGeom& pg, const ComposeRec& r, uint32_t y, int32_t eu, uint32_t e0, uint32_t e1) {
    const uint32_t cs = pg.g.cs, se0 = r.sxe + (e0 - r.dxe), spx0 = cs == 1 ? se0 : se0 / cs;
    PasteFetch16 f;
    f.ph0 = se0 - spx0 * cs, f.p0 = uint32_t(int32_t(e0) - eu), f.n_el = e1 - e0;
    f.npx = cs == 1 ? f.n_el : (f.ph0 + f.n_el + cs - 1) / cs;
    f.at = paste16_mask_row(pg, r.src, r.sy + (y - r.dy)) + 2 * uint64_t(spx0);
    f.a = f.at & ~uint64_t(15), f.sh = uint32_t(f.at & 15u), f.units = (f.sh + 2 * f.npx + 15u) / 16u;
    f.inside = f.a >= pg.mask && f.a + 16u * f.units <= pg.mask + pg.mask_bytes;
    return f;
}

struct PasteTodo16 {
    uint32_t work;
    uint32_t y, e_lo, e_hi;  // the unit's elements of the row
    int32_t eu;              // the row's element that the unit's first would be (compose_rule.hpp: ComposeTodo)
    int32_t hit;
    uint64_t u;
    PasteFetch16 f;
};
// the elements of the unit's row that r reaches: [e0, e1), false for none
LLMI_HD inline bool paste16_reach(const ComposeRec& r, const PasteTodo16& t, uint32_t& e0, uint32_t& e1) {
    if (t.y - r.dy >= r.h) return false;
    e0 = t.e_lo > r.dxe ? t.e_lo : r.dxe, e1 = t.e_hi < r.dxe + r.ew ? t.e_hi : r.dxe + r.ew;
    return e0 < e1;
}
template <uint32_t ES>
LLMI_HD inline PasteTodo16 paste16_decide(const PasteGeom& pg, const PasteWork16& k, uint32_t y, uint64_t row_addr, uint64_t u) {
    const uint64_t row_end = row_addr + uint64_t(pg.g.rwd) * ES;
    PasteTodo16 t{};
    t.y = y, t.u = u;
    t.eu = int32_t((int64_t(u) - int64_t(row_addr)) / int64_t(ES));
    t.e_lo = t.eu > 0 ? uint32_t(t.eu) : 0u;
    t.e_hi = u + 16 < row_end ? uint32_t((u + 16 - row_addr) / ES) : pg.g.rwd;
    t.hit = -1;
    for (uint32_t i = k.n_list; i-- > 0;) {
        uint32_t e0, e1;
        if (!paste16_reach(k.list[i].r, t, e0, e1)) continue;
        t.work = 1, t.hit = int32_t(i);
        t.f = paste16_fetch_of(pg, k.list[i].r, y, t.eu, e0, e1);
        break;
    }
    return t;
}

// the mask units of a fetch, as the tile pass asks for them ahead of the walk
struct PasteMaskUnits {
    ComposeChunk u[3];
};
template <uint32_t ES, class Mem>
LLMI_HD inline void paste16_load_units(const PasteFetch16& f, PasteMaskUnits& m, Mem& mem) {
    m.u[0] = mem.load16(f.a);
    if (f.units > 1) m.u[1] = mem.load16(f.a + 16);
    if constexpr (ES == 1)
        if (f.units > 2) m.u[2] = mem.load16(f.a + 32);
}

// The elements of [e0, e1) of the unit that r selects, as a mask with bit p for the unit's element p: the mask pixels of their pixels
// as shifted copies of the aligned units that hold them (pre: already loaded when `have`), single pixels only where such a unit
// sticks out of the mask batch; each pixel against the window; a pixel's bit to its elements (c of them in HWC, one in CHW).
template <uint32_t ES, class Mem>
LLMI_HD inline uint32_t paste16_selected(const PasteGeom& pg, const PasteRec16& r, const PasteFetch16& f, bool have, const PasteMaskUnits& pre, Mem& mem) {
    constexpr uint32_t PER = 16 / ES;
    const uint32_t cs = pg.g.cs;
    ComposeChunk mv0{{0u, 0u, 0u, 0u}}, mv1{{0u, 0u, 0u, 0u}};  // pixels 0..7 and, for 1-byte elements, 8..15
    if (f.inside) {
        PasteMaskUnits m{{{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}}};
        if (have) m = pre;
        else paste16_load_units<ES>(f, m, mem);
        mv0 = f.sh ? compose_shift(m.u[0], m.u[1], f.sh) : m.u[0];
        if constexpr (ES == 1) mv1 = f.sh ? compose_shift(m.u[1], m.u[2], f.sh) : m.u[1];
    } else {  // at the first or the last bytes of the mask batch: the pixels that belong, one by one
        LLMI_UNROLL
        for (uint32_t j = 0; j < PER; ++j)
            if (j < f.npx) {
                const uint32_t v = mem.template load_el<2>(f.at + 2 * uint64_t(j));
                if (j < 8) chunk_or<2>(mv0.w, j, v);
                else chunk_or<2>(mv1.w, j - 8, v);
            }
    }
    uint32_t selpx = 0;
    LLMI_UNROLL
    for (uint32_t j = 0; j < PER; ++j) selpx |= uint32_t(paste16_id_set(r.id_base, r.ids, j < 8 ? chunk_get<2>(mv0.w, j) : chunk_get<2>(mv1.w, j - 8))) << j;
    const uint32_t span = compose_span(f.p0, f.p0 + f.n_el);
    if (cs == 1) return (selpx << f.p0) & span;
    uint32_t em = 0, j = 0, ph = f.ph0;
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p) {
        if (!((span >> p) & 1u)) continue;
        em |= ((selpx >> j) & 1u) << p;
        if (++ph == cs) ph = 0, ++j;
    }
    return em;
}

// ... and the walk, as paste_finish: the list from `hit` down, every piece that reaches elements nobody has claimed yet is asked which
// of them it selects, and gives those from its own shifted copy of the unit or from its value, until the unit's elements of the row
// are claimed or the list ends.  16 bytes are stored when all 16 are claimed, the claimed elements one by one otherwise, nothing when
// none is.
template <uint32_t ES, class Mem>
LLMI_HD inline void paste16_finish(const PasteGeom& pg, const PasteWork16& k, const PasteTodo16& t, const PasteMaskUnits& pre, Mem& mem) {
    constexpr uint32_t PER = 16 / ES;
    if (!t.work) return;
    const ComposeGeom& g = pg.g;
    const uint32_t need = compose_span(uint32_t(int32_t(t.e_lo) - t.eu), uint32_t(int32_t(t.e_hi) - t.eu));
    ComposeChunk acc{{0u, 0u, 0u, 0u}};
    uint32_t claimed = 0;
    for (uint32_t i = uint32_t(t.hit) + 1; i-- > 0 && claimed != need;) {
        const PasteRec16& r = k.list[i];
        uint32_t e0, e1;
        if (!paste16_reach(r.r, t, e0, e1)) continue;
        const uint32_t open = compose_span(uint32_t(int32_t(e0) - t.eu), uint32_t(int32_t(e1) - t.eu)) & ~claimed;
        if (!open) continue;
        const bool first = int32_t(i) == t.hit;
        const uint32_t m = paste16_selected<ES>(pg, r, first ? t.f : paste16_fetch_of(pg, r.r, t.y, t.eu, e0, e1), first && t.f.inside, pre, mem) & open;
        if (!m) continue;
        ComposeChunk v{{0u, 0u, 0u, 0u}};
        if (r.r.flags & LLCOMP_MI_PASTE_VALUE) {
            v = paste_value_unit<ES>(r.value);
        } else {
            const uint64_t s = compose_src_of_unit(g, ES, r.r, k.pl, t.y, t.eu);
            if (compose_src_units_inside(g, s)) {
                const ComposeChunk a = mem.load16(s & ~uint64_t(15));
                v = (s & 15u) ? compose_shift(a, mem.load16((s & ~uint64_t(15)) + 16), uint32_t(s & 15u)) : a;
            } else {  // at the first or the last bytes of the src batch: the elements that belong, one by one
                LLMI_UNROLL
                for (uint32_t p = 0; p < PER; ++p)
                    if ((m >> p) & 1u) chunk_or<ES>(v.w, p, mem.template load_el<ES>(s + uint64_t(p) * ES));
            }
        }
        acc = compose_merge<ES>(acc, v, m);
        claimed |= m;
    }
    if (!claimed) return;
    if (claimed == (1u << PER) - 1u) return mem.store16(t.u, acc);
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p)
        if ((claimed >> p) & 1u) mem.store_el(t.u + uint64_t(p) * ES, chunk_get<ES>(acc.w, p));
}

// One tile's rows and units, thread `tid` of `threads`, as paste_tile_pass: a thread decides kPasteBatch units and asks for the mask
// units of all of them before it walks the first, so that its loads are in flight together.
template <uint32_t ES, class Mem>
LLMI_HD inline void paste16_tile_pass(const PasteGeom& pg, const PasteWork16& k, const ComposeTileBox& b, uint32_t tid, uint32_t threads, Mem& mem) {
    const ComposeGeom& g = pg.g;
    const uint32_t upr = compose_units_per_row(g.tile_w, ES), total = (b.y1 - b.y0) * upr;
    for (uint32_t i0 = tid; i0 < total; i0 += threads * kPasteBatch) {
        PasteTodo16 todo[kPasteBatch];
        PasteMaskUnits pre[kPasteBatch];
        LLMI_UNROLL
        for (uint32_t j = 0; j < kPasteBatch; ++j) {
            const uint32_t i = i0 + j * threads;
            todo[j] = PasteTodo16{};
            pre[j] = PasteMaskUnits{{{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}}};
            if (i >= total) continue;
            const uint32_t row = i / upr, col = i - row * upr, y = b.y0 + row;
            const uint64_t row_addr = compose_dst_row(g, ES, k.d, k.pl, y);
            const ComposeUnits un = compose_row_units(b, ES, row_addr);
            const uint64_t u = un.first + 16 * uint64_t(col);
            if (u >= un.end) continue;
            todo[j] = paste16_decide<ES>(pg, k, y, row_addr, u);
            if (todo[j].work && todo[j].f.inside) paste16_load_units<ES>(todo[j].f, pre[j], mem);
        }
        LLMI_UNROLL
        for (uint32_t j = 0; j < kPasteBatch; ++j) paste16_finish<ES>(pg, k, todo[j], pre[j], mem);
    }
}

}  // namespace llcomp_mi
