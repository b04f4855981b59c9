// paste_rule.hpp -- the rule of the batch copy-paste for both widths of id map (include/llcomp_mi.h: "Batch copy-paste" and "Batch
// copy-paste by 16-bit ids", "Wide id maps"), stated ONCE, templated on MB, the mask's bytes per pixel (1 or 2; 3 or 4 for the wide
// id maps, whose windows have any 32-bit base and whose 3-byte pixels may straddle the shifted copies), next to ES, the element's: these
// functions are compiled into the kernel (paste_kernels.hip), into the references and the planner's checks (paste_plan.cpp) and into
// the host check that walks the kernel's own decisions without a GPU (tests/helpers/paste_check.cpp).
//
// The batches, the tiles, the 16-byte units of dst MEMORY a tile owns, the shifted copy and the merge are the composition's
// (compose_rule.hpp), by #include: a thread owns units of dst memory exactly as in k_compose, which is what keeps "written at most once"
// true although WHICH elements are written now depends on device data.  What is the paste's own: the record with its id set, the mask
// bytes of a unit's pixel span (paste_fetch_of, paste_selected) and the walk of the short list from the back (paste_finish), where an
// element falls through a piece that covers it without selecting it.
// What is a width's own: the record (MB 2 adds the base of its window of 256 ids), the id test (MB 2: one subtract, one compare, one
// bit test), the mask row's address, and how many aligned units of mask memory a fetch takes (paste_fetch_bytes): one or two for MB 1;
// for MB 2 a unit's npx pixels have 2 * npx mask bytes, up to 32 for 1-byte CHW elements, so one to three.  A 2-byte mask is aligned to
// 2 bytes, so a pixel never straddles a unit.
// Mem: batch_chunk.hpp's (load_el<MB> of a mask pixel, load_el<ES> / store_el<ES> of an element).
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "compose_rule.hpp"

namespace llcomp_mi {

constexpr uint32_t kPasteMaxPieces = 1u << 20;      // of a call
constexpr uint32_t kPasteMaxPiecesPerSample = 256;  // with w and h above 0 on one dst sample: the workgroup's list in LDS

// the mask's bytes per pixel of a call's piece type
template <class P> inline constexpr uint32_t kPasteMaskBytesOf = 0;
template <> inline constexpr uint32_t kPasteMaskBytesOf<llcomp_mi_paste_piece> = 1;
template <> inline constexpr uint32_t kPasteMaskBytesOf<llcomp_mi_paste_piece16> = 2;
// The wide call's piece, llcomp_mi_paste_piece32, serves maps of 3 and of 4 bytes per pixel; inside, the two are two types of the same
// layout, so that everything written over the piece type knows the width at compile time (codec.hip and paste_plan.cpp cast on entry)
struct PastePiece3 : llcomp_mi_paste_piece32 {};
struct PastePiece4 : llcomp_mi_paste_piece32 {};
template <> inline constexpr uint32_t kPasteMaskBytesOf<PastePiece3> = 3;
template <> inline constexpr uint32_t kPasteMaskBytesOf<PastePiece4> = 4;
// the flag bits a width's pieces may carry: VALUE_PIXEL is the wide call's only
template <uint32_t MB> inline constexpr uint32_t kPasteFlagBits = MB >= 3 ? (LLCOMP_MI_PASTE_VALUE | LLCOMP_MI_PASTE_VALUE_PIXEL) : LLCOMP_MI_PASTE_VALUE;
// the alignment of a mask of MB bytes per pixel: a 3-byte map lies at any address
LLMI_HD constexpr uint32_t paste_mask_align(uint32_t mb) { return mb == 3 ? 1u : mb; }

// THE id test, of a record or of a piece.  MB 1: mask byte m against the 256 bits.  MB 2: id m against the window of 256 ids from
// id_base on (32-bit unsigned arithmetic: ids below the base wrap above 255)
template <uint32_t MB, class R>
LLMI_HD inline bool paste_id_set(const R& r, uint32_t m) {
    if constexpr (MB == 1) {
        return (r.ids[m >> 5] >> (m & 31u)) & 1u;
    } else {
        const uint32_t d = m - r.id_base;
        if constexpr (MB == 4)  // (a window that passes 0xFFFFFFFF selects nothing there: an id below the base must not wrap into it)
            if (m < r.id_base) return false;
        return d < 256u && ((r.ids[d >> 5] >> (d & 31u)) & 1u);
    }
}
template <class P>
LLMI_HD inline bool paste_covers(const P& p, uint32_t x, uint32_t y) { return x - p.dx < p.w && y - p.dy < p.h; }
template <class P>
LLMI_HD inline bool paste_empty(const P& p) { return !p.w || !p.h; }
// ... or one that selects nothing: checked and ignored
LLMI_HD inline bool paste_idle(const llcomp_mi_paste_piece& p) {
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) any |= p.ids[i];
    return paste_empty(p) || !any;
}
// ... which for a window is one with no id bit set below 65536
LLMI_HD inline bool paste_idle(const llcomp_mi_paste_piece16& p) {
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t lo = p.id_base + 32 * i;  // the id of the word's bit 0
        const uint32_t keep = lo > 65535u ? 0u : 65536u - lo >= 32u ? 0xFFFFFFFFu : (1u << (65536u - lo)) - 1u;
        any |= p.ids[i] & keep;
    }
    return paste_empty(p) || !any;
}
// ... and for the wide windows below 2^24 or 2^32
template <uint32_t MB>
LLMI_HD inline bool paste_idle_wide(const llcomp_mi_paste_piece32& p) {
    const uint64_t end = 1ull << (8 * MB);  // one past the top id
    uint32_t any = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint64_t lo = uint64_t(p.id_base) + 32 * i;
        const uint32_t keep = lo >= end ? 0u : end - lo >= 32u ? 0xFFFFFFFFu : (1u << uint32_t(end - lo)) - 1u;
        any |= p.ids[i] & keep;
    }
    return paste_empty(p) || !any;
}
LLMI_HD inline bool paste_idle(const PastePiece3& p) { return paste_idle_wide<3>(p); }
LLMI_HD inline bool paste_idle(const PastePiece4& p) { return paste_idle_wide<4>(p); }

// A piece as the kernel reads it: ComposeRec's eight words (columns in elements), the value in the dtype's bits, the id set -- 68 bytes;
// MB 2: and the window's base -- 72 bytes.  (The 8-bit kernel's list in LDS and its filter's copy carry no word of the other width.)
template <uint32_t MB>
struct PasteRec;
template <>
struct PasteRec<1> {
    ComposeRec r;
    uint32_t value;
    uint32_t ids[8];
};
template <>
struct PasteRec<2> {
    ComposeRec r;
    uint32_t value;
    uint32_t id_base;
    uint32_t ids[8];
};
template <>
struct PasteRec<3> : PasteRec<2> {};  // (the wide records: the 16-bit record's words, the base any 32-bit value)
template <>
struct PasteRec<4> : PasteRec<2> {};
static_assert(sizeof(PasteRec<1>) == 68 && sizeof(PasteRec<2>) == 72 && sizeof(PasteRec<3>) == 72 && sizeof(PasteRec<4>) == 72, "the table's records");
LLMI_HD inline PasteRec<1> paste_rec(const llcomp_mi_paste_piece& p, uint32_t cs, uint32_t value_bits) {
    PasteRec<1> o;
    o.r = ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags};
    o.value = value_bits;
    for (uint32_t i = 0; i < 8; ++i) o.ids[i] = p.ids[i];
    return o;
}
LLMI_HD inline PasteRec<2> paste_rec(const llcomp_mi_paste_piece16& p, uint32_t cs, uint32_t value_bits) {
    PasteRec<2> o;
    o.r = ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags};
    o.value = value_bits, o.id_base = p.id_base;
    for (uint32_t i = 0; i < 8; ++i) o.ids[i] = p.ids[i];
    return o;
}
template <class P, uint32_t MB = kPasteMaskBytesOf<P>>
LLMI_HD inline PasteRec<MB> paste_rec_wide(const P& p, uint32_t cs, uint32_t value_bits) {
    PasteRec<MB> o;
    o.r = ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags};
    o.value = value_bits, o.id_base = p.id_base;
    for (uint32_t i = 0; i < 8; ++i) o.ids[i] = p.ids[i];
    return o;
}
LLMI_HD inline PasteRec<3> paste_rec(const PastePiece3& p, uint32_t cs, uint32_t value_bits) { return paste_rec_wide(p, cs, value_bits); }
LLMI_HD inline PasteRec<4> paste_rec(const PastePiece4& p, uint32_t cs, uint32_t value_bits) { return paste_rec_wide(p, cs, value_bits); }

// One call as the kernel sees it: the composition's geometry under KEEP (there is no fill) and the mask batch, MB bytes per pixel
struct PasteGeom {
    ComposeGeom g;
    uint64_t mask, mask_bytes;
    uint32_t iw;
};
template <uint32_t MB>
LLMI_HD inline PasteGeom paste_geom(uint64_t dst, uint64_t src, uint64_t mask, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh,
                                    uint32_t c, uint32_t esize, bool chw) {
    PasteGeom pg;
    pg.g = compose_geom(dst, src, n_src, iw, ih, ow, oh, c, esize, chw, true);
    pg.mask = mask, pg.mask_bytes = MB * uint64_t(n_src) * iw * ih, pg.iw = iw;
    return pg;
}
// THE address of mask(s, y, 0)
template <uint32_t MB>
LLMI_HD inline uint64_t paste_mask_row(const PasteGeom& pg, uint32_t s, uint32_t y) { return pg.mask + MB * (uint64_t(s) * pg.g.ih + y) * pg.iw; }

// THE rule, per pixel: does piece p select (x, y) of its dst sample?
template <uint32_t MB, class P, class Mem>
LLMI_HD inline bool paste_selects(const PasteGeom& pg, const P& p, uint32_t x, uint32_t y, Mem& mem) {
    if (!paste_covers(p, x, y)) return false;
    return paste_id_set<MB>(p, mem.template load_el<MB>(paste_mask_row<MB>(pg, p.src, p.sy + (y - p.dy)) + MB * uint64_t(p.sx + (x - p.dx))));
}

// What a workgroup knows beside its geometry, the same in every thread
template <uint32_t MB>
struct PasteWork {
    const PasteRec<MB>* list;  // the pieces that matter to the tile, in order
    uint32_t n_list;
    uint32_t d, pl;  // the dst sample and the plane
};

// The mask pixels of the elements [e0, e1) of the unit's row in piece r: pixel 0 is the pixel of e0, at `at`; the unit's element p0 is
// e0 and its channel is ph0 (HWC; CHW: 0); there are npx of them.  Their bytes lie in the `units` aligned units from a on, from byte
// sh on; inside: those units lie whole in the mask batch.
struct PasteFetch {
    uint64_t at, a;
    uint32_t sh, units, inside;
    uint32_t p0, n_el, ph0, npx;
};
// The bytes from `at` on that a fetch spans.  The two widths bound them differently, and each keeps its bound, because the bound
// decides which memory is read: MB 1 takes the n_el bytes that hold the pixels of n_el elements whatever c is (a pixel has an element
// at least), MB 2 the 2 * npx bytes of the pixels themselves.
template <uint32_t MB>
LLMI_HD constexpr uint32_t paste_fetch_bytes(uint32_t n_el, uint32_t npx) { return MB == 1 ? n_el : MB * npx; }
template <uint32_t MB>
LLMI_HD inline PasteFetch paste_fetch_of(const PasteGeom& pg, const ComposeRec& r, uint32_t y, int32_t eu, uint32_t e0, uint32_t e1) {
    const uint32_t cs = pg.g.cs, se0 = r.sxe + (e0 - r.dxe), spx0 = cs == 1 ? se0 : se0 / cs;
    PasteFetch f;
    f.ph0 = se0 - spx0 * cs, f.p0 = uint32_t(int32_t(e0) - eu), f.n_el = e1 - e0;
    f.npx = cs == 1 ? f.n_el : (f.ph0 + f.n_el + cs - 1) / cs;
    f.at = paste_mask_row<MB>(pg, r.src, r.sy + (y - r.dy)) + MB * uint64_t(spx0);
    f.a = f.at & ~uint64_t(15), f.sh = uint32_t(f.at & 15u), f.units = (f.sh + paste_fetch_bytes<MB>(f.n_el, f.npx) + 15u) / 16u;
    f.inside = f.a >= pg.mask && f.a + 16u * f.units <= pg.mask + pg.mask_bytes;
    return f;
}

// What a thread does with one unit of dst memory at address u in row y, decided before anything is read: nothing where no piece of the
// list reaches the unit's elements of the row; otherwise the walk from piece `hit` down, whose mask units (f) the tile pass asks for
// ahead of the walk
struct PasteTodo {
    uint32_t work;
    uint32_t y, e_lo, e_hi;  // the unit's elements of the row
    int32_t eu;              // the row's element that the unit's first would be (compose_rule.hpp: ComposeTodo)
    int32_t hit;
    uint64_t u;
    PasteFetch f;
};
// the elements of the unit's row that r reaches: [e0, e1), false for none
LLMI_HD inline bool paste_reach(const ComposeRec& r, const PasteTodo& t, uint32_t& e0, uint32_t& e1) {
    if (t.y - r.dy >= r.h) return false;
    e0 = t.e_lo > r.dxe ? t.e_lo : r.dxe, e1 = t.e_hi < r.dxe + r.ew ? t.e_hi : r.dxe + r.ew;
    return e0 < e1;
}
template <uint32_t MB, uint32_t ES>
LLMI_HD inline PasteTodo paste_decide(const PasteGeom& pg, const PasteWork<MB>& k, uint32_t y, uint64_t row_addr, uint64_t u) {
    const uint64_t row_end = row_addr + uint64_t(pg.g.rwd) * ES;
    PasteTodo t{};
    t.y = y, t.u = u;
    t.eu = int32_t((int64_t(u) - int64_t(row_addr)) / int64_t(ES));
    t.e_lo = t.eu > 0 ? uint32_t(t.eu) : 0u;
    t.e_hi = u + 16 < row_end ? uint32_t((u + 16 - row_addr) / ES) : pg.g.rwd;
    t.hit = -1;
    for (uint32_t i = k.n_list; i-- > 0;) {
        uint32_t e0, e1;
        if (!paste_reach(k.list[i].r, t, e0, e1)) continue;
        t.work = 1, t.hit = int32_t(i);
        t.f = paste_fetch_of<MB>(pg, k.list[i].r, y, t.eu, e0, e1);
        break;
    }
    return t;
}

// The mask units of a fetch, as the tile pass asks for them ahead of the walk.  A unit's 16 / ES pixels are 16 * MB / ES mask bytes:
// one shifted copy of two units, or -- MB 2 with 1-byte elements only -- two copies of three.
template <uint32_t MB, uint32_t ES>
constexpr uint32_t kPasteCopies = (16 / ES * MB + 15) / 16;
template <uint32_t N>
struct PasteMaskUnits {
    ComposeChunk u[N];
};
template <uint32_t MB, uint32_t ES>
using PasteUnits = PasteMaskUnits<kPasteCopies<MB, ES> + 1>;
static_assert(sizeof(PasteUnits<1, 1>) == 32 && sizeof(PasteUnits<1, 4>) == 32 && sizeof(PasteUnits<2, 2>) == 32 && sizeof(PasteUnits<2, 1>) == 48,
              "a third unit only for 2-byte masks under 1-byte elements");
static_assert(sizeof(PasteUnits<3, 1>) == 64 && sizeof(PasteUnits<3, 2>) == 48 && sizeof(PasteUnits<3, 4>) == 32 && sizeof(PasteUnits<4, 1>) == 80 &&
                  sizeof(PasteUnits<4, 2>) == 48 && sizeof(PasteUnits<4, 4>) == 32,
              "the wide masks: up to 48 or 64 mask bytes of a unit's pixels, in one to four or one to five aligned units");
template <uint32_t N, class Mem>
LLMI_HD inline void paste_load_units(const PasteFetch& f, PasteMaskUnits<N>& m, Mem& mem) {  // (into units of zeros)
    m.u[0] = mem.load16(f.a);
    if (f.units > 1) m.u[1] = mem.load16(f.a + 16);
    if constexpr (N > 2)
        if (f.units > 2) m.u[2] = mem.load16(f.a + 32);
    if constexpr (N > 3)
        if (f.units > 3) m.u[3] = mem.load16(f.a + 48);
    if constexpr (N > 4)
        if (f.units > 4) m.u[4] = mem.load16(f.a + 64);
}
// MB 3: pixel j of the shifted copies is bytes 3 j .. 3 j + 2 of the array they form, and may straddle two words or two copies (j a
// constant after unrolling: the words are never indexed by a variable)
template <uint32_t COPIES>
LLMI_CHUNK_FN uint32_t paste_px3(const ComposeChunk (&mv)[COPIES], uint32_t j) {
    const uint32_t b = 3 * j, k = b >> 2, sh = 8 * (b & 3);
    uint32_t v = mv[k >> 2].w[k & 3] >> sh;
    if (sh > 8) v |= mv[(k + 1) >> 2].w[(k + 1) & 3] << (32 - sh);
    return v & 0xFFFFFFu;
}

// pixel j of the shifted copies, and its place in copies of zeros
template <uint32_t MB, uint32_t COPIES>
LLMI_CHUNK_FN uint32_t paste_px(const ComposeChunk (&mv)[COPIES], uint32_t j) {
    if constexpr (MB == 3) return paste_px3(mv, j);
    else return chunk_get<MB>(mv[j / (16 / MB)].w, j % (16 / MB));
}
template <uint32_t MB, uint32_t COPIES>
LLMI_CHUNK_FN void paste_px_put(ComposeChunk (&mv)[COPIES], uint32_t j, uint32_t bits) {
    if constexpr (MB == 3) {
        LLMI_UNROLL
        for (uint32_t q = 0; q < 3; ++q) chunk_or<1>(mv[(3 * j + q) >> 4].w, (3 * j + q) & 15u, (bits >> (8 * q)) & 0xFFu);
    } else {
        chunk_or<MB>(mv[j / (16 / MB)].w, j % (16 / MB), bits);
    }
}

// The elements of [e0, e1) of the unit that r selects, as a mask with bit p for the unit's element p: the mask pixels of their pixels
// as shifted copies of the aligned units that hold them (pre: already loaded when `have`), single pixels only where such a unit
// sticks out of the mask batch; each pixel against the id set; a pixel's bit to its elements (c of them in HWC, one in CHW).
template <uint32_t MB, uint32_t ES, class Mem>
LLMI_HD inline uint32_t paste_selected(const PasteGeom& pg, const PasteRec<MB>& r, const PasteFetch& f, bool have, const PasteUnits<MB, ES>& pre, Mem& mem) {
    constexpr uint32_t PER = 16 / ES, COPIES = kPasteCopies<MB, ES>;
    const uint32_t cs = pg.g.cs;
    ComposeChunk mv[COPIES];
    LLMI_UNROLL
    for (uint32_t q = 0; q < COPIES; ++q) mv[q] = ComposeChunk{{0u, 0u, 0u, 0u}};
    if (f.inside) {
        PasteUnits<MB, ES> m{};
        if (have) m = pre;
        else paste_load_units(f, m, mem);
        LLMI_UNROLL
        for (uint32_t q = 0; q < COPIES; ++q) mv[q] = f.sh ? compose_shift(m.u[q], m.u[q + 1], f.sh) : m.u[q];
    } else {  // at the first or the last bytes of the mask batch: the pixels that belong, one by one
        LLMI_UNROLL
        for (uint32_t j = 0; j < PER; ++j)
            if (j < f.npx) paste_px_put<MB>(mv, j, mem.template load_el<MB>(f.at + MB * uint64_t(j)));
    }
    uint32_t selpx = 0;
    LLMI_UNROLL
    for (uint32_t j = 0; j < PER; ++j) selpx |= uint32_t(paste_id_set<MB>(r, paste_px<MB>(mv, j))) << j;
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

// a VALUE piece's unit: the value in every element
template <uint32_t ES>
LLMI_HD inline ComposeChunk paste_value_unit(uint32_t bits) {
    const uint32_t w = ES == 4 ? bits : ES == 2 ? (bits & 0xFFFFu) * 0x00010001u : (bits & 0xFFu) * 0x01010101u;
    return ComposeChunk{{w, w, w, w}};
}

// a VALUE_PIXEL piece's unit (U8 HWC, the wide call): element p of the unit is channel (eu + p) mod cs of its pixel and takes that byte
// of the value; eu is negative for a unit that begins before its row
LLMI_HD inline ComposeChunk paste_value_pixel_unit(uint32_t bits, uint32_t cs, int32_t eu) {
    ComposeChunk v{{0u, 0u, 0u, 0u}};
    uint32_t ph = uint32_t((eu % int32_t(cs) + int32_t(cs)) % int32_t(cs));
    LLMI_UNROLL
    for (uint32_t p = 0; p < 16; ++p) {
        chunk_or<1>(v.w, p, (bits >> (8 * ph)) & 0xFFu);
        ph = ph + 1 == cs ? 0 : ph + 1;
    }
    return v;
}

// ... and the walk.  The list from `hit` down: every piece that reaches elements nobody has claimed yet is asked which of them it
// selects, and gives those from its own shifted copy of the unit (compose_rule.hpp) or from its value, until the unit's elements of the
// row are claimed or the list ends.  16 bytes are stored when all 16 are claimed, the claimed elements one by one otherwise, nothing
// when none is.  (pre is piece `hit`'s mask units; paste_selected reads them only where that piece's fetch lies inside.)
template <uint32_t MB, uint32_t ES, class Mem>
LLMI_HD inline void paste_finish(const PasteGeom& pg, const PasteWork<MB>& k, const PasteTodo& t, const PasteUnits<MB, ES>& pre, Mem& mem) {
    constexpr uint32_t PER = 16 / ES;
    if (!t.work) return;
    const ComposeGeom& g = pg.g;
    const uint32_t need = compose_span(uint32_t(int32_t(t.e_lo) - t.eu), uint32_t(int32_t(t.e_hi) - t.eu));
    ComposeChunk acc{{0u, 0u, 0u, 0u}};
    uint32_t claimed = 0;
    for (uint32_t i = uint32_t(t.hit) + 1; i-- > 0 && claimed != need;) {
        const PasteRec<MB>& r = k.list[i];
        uint32_t e0, e1;
        if (!paste_reach(r.r, t, e0, e1)) continue;
        const uint32_t open = compose_span(uint32_t(int32_t(e0) - t.eu), uint32_t(int32_t(e1) - t.eu)) & ~claimed;
        if (!open) continue;
        const bool first = int32_t(i) == t.hit;
        const uint32_t m = paste_selected<MB, ES>(pg, r, first ? t.f : paste_fetch_of<MB>(pg, r.r, t.y, t.eu, e0, e1), first, pre, mem) & open;
        if (!m) continue;
        ComposeChunk v{{0u, 0u, 0u, 0u}};
        if (r.r.flags & LLCOMP_MI_PASTE_VALUE) {
            v = paste_value_unit<ES>(r.value);
            if constexpr (MB >= 3 && ES == 1)
                if (r.r.flags & LLCOMP_MI_PASTE_VALUE_PIXEL) v = paste_value_pixel_unit(r.value, g.cs, t.eu);
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
        if ((claimed >> p) & 1u) mem.template store_el<ES>(t.u + uint64_t(p) * ES, chunk_get<ES>(acc.w, p));
}

// One tile's rows and units, thread `tid` of `threads`, as compose_tile_pass: a thread decides kPasteBatch units and asks for the mask
// units of all of them before it walks the first, so that its loads are in flight together.
constexpr uint32_t kPasteBatch = 2;
template <uint32_t MB, uint32_t ES, class Mem>
LLMI_HD inline void paste_tile_pass(const PasteGeom& pg, const PasteWork<MB>& k, const ComposeTileBox& b, uint32_t tid, uint32_t threads, Mem& mem) {
    const ComposeGeom& g = pg.g;
    const uint32_t upr = compose_units_per_row(g.tile_w, ES), total = (b.y1 - b.y0) * upr;
    for (uint32_t i0 = tid; i0 < total; i0 += threads * kPasteBatch) {
        PasteTodo todo[kPasteBatch];
        PasteUnits<MB, ES> pre[kPasteBatch];
        LLMI_UNROLL
        for (uint32_t j = 0; j < kPasteBatch; ++j) {
            const uint32_t i = i0 + j * threads;
            todo[j] = PasteTodo{};
            pre[j] = PasteUnits<MB, ES>{};
            if (i >= total) continue;
            const uint32_t row = i / upr, col = i - row * upr, y = b.y0 + row;
            const uint64_t row_addr = compose_dst_row(g, ES, k.d, k.pl, y);
            const ComposeUnits un = compose_row_units(b, ES, row_addr);
            const uint64_t u = un.first + 16 * uint64_t(col);
            if (u >= un.end) continue;
            todo[j] = paste_decide<MB, ES>(pg, k, y, row_addr, u);
            if (todo[j].work && todo[j].f.inside) paste_load_units(todo[j].f, pre[j], mem);
        }
        LLMI_UNROLL
        for (uint32_t j = 0; j < kPasteBatch; ++j) paste_finish<MB, ES>(pg, k, todo[j], pre[j], mem);
    }
}

}  // namespace llcomp_mi
