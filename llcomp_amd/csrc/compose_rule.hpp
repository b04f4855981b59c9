// compose_rule.hpp -- the rule of the batch composition (include/llcomp_mi.h: "Batch composition"), stated ONCE: these functions are
// compiled into the kernel (compose_kernels.hip), into llcomp_mi_compose_reference and the planner's checks (compose_plan.cpp) and into
// the host check that walks the kernel's own decisions without a GPU (tests/helpers/compose_plan_check.cpp).
//
// Both batches are seen as planes of rows of ELEMENTS: CHW has c planes per sample and rows of ow elements, HWC one plane and rows of
// ow * c elements, so a piece's columns are scaled by cs = 1 or c (ComposeRec) and nothing below knows a pixel.  A workgroup owns a tile
// of one plane of one dst sample, compose_tile_rows rows by kComposeTile pixels, and takes the tile's rows in the 16-byte units of dst
// MEMORY they lie in: a unit that straddles the border of two tiles of a row belongs to the tile that holds the unit's first element
// of the row, whole, so every (row, unit) has one owner and one thread (compose_row_units, compose_decide, compose_finish).
// The element's size and the shape of a batch: batch_ops.hpp (through mix_rule.hpp); an element's place in a unit: batch_chunk.hpp.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "batch_chunk.hpp"
#include "mix_rule.hpp"

namespace llcomp_mi {

constexpr uint32_t kComposeTile = 128;                // pixels across a tile (llcomp_mi_compose_tile)
constexpr uint32_t kComposeMaxPieces = 1u << 20;      // of a call
constexpr uint32_t kComposeMaxPiecesPerSample = 1024; // with w and h above 0 on one dst sample (llcomp_mi_compose_max_pieces_per_sample)
constexpr uint32_t kComposeListCap = 256;             // pieces of a workgroup's short list in LDS; a sample with more resolves against its whole run
constexpr uint32_t kComposePatterns = 32;             // fill patterns a workgroup builds: one per phase of a pixel's elements against a unit

// The rows of a tile by the bytes of a pixel as the kernel sees one (CHW: the element; HWC: c elements): the power of two, at most 64,
// that keeps a tile within 16 KiB of dst memory
LLMI_HD constexpr uint32_t compose_tile_rows(uint32_t pixel_bytes) {
    uint32_t r = 64;
    while (r > 1 && uint64_t(kComposeTile) * r * pixel_bytes > 16384u) r /= 2;
    return r;
}

// (x, y) of a dst sample lies in the piece's rectangle
LLMI_HD inline bool compose_covers(const llcomp_mi_compose_piece& p, uint32_t x, uint32_t y) { return x - p.dx < p.w && y - p.dy < p.h; }
LLMI_HD inline bool compose_empty(const llcomp_mi_compose_piece& p) { return !p.w || !p.h; }

// A piece as the kernel reads it: columns in elements (dx * cs ...), 32 bytes
struct ComposeRec {
    uint32_t src, dxe, dy, sxe, sy, ew, h, flags;
};
LLMI_HD inline ComposeRec compose_rec(const llcomp_mi_compose_piece& p, uint32_t cs) {
    return ComposeRec{p.src, p.dx * cs, p.dy, p.sx * cs, p.sy, p.w * cs, p.h, p.flags};
}

// One call as the kernel sees it.  Addresses are integers, so the host check can state them for batches at any byte offset.
struct ComposeGeom {
    uint64_t dst, src, src_bytes;  // the batches' first bytes; the src batch's size (0 without one)
    uint32_t rwd, rws;             // elements of a row of dst / src: ow * cs, iw * cs
    uint32_t oh, ih;
    uint32_t planes, cs;           // CHW: c, 1; HWC: 1, c
    uint32_t keep;
    uint32_t tile_w, tile_rows;    // of a tile, in elements (kComposeTile * cs) and rows
    uint32_t tiles_x, tiles_y;
};
LLMI_HD inline ComposeGeom compose_geom(uint64_t dst, uint64_t src, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh, uint32_t c,
                                        uint32_t esize, bool chw, bool keep) {
    ComposeGeom g{};
    g.dst = dst, g.src = src, g.src_bytes = uint64_t(n_src) * c * iw * ih * esize;
    g.planes = chw ? c : 1u, g.cs = chw ? 1u : c;
    g.rwd = ow * g.cs, g.rws = iw * g.cs, g.oh = oh, g.ih = ih, g.keep = keep ? 1u : 0u;
    g.tile_w = kComposeTile * g.cs, g.tile_rows = compose_tile_rows(g.cs * esize);
    g.tiles_x = (ow + kComposeTile - 1) / kComposeTile, g.tiles_y = (oh + g.tile_rows - 1) / g.tile_rows;
    return g;
}
// THE address functions: row y of plane pl of a sample, in either batch
LLMI_HD inline uint64_t compose_dst_row(const ComposeGeom& g, uint32_t es, uint32_t d, uint32_t pl, uint32_t y) {
    return g.dst + ((uint64_t(d) * g.planes + pl) * g.oh + y) * g.rwd * es;
}
LLMI_HD inline uint64_t compose_src_row(const ComposeGeom& g, uint32_t es, uint32_t s, uint32_t pl, uint32_t y) {
    return g.src + ((uint64_t(s) * g.planes + pl) * g.ih + y) * g.rws * es;
}

// A tile: elements [x0, x1) of rows [y0, y1); and the columns its units can reach, up to a unit less an element past x1
struct ComposeTileBox {
    uint32_t x0, x1, y0, y1, reach;
};
LLMI_HD inline ComposeTileBox compose_tile_box(const ComposeGeom& g, uint32_t es, uint32_t tile) {
    const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    ComposeTileBox b;
    b.x0 = tx * g.tile_w, b.x1 = g.rwd - b.x0 < g.tile_w ? g.rwd : b.x0 + g.tile_w;
    b.y0 = ty * g.tile_rows, b.y1 = g.oh - b.y0 < g.tile_rows ? g.oh : b.y0 + g.tile_rows;
    const uint32_t over = 16 / es - 1;
    b.reach = g.rwd - b.x1 < over ? g.rwd : b.x1 + over;
    return b;
}
// does the piece matter to the tile?  (the filter of the workgroup's short list)
LLMI_HD inline bool compose_hits(const ComposeRec& r, const ComposeTileBox& b) {
    return r.dxe < b.reach && r.dxe + r.ew > b.x0 && r.dy < b.y1 && r.dy + r.h > b.y0;
}

// one piece, and it covers everything the tile's units can reach
LLMI_HD inline bool compose_solo(const ComposeRec* list, uint32_t n, const ComposeTileBox& b) {
    return n == 1 && list[0].dxe <= b.x0 && list[0].dxe + list[0].ew >= b.reach && list[0].dy <= b.y0 && list[0].dy + list[0].h >= b.y1;
}

// The units of row `row_addr` that the tile owns: addresses first, first + 16, ... below end.  A unit belongs to the tile that holds
// the first of the unit's elements of the row.
struct ComposeUnits {
    uint64_t first, end;
};
LLMI_HD inline ComposeUnits compose_row_units(const ComposeTileBox& b, uint32_t es, uint64_t row_addr) {
    const uint64_t lo = row_addr + uint64_t(b.x0) * es;
    return ComposeUnits{b.x0 ? (lo + 15) & ~uint64_t(15) : lo & ~uint64_t(15), row_addr + uint64_t(b.x1) * es};
}
// the most units of a row to a tile
LLMI_HD constexpr uint32_t compose_units_per_row(uint32_t tile_w, uint32_t es) { return (tile_w * es + 15) / 16 + 1; }

// The last piece of the list that covers an element of [e_lo, e_hi) in row y, -1 for none; whole: it covers all of them (or none does)
LLMI_HD inline int32_t compose_resolve(const ComposeRec* list, uint32_t n, uint32_t e_lo, uint32_t e_hi, uint32_t y, bool& whole) {
    for (uint32_t i = n; i-- > 0;) {
        const ComposeRec& r = list[i];
        if (y - r.dy >= r.h) continue;
        const uint32_t lo = e_lo > r.dxe ? e_lo : r.dxe, hi = e_hi < r.dxe + r.ew ? e_hi : r.dxe + r.ew;
        if (lo >= hi) continue;
        whole = lo == e_lo && hi == e_hi;
        return int32_t(i);
    }
    whole = true;
    return -1;
}

// (ComposeChunk, 16 bytes for the host check as for the kernel, and an element's word and shift in its w: batch_chunk.hpp)
LLMI_HD inline uint32_t compose_alignbyte(uint32_t hi, uint32_t lo, uint32_t r) {  // bytes r .. r + 3 of hi:lo
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return r ? (lo >> (8 * r)) | (hi << (32 - 8 * r)) : lo;
#endif
}
// THE shifted copy: bytes sh .. sh + 15 of the 32 bytes hi:lo, two aligned units of src memory (sh = 0: hi is not read).  A dword
// select for the multiple of 4 in the shift, a byte funnel shift for the rest.
LLMI_HD inline ComposeChunk compose_shift(const ComposeChunk& lo, const ComposeChunk& hi, uint32_t sh) {
    uint32_t w[8] = {lo.w[0], lo.w[1], lo.w[2], lo.w[3], hi.w[0], hi.w[1], hi.w[2], hi.w[3]};
    if (sh & 8) w[0] = w[2], w[1] = w[3], w[2] = w[4], w[3] = w[5], w[4] = w[6], w[5] = w[7];
    if (sh & 4) w[0] = w[1], w[1] = w[2], w[2] = w[3], w[3] = w[4], w[4] = w[5];
    const uint32_t r = sh & 3;
    return ComposeChunk{{compose_alignbyte(w[1], w[0], r), compose_alignbyte(w[2], w[1], r), compose_alignbyte(w[3], w[2], r),
                         compose_alignbyte(w[4], w[3], r)}};
}
// The fill pattern of phase ph: the unit's element e is of channel (ph + e) % cmod.  fill: the channels' values in the dtype, from the
// plane's own on in CHW (cmod 1)
template <uint32_t ES>
LLMI_HD inline ComposeChunk compose_pattern(const uint32_t* fill, uint32_t cmod, uint32_t ph) {
    ComposeChunk v{{0u, 0u, 0u, 0u}};
    for (uint32_t e = 0; e < 16 / ES; ++e) {
        chunk_or<ES>(v.w, e, fill[ph]);
        if (++ph >= cmod) ph = 0;
    }
    return v;
}

// What a workgroup knows beside its geometry, the same in every thread
struct ComposeWork {
    const ComposeRec* list;  // the pieces that matter to the tile, in order
    uint32_t n_list;
    const uint32_t* fill;          // the channels' fill values in the dtype; CHW: the plane's own first
    uint32_t cmod;                 // CHW 1, HWC cs
    const ComposeChunk* patterns;  // min(cmod, kComposePatterns) of them when cmod <= kComposePatterns, else none
    uint32_t d, pl;                // the dst sample and the plane
    bool solo;                     // the list is ONE piece that covers every unit of the tile: nothing to resolve (compose_solo)
};

// The elements [a, b) of a unit as a mask, bit p for element p; and the elements of v that the mask names put into acc
LLMI_HD inline uint32_t compose_span(uint32_t a, uint32_t b) { return ((1u << b) - 1u) & ~((1u << a) - 1u); }
template <uint32_t ES>
LLMI_HD inline ComposeChunk compose_merge(const ComposeChunk& acc, const ComposeChunk& v, uint32_t m) {
    ComposeChunk o;
    LLMI_UNROLL
    for (uint32_t d = 0; d < 4; ++d) {
        uint32_t bytes;
        if constexpr (ES == 4) {
            bytes = (m >> d) & 1u ? 0xFFFFFFFFu : 0u;
        } else if constexpr (ES == 2) {
            bytes = ((m >> (2 * d)) & 1u ? 0x0000FFFFu : 0u) | ((m >> (2 * d + 1)) & 1u ? 0xFFFF0000u : 0u);
        } else {
            const uint32_t b = m >> (4 * d);
            bytes = (b & 1u ? 0x000000FFu : 0u) | (b & 2u ? 0x0000FF00u : 0u) | (b & 4u ? 0x00FF0000u : 0u) | (b & 8u ? 0xFF000000u : 0u);
        }
        o.w[d] = (acc.w[d] & ~bytes) | (v.w[d] & bytes);
    }
    return o;
}
// the fill pattern of a unit whose element 0 is the row's element eu (below 0: in front of the row)
template <uint32_t ES>
LLMI_HD inline ComposeChunk compose_fill_unit(const ComposeWork& k, int32_t eu) {
    const int32_t cm = int32_t(k.cmod);
    const uint32_t ph = cm > 1 ? uint32_t(((eu % cm) + cm) % cm) : 0u;
    return k.cmod <= kComposePatterns ? k.patterns[ph] : compose_pattern<ES>(k.fill, k.cmod, ph);
}

// What a thread does with one unit of dst memory at address u in row y (row_addr), decided before anything is read
enum : uint32_t { kComposeNothing = 0, kComposePattern = 1, kComposeCopy = 2, kComposeMixed = 3 };
struct ComposeTodo {
    uint32_t kind;
    uint32_t y, e_lo, e_hi;  // the unit's elements of the row
    int32_t eu;              // the row's element that the unit's first would be: e_lo, or below 0 where the row begins inside the unit
    uint32_t sh;             // kComposeCopy: the source run begins sh bytes into the aligned unit at s_lo
    uint64_t s_lo, u;
};
// the address that the unit's first byte is read from in piece r -- for the elements of the unit that r covers; the others' bytes there
// belong to the neighbours in memory
LLMI_HD inline uint64_t compose_src_of_unit(const ComposeGeom& g, uint32_t es, const ComposeRec& r, uint32_t pl, uint32_t y, int32_t eu) {
    return compose_src_row(g, es, r.src, pl, r.sy + (y - r.dy)) + uint64_t((int64_t(r.sxe) + eu - int64_t(r.dxe)) * int64_t(es));
}
// are the one or two aligned units that hold the 16 bytes from s on whole inside the src batch?
LLMI_HD inline bool compose_src_units_inside(const ComposeGeom& g, uint64_t s) {
    const uint64_t s_lo = s & ~uint64_t(15);
    return s_lo >= g.src && s_lo + ((s & 15u) ? 32u : 16u) <= g.src + g.src_bytes;
}
template <uint32_t ES>
LLMI_HD inline ComposeTodo compose_decide(const ComposeGeom& g, const ComposeWork& k, uint32_t y, uint64_t row_addr, uint64_t u) {
    constexpr uint32_t PER = 16 / ES;
    const uint64_t row_end = row_addr + uint64_t(g.rwd) * ES;
    ComposeTodo t{};
    t.y = y, t.u = u;
    t.eu = int32_t((int64_t(u) - int64_t(row_addr)) / int64_t(ES));
    t.e_lo = t.eu > 0 ? uint32_t(t.eu) : 0u;
    t.e_hi = u + 16 < row_end ? uint32_t((u + 16 - row_addr) / ES) : g.rwd;
    bool whole = true;
    const int32_t hit = k.solo ? 0 : compose_resolve(k.list, k.n_list, t.e_lo, t.e_hi, y, whole);
    t.kind = kComposeMixed;
    if (whole) {
        if (hit < 0 && g.keep) return t.kind = kComposeNothing, t;
        if (t.e_hi - t.e_lo == PER) {
            if (hit < 0 || (k.list[hit].flags & LLCOMP_MI_COMPOSE_FILL)) return t.kind = kComposePattern, t;
            const uint64_t s = compose_src_of_unit(g, ES, k.list[hit], k.pl, y, t.eu);
            t.s_lo = s & ~uint64_t(15), t.sh = uint32_t(s & 15u);
            if (compose_src_units_inside(g, s)) t.kind = kComposeCopy;
        }
    }
    return t;
}
// ... and what is left of it once the source units of a kComposeCopy are there: every element of the row in the unit is written once,
// or left under KEEP.  Mem: load16 / store16 of aligned units, load_el / store_el of single elements; nothing else touches memory.
template <uint32_t ES, class Mem>
LLMI_HD inline void compose_finish(const ComposeGeom& g, const ComposeWork& k, const ComposeTodo& t, const ComposeChunk& lo, const ComposeChunk& hi,
                                   Mem& mem) {
    constexpr uint32_t PER = 16 / ES;
    if (t.kind == kComposeNothing) return;
    if (t.kind == kComposeCopy) return mem.store16(t.u, t.sh ? compose_shift(lo, hi, t.sh) : lo);
    if (t.kind == kComposePattern) return mem.store16(t.u, compose_fill_unit<ES>(k, t.eu));
    // A piece's border inside the unit, a unit the row covers in part, a source unit that sticks out of its batch.  The list from the
    // back: every piece that covers elements nobody has claimed yet gives them, from its own shifted copy of the unit -- the copy's
    // other bytes are its neighbours' in memory and are dropped -- until the unit's elements of the row are claimed.
    const uint32_t need = compose_span(uint32_t(int32_t(t.e_lo) - t.eu), uint32_t(int32_t(t.e_hi) - t.eu));
    ComposeChunk acc{{0u, 0u, 0u, 0u}};
    uint32_t claimed = 0;
    for (uint32_t i = k.n_list; i-- > 0 && claimed != need;) {
        const ComposeRec& r = k.list[i];
        if (t.y - r.dy >= r.h) continue;
        const uint32_t e0 = t.e_lo > r.dxe ? t.e_lo : r.dxe, e1 = t.e_hi < r.dxe + r.ew ? t.e_hi : r.dxe + r.ew;
        if (e0 >= e1) continue;
        const uint32_t m = compose_span(uint32_t(int32_t(e0) - t.eu), uint32_t(int32_t(e1) - t.eu)) & ~claimed;
        if (!m) continue;
        ComposeChunk v{{0u, 0u, 0u, 0u}};
        if (r.flags & LLCOMP_MI_COMPOSE_FILL) {
            v = compose_fill_unit<ES>(k, t.eu);
        } else {
            const uint64_t s = compose_src_of_unit(g, ES, r, k.pl, t.y, t.eu);
            if (compose_src_units_inside(g, s)) {
                const ComposeChunk a = mem.load16(s & ~uint64_t(15));
                v = (s & 15u) ? compose_shift(a, mem.load16((s & ~uint64_t(15)) + 16), uint32_t(s & 15u)) : a;
            } else {  // at the first or the last bytes of the src batch: the elements that belong, one by one
                LLMI_UNROLL
                for (uint32_t p = 0; p < PER; ++p)
                    if ((m >> p) & 1u) chunk_or<ES>(v.w, p, mem.load_el(s + uint64_t(p) * ES));
            }
        }
        acc = compose_merge<ES>(acc, v, m);
        claimed |= m;
    }
    if (claimed != need && !g.keep) {
        acc = compose_merge<ES>(acc, compose_fill_unit<ES>(k, t.eu), need & ~claimed);
        claimed = need;
    }
    if (claimed == (1u << PER) - 1u) return mem.store16(t.u, acc);
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p)
        if ((claimed >> p) & 1u) mem.store_el(t.u + uint64_t(p) * ES, chunk_get<ES>(acc.w, p));
}

// One tile's rows and units, thread `tid` of `threads`: what the kernel's threads do behind the filter's barrier.  A thread decides
// kComposeBatch units and asks for all their source units before it stores the first, so that its loads are in flight together.
constexpr uint32_t kComposeBatch = 2;  // (1, 2 and 4 were measured: DESIGN.md "Batch composition")
template <uint32_t ES, class Mem>
LLMI_HD inline void compose_tile_pass(const ComposeGeom& g, const ComposeWork& k, const ComposeTileBox& b, uint32_t tid, uint32_t threads, Mem& mem) {
    const uint32_t upr = compose_units_per_row(g.tile_w, ES), total = (b.y1 - b.y0) * upr;
    for (uint32_t i0 = tid; i0 < total; i0 += threads * kComposeBatch) {
        ComposeTodo todo[kComposeBatch];
        ComposeChunk lo[kComposeBatch], hi[kComposeBatch];
        LLMI_UNROLL
        for (uint32_t j = 0; j < kComposeBatch; ++j) {
            const uint32_t i = i0 + j * threads;
            todo[j].kind = kComposeNothing;
            lo[j] = hi[j] = ComposeChunk{{0u, 0u, 0u, 0u}};
            if (i >= total) continue;
            const uint32_t row = i / upr, col = i - row * upr, y = b.y0 + row;
            const uint64_t row_addr = compose_dst_row(g, ES, k.d, k.pl, y);
            const ComposeUnits un = compose_row_units(b, ES, row_addr);
            const uint64_t u = un.first + 16 * uint64_t(col);
            if (u >= un.end) continue;
            todo[j] = compose_decide<ES>(g, k, y, row_addr, u);
            if (todo[j].kind == kComposeCopy) {
                lo[j] = mem.load16(todo[j].s_lo);
                if (todo[j].sh) hi[j] = mem.load16(todo[j].s_lo + 16);
            }
        }
        LLMI_UNROLL
        for (uint32_t j = 0; j < kComposeBatch; ++j) compose_finish<ES>(g, k, todo[j], lo[j], hi[j], mem);
    }
}

}  // namespace llcomp_mi
