// label_boxes_rule.hpp -- the rule of the label boxes of both calls (include/llcomp_mi.h: "Label boxes", "Label boxes of listed ids"),
// stated ONCE, templated on MB, the map's bytes per pixel (1 or 2; 3 or 4 for the wide id maps): the record's identity, the update of a record by a run of equal
// ids, and what a thread does with one 16-byte unit of map memory (label_boxes_unit).  Compiled into the kernels
// (label_boxes_kernels.hip), into llcomp_mi_label_boxes_reference and llcomp_mi_label_boxes16_reference (label_boxes.cpp), which walk
// the kernels' own bands, threads and units on the host, and into the stand-alone host check.  The lists of the listed call:
// label_lists.hpp.
//
// A sample's rows are dense, so a band of kLabelBoxRows rows is one byte range; a workgroup takes it in the aligned 16-byte units of
// MEMORY it lies in, 16 / MB pixels each, of which a thread uses the pixels that belong to the band -- the others are the neighbouring
// band's or sample's.  A 2-byte map is aligned to 2 bytes and a 4-byte map to 4, so a band's bounds are multiples of MB and a pixel
// never straddles a unit.  A 3-byte map lies at any address: a pixel BELONGS to the unit that holds its first byte, whose thread reads
// the pixel's last bytes, at most two, from the next unit (batch_chunk.hpp: chunk_pixels3, chunk_read3) -- five or six pixels to a
// unit, each pixel of a band in exactly one.
// Mem: batch_chunk.hpp's (load16 of an aligned unit, load_el<MB> of a pixel).  Sink: run(id, x_first, x_end, y, length), in any order.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "batch_chunk.hpp"
#include "batch_ops.hpp"

namespace llcomp_mi {

constexpr uint32_t kLabelIds = 256;      // records of a sample of the dense call
constexpr uint32_t kLabelBoxRows = 32;   // rows of a workgroup's band (llcomp_mi_label_boxes_rows)
constexpr uint32_t kLabelThreads = 256;  // of a workgroup

// the record of an id without a pixel: the identities of min and max
LLMI_HD inline llcomp_mi_label_box label_box_identity(uint32_t ow, uint32_t oh) { return llcomp_mi_label_box{0u, ow, oh, 0u, 0u}; }
// THE run update: `length` pixels of the id in columns [x_first, x_end) of row y
LLMI_HD inline void label_box_update(llcomp_mi_label_box& b, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
    b.count += length;
    b.x0 = x_first < b.x0 ? x_first : b.x0, b.x1 = x_end > b.x1 ? x_end : b.x1;
    b.y0 = y < b.y0 ? y : b.y0, b.y1 = y + 1 > b.y1 ? y + 1 : b.y1;
}

// A whole call of the dense kind but for its pointers
LLMI_HD inline int label_boxes_check_call(uint32_t n, uint32_t ow, uint32_t oh) {
    if (int rc = batch_check_shape(n, 1, ow, oh, LLCOMP_MI_DTYPE_U8, LLCOMP_MI_LAYOUT_HWC)) return rc;
    return uint64_t(ow) * oh >= (1ull << 32) ? LLCOMP_MI_BAD_ARGS : LLCOMP_MI_OK;
}

struct LabelGeom {
    uint64_t maps, bytes;  // the batch's first byte and its size
    uint32_t ow, oh, bands;
};
template <uint32_t MB>
LLMI_HD inline LabelGeom label_geom(uint64_t maps, uint32_t n, uint32_t ow, uint32_t oh) {
    return LabelGeom{maps, MB * uint64_t(n) * ow * oh, ow, oh, (oh + kLabelBoxRows - 1) / kLabelBoxRows};
}
// the bytes of band b of sample i: [lo, hi)
template <uint32_t MB>
LLMI_HD inline void label_band(const LabelGeom& g, uint32_t i, uint32_t b, uint64_t& sample, uint64_t& lo, uint64_t& hi) {
    const uint32_t y0 = b * kLabelBoxRows, y1 = g.oh - y0 < kLabelBoxRows ? g.oh : y0 + kLabelBoxRows;
    sample = g.maps + MB * uint64_t(i) * g.ow * g.oh;
    lo = sample + MB * uint64_t(y0) * g.ow, hi = sample + MB * uint64_t(y1) * g.ow;
}

// THE walk of a unit's pixels of the band, in order: runs of equal ids within a row collapsed, one update per run
struct LabelRunWalk {
    uint32_t x, y, xs, id;  // the last pixel's column and row, its run's first column and id
    template <class Sink>
    LLMI_HD inline void next(uint32_t m, uint32_t ow, Sink& sink) {  // the pixel behind it has id m
        ++x;
        if (x == ow) {
            sink.run(id, xs, x, y, x - xs);
            x = 0, xs = 0, ++y, id = m;
        } else if (m != id) {
            sink.run(id, xs, x, y, x - xs);
            xs = x, id = m;
        }
    }
    template <class Sink>
    LLMI_HD inline void end(Sink& sink) { sink.run(id, xs, x + 1, y, x + 1 - xs); }
};

// The unit at the aligned address u, which holds pixels of the band [lo, hi) of the sample at `sample`: its pixels of the band, runs of
// equal ids within a row collapsed, one update per run.  The unit is read whole where it lies inside the batch, pixel by pixel where
// it sticks out (chunk_read).
template <uint32_t MB, class Mem, class Sink>
LLMI_HD inline void label_boxes_unit(const LabelGeom& g, uint64_t sample, uint64_t lo, uint64_t hi, uint64_t u, Mem& mem, Sink& sink) {
    constexpr uint32_t PER = 16 / MB;
    const uint32_t p0 = (u < lo ? uint32_t(lo - u) : 0u) / MB, p1 = (u + 16 > hi ? uint32_t(hi - u) : 16u) / MB;
    if (p0 >= p1) return;
    const LabelChunk v = chunk_read<MB>(g.maps, g.bytes, u, p0, p1, mem);
    const uint32_t off = uint32_t((u + MB * p0 - sample) / MB);  // (in pixels: ow * oh < 2^32)
    const uint32_t y0 = off / g.ow, x0 = off - y0 * g.ow;
    LabelRunWalk w{x0, y0, x0, 0u};
    LLMI_UNROLL
    for (uint32_t p = 0; p < PER; ++p) {  // (p is a constant in every turn: the unit's words are never indexed by a variable)
        if (p < p0 || p >= p1) continue;
        const uint32_t m = chunk_get<MB>(v.w, p);
        if (p == p0) w.id = m;
        else w.next(m, g.ow, sink);
    }
    w.end(sink);
}
// ... of a 3-byte map: the band's pixels that BELONG to the unit, the straddling one's last bytes from the next unit
template <class Mem, class Sink>
LLMI_HD inline void label_boxes_unit3(const LabelGeom& g, uint64_t sample, uint64_t lo, uint64_t hi, uint64_t u, Mem& mem, Sink& sink) {
    uint32_t s;
    const uint32_t npx = chunk_pixels3(lo, hi, u, s), b1 = s + 3 * npx, phase = s % 3;
    if (!npx) return;
    const WideChunk v = chunk_read3(g.maps, g.bytes, u, s, b1, mem);
    const uint32_t off = uint32_t((u + s - sample) / 3);  // (in pixels: ow * oh < 2^32)
    const uint32_t y0 = off / g.ow, x0 = off - y0 * g.ow;
    LabelRunWalk w{x0, y0, x0, 0u};
    LLMI_UNROLL
    for (uint32_t b = 0; b < 16; ++b) {  // (b is a constant in every turn: a pixel's first byte)
        if (b % 3 != phase || b < s || b >= b1) continue;
        const uint32_t m = chunk_get3(v.w, b);
        if (b == s) w.id = m;
        else w.next(m, g.ow, sink);
    }
    w.end(sink);
}

// Thread t of the workgroup of the band [lo, hi): the band's aligned units t, t + 256, ...
template <uint32_t MB, class Mem, class Sink>
LLMI_HD inline void label_boxes_thread(const LabelGeom& g, uint64_t sample, uint64_t lo, uint64_t hi, uint32_t t, Mem& mem, Sink& sink) {
    for (uint64_t u = (lo & ~uint64_t(15)) + 16 * uint64_t(t); u < hi; u += 16 * uint64_t(kLabelThreads)) {
        if constexpr (MB == 3) label_boxes_unit3(g, sample, lo, hi, u, mem, sink);
        else label_boxes_unit<MB>(g, sample, lo, hi, u, mem, sink);
    }
}

}  // namespace llcomp_mi
