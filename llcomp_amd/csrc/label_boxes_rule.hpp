// label_boxes_rule.hpp -- the rule of the label boxes (include/llcomp_mi.h: "Label boxes"), stated ONCE: the record's identity, the
// update of a record by a run of equal bytes, and what a thread does with one 16-byte unit of map memory (label_boxes_unit).  Compiled
// into the kernel (label_boxes_kernels.hip) and into llcomp_mi_label_boxes_reference (label_boxes.cpp), which walks the kernel's own
// bands and units on the host.
//
// A sample's rows are dense, so a band of kLabelBoxRows rows is one byte range; a workgroup takes it in the aligned 16-byte units of
// MEMORY it lies in, of which a thread uses the bytes that belong to the band -- the others are the neighbouring band's or sample's.
// Mem: load16 of an aligned unit, load_el<1> of a byte.  Sink: run(id, x_first, x_end, y, length), in any order.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "batch_chunk.hpp"
#include "batch_ops.hpp"

#if defined(__clang__)
#define LLMI_LABEL_UNROLL _Pragma("unroll")
#else
#define LLMI_LABEL_UNROLL
#endif

namespace llcomp_mi {

constexpr uint32_t kLabelIds = 256;      // records of a sample
constexpr uint32_t kLabelBoxRows = 32;   // rows of a workgroup's band (llcomp_mi_label_boxes_rows)

// the record of an id without a pixel: the identities of min and max
LLMI_HD inline llcomp_mi_label_box label_box_identity(uint32_t ow, uint32_t oh) { return llcomp_mi_label_box{0u, ow, oh, 0u, 0u}; }
// THE run update: `length` pixels of the id in columns [x_first, x_end) of row y
LLMI_HD inline void label_box_update(llcomp_mi_label_box& b, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
    b.count += length;
    b.x0 = x_first < b.x0 ? x_first : b.x0, b.x1 = x_end > b.x1 ? x_end : b.x1;
    b.y0 = y < b.y0 ? y : b.y0, b.y1 = y + 1 > b.y1 ? y + 1 : b.y1;
}

// A whole call but for its pointers
LLMI_HD inline int label_boxes_check_call(uint32_t n, uint32_t ow, uint32_t oh) {
    if (int rc = batch_check_shape(n, 1, ow, oh, LLCOMP_MI_DTYPE_U8, LLCOMP_MI_LAYOUT_HWC)) return rc;
    return uint64_t(ow) * oh >= (1ull << 32) ? LLCOMP_MI_BAD_ARGS : LLCOMP_MI_OK;
}

struct LabelGeom {
    uint64_t maps, bytes;  // the batch's first byte and its size
    uint32_t ow, oh, bands;
};
LLMI_HD inline LabelGeom label_geom(uint64_t maps, uint32_t n, uint32_t ow, uint32_t oh) {
    return LabelGeom{maps, uint64_t(n) * ow * oh, ow, oh, (oh + kLabelBoxRows - 1) / kLabelBoxRows};
}
// the bytes of band b of sample i: [lo, hi)
LLMI_HD inline void label_band(const LabelGeom& g, uint32_t i, uint32_t b, uint64_t& sample, uint64_t& lo, uint64_t& hi) {
    const uint32_t y0 = b * kLabelBoxRows, y1 = g.oh - y0 < kLabelBoxRows ? g.oh : y0 + kLabelBoxRows;
    sample = g.maps + uint64_t(i) * g.ow * g.oh;
    lo = sample + uint64_t(y0) * g.ow, hi = sample + uint64_t(y1) * g.ow;
}

struct LabelChunk {
    uint32_t w[4];
};

// The unit at the aligned address u, which holds bytes of the band [lo, hi) of the sample at `sample`: its bytes of the band, runs of
// equal bytes within a row collapsed, one update per run.  The unit is read whole where it lies inside the batch, byte by byte where
// it sticks out.
template <class Mem, class Sink>
LLMI_HD inline void label_boxes_unit(const LabelGeom& g, uint64_t sample, uint64_t lo, uint64_t hi, uint64_t u, Mem& mem, Sink& sink) {
    const uint32_t p0 = u < lo ? uint32_t(lo - u) : 0u, p1 = u + 16 > hi ? uint32_t(hi - u) : 16u;
    if (p0 >= p1) return;
    LabelChunk v{{0u, 0u, 0u, 0u}};
    if (u >= g.maps && u + 16 <= g.maps + g.bytes) {
        v = mem.load16(u);
    } else {
        LLMI_LABEL_UNROLL
        for (uint32_t p = 0; p < 16; ++p)
            if (p >= p0 && p < p1) chunk_or<1>(v.w, p, mem.template load_el<1>(u + p));
    }
    const uint32_t off = uint32_t(u + p0 - sample);
    uint32_t y = off / g.ow, x = off - y * g.ow;
    uint32_t id = 0, xs = x;
    LLMI_LABEL_UNROLL
    for (uint32_t p = 0; p < 16; ++p) {  // (p is a constant in every turn: the unit's words are never indexed by a variable)
        if (p < p0 || p >= p1) continue;
        const uint32_t m = chunk_get<1>(v.w, p);
        if (p == p0) {
            id = m;
            continue;
        }
        ++x;
        if (x == g.ow) {
            sink.run(id, xs, x, y, x - xs);
            x = 0, xs = 0, ++y, id = m;
        } else if (m != id) {
            sink.run(id, xs, x, y, x - xs);
            xs = x, id = m;
        }
    }
    sink.run(id, xs, x + 1, y, x + 1 - xs);
}

}  // namespace llcomp_mi
