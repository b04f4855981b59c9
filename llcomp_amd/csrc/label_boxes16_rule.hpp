// label_boxes16_rule.hpp -- the rule of the label boxes of LISTED ids in 16-bit id maps (include/llcomp_mi.h: "Label boxes of listed
// ids"), stated ONCE on top of label_boxes_rule.hpp, whose record, identity and run update it keeps: the check of a call's lists, the
// table the lists travel in, the search of a run's id in a sample's sorted list, and what a thread does with one 16-byte unit of map
// memory (label_boxes16_unit).  Compiled into the kernel (label_boxes16_kernels.hip), into llcomp_mi_label_boxes16_reference
// (label_boxes16.cpp), which walks the kernel's own bands and units on the host, and into the stand-alone host check.
//
// A map is dense little-endian uint16_t aligned to 2 bytes, so a band of kLabelBoxRows rows is one byte range of even bounds and a
// pixel never straddles an aligned 16-byte unit: a unit holds 8 pixels, of which a thread uses those that belong to the band.
// Mem: load16 of an aligned unit, load_el<2> of a pixel.  Sink: run(id, x_first, x_end, y, length), in any order.
#pragma once
#include <cstdint>

#include "label_boxes_rule.hpp"

namespace llcomp_mi {

constexpr uint32_t kLabel16MaxIds = 4096;          // listed ids of a sample (llcomp_mi_label_boxes16_max_ids): 22 bytes of LDS per id
constexpr uint32_t kLabel16MaxTotal = 1u << 20;    // listed ids of a call
constexpr uint32_t kLabel16IdBytes = 2 + 5 * 4;    // of LDS per listed id: the id and the record's five words
constexpr uint32_t kLabel16None = 0xFFFFFFFFu;     // label_list_find: the id is not listed
constexpr uint32_t kLabel16Capacities[3] = {256, 1024, 4096};

// The capacity a call of lists of at most `longest` ids runs at
inline uint32_t label16_capacity(uint32_t longest) {
    return longest <= kLabel16Capacities[0] ? kLabel16Capacities[0] : longest <= kLabel16Capacities[1] ? kLabel16Capacities[1] : kLabel16Capacities[2];
}

// A whole call but for its device pointers.  *longest: the longest list; *n_listed: the samples with a list that is not empty.
inline int label_boxes16_check_call(uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids, const uint32_t* first, uint32_t* longest = nullptr,
                                    uint32_t* n_listed = nullptr) {
    if (int rc = batch_check_shape(n, 1, ow, oh, LLCOMP_MI_DTYPE_F16, LLCOMP_MI_LAYOUT_HWC)) return rc;  // (a 2-byte element)
    if (uint64_t(ow) * oh >= (1ull << 32) || !ids || !first || first[0] != 0) return LLCOMP_MI_BAD_ARGS;
    uint32_t most = 0, listed = 0;
    for (uint32_t i = 0; i < n; ++i) {  // (the bounds first: no id is read before first says where the ids end)
        if (first[i + 1] < first[i] || first[i + 1] > kLabel16MaxTotal) return LLCOMP_MI_BAD_ARGS;
        const uint32_t cnt = first[i + 1] - first[i];
        if (cnt > kLabel16MaxIds) return LLCOMP_MI_BAD_ARGS;
        most = cnt > most ? cnt : most, listed += cnt != 0;
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = first[i] + 1; j < first[i + 1]; ++j)
            if (ids[j] <= ids[j - 1]) return LLCOMP_MI_BAD_ARGS;
    if (longest) *longest = most;
    if (n_listed) *n_listed = listed;
    return LLCOMP_MI_OK;
}

// The table of a call in device memory: first[n + 1], then the n_listed samples that get workgroups, ascending, then the ids
struct Label16Table {
    uint64_t first_at, samples_at, ids_at, bytes;
    Label16Table(uint64_t n, uint64_t n_listed, uint64_t total) : first_at(0), samples_at(4 * (n + 1)), ids_at(samples_at + 4 * n_listed), bytes(ids_at + 2 * total) {}
};
inline uint64_t label16_table_bound(uint64_t n, uint64_t total_ids) { return Label16Table(n, n, total_ids).bytes; }

// id in the strictly ascending list[0 .. count): its index, or kLabel16None
template <class List>
LLMI_HD inline uint32_t label_list_find(const List& list, uint32_t count, uint32_t id) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uint32_t(list[mid]) < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < count && uint32_t(list[lo]) == id ? lo : kLabel16None;
}
// ... behind a comparison with the id of the thread's previous run, which neighbouring units mostly repeat
template <class List>
struct LabelFinder {
    List list;
    uint32_t count;
    uint32_t prev_id = kLabel16None, prev_slot = kLabel16None;  // (no id is 0xFFFFFFFF)
    LLMI_HD inline uint32_t find(uint32_t id) {
        if (id != prev_id) prev_id = id, prev_slot = label_list_find(list, count, id);
        return prev_slot;
    }
};

struct LabelGeom16 {
    uint64_t maps, bytes;  // the batch's first byte and its size
    uint32_t ow, oh, bands;
};
LLMI_HD inline LabelGeom16 label_geom16(uint64_t maps, uint32_t n, uint32_t ow, uint32_t oh) {
    return LabelGeom16{maps, 2 * uint64_t(n) * ow * oh, ow, oh, (oh + kLabelBoxRows - 1) / kLabelBoxRows};
}
// the bytes of band b of sample i: [lo, hi)
LLMI_HD inline void label_band16(const LabelGeom16& g, uint32_t i, uint32_t b, uint64_t& sample, uint64_t& lo, uint64_t& hi) {
    const uint32_t y0 = b * kLabelBoxRows, y1 = g.oh - y0 < kLabelBoxRows ? g.oh : y0 + kLabelBoxRows;
    sample = g.maps + 2 * uint64_t(i) * g.ow * g.oh;
    lo = sample + 2 * uint64_t(y0) * g.ow, hi = sample + 2 * uint64_t(y1) * g.ow;
}

// The unit at the aligned address u, which holds pixels of the band [lo, hi) of the sample at `sample`: its pixels of the band, runs of
// equal ids within a row collapsed, one update per run.  The unit is read whole where it lies inside the batch, pixel by pixel where
// it sticks out.  (lo, hi and sample are even: so are p0 and p1.)
template <class Mem, class Sink>
LLMI_HD inline void label_boxes16_unit(const LabelGeom16& g, uint64_t sample, uint64_t lo, uint64_t hi, uint64_t u, Mem& mem, Sink& sink) {
    const uint32_t p0 = (u < lo ? uint32_t(lo - u) : 0u) >> 1, p1 = (u + 16 > hi ? uint32_t(hi - u) : 16u) >> 1;
    if (p0 >= p1) return;
    LabelChunk v{{0u, 0u, 0u, 0u}};
    if (u >= g.maps && u + 16 <= g.maps + g.bytes) {
        v = mem.load16(u);
    } else {
        LLMI_LABEL_UNROLL
        for (uint32_t p = 0; p < 8; ++p)
            if (p >= p0 && p < p1) chunk_or<2>(v.w, p, mem.template load_el<2>(u + 2 * p));
    }
    const uint32_t off = uint32_t((u + 2 * p0 - sample) >> 1);  // (in pixels: ow * oh < 2^32)
    uint32_t y = off / g.ow, x = off - y * g.ow;
    uint32_t id = 0, xs = x;
    LLMI_LABEL_UNROLL
    for (uint32_t p = 0; p < 8; ++p) {  // (p is a constant in every turn: the unit's words are never indexed by a variable)
        if (p < p0 || p >= p1) continue;
        const uint32_t m = chunk_get<2>(v.w, p);
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

constexpr uint32_t kLabel16Threads = 256;  // of a workgroup
// Thread t of the workgroup of the band [lo, hi): the band's aligned units t, t + 256, ...
template <class Mem, class Sink>
LLMI_HD inline void label_boxes16_thread(const LabelGeom16& g, uint64_t sample, uint64_t lo, uint64_t hi, uint32_t t, Mem& mem, Sink& sink) {
    for (uint64_t u = (lo & ~uint64_t(15)) + 16 * uint64_t(t); u < hi; u += 16 * uint64_t(kLabel16Threads)) label_boxes16_unit(g, sample, lo, hi, u, mem, sink);
}

}  // namespace llcomp_mi
