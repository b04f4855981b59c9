// label_targets_rule.hpp -- the rule of the label targets (include/llcomp_mi.h: "Label targets"), stated ONCE on top of batch_ops.hpp,
// batch_chunk.hpp and label_lists.hpp, whose list check and list search it keeps: the check of a call, the table a call travels
// in, the value of a pixel, and what a thread does with one 16-byte unit of MAP memory (label_targets_read_unit) and with one 16-byte
// unit of OUTPUT memory (label_targets_write_thread).  Compiled into the kernel (label_targets_kernels.hip), into
// llcomp_mi_label_targets_reference (label_targets.cpp) and into the stand-alone host check, which both walk the kernel's own
// workgroups, threads and units on the host (label_targets_host_workgroup below).
//
// Everything is linear in the pixel index p of a sample, for the map, for the index tensor and for every plane: there are no rows or
// columns here, only segments of kTargetSegment pixels.  A workgroup owns one segment of one sample (and, for PLANES, one chunk of
// kTargetPlaneChunk of that sample's planes): it looks every pixel of the segment up once and leaves the values in its LDS, then
// builds the aligned 16-byte units of output memory that the segment covers from them.  A unit that the segment covers only in part
// -- its other elements are the neighbouring segment's, plane's or sample's, or lie outside the output -- gets exactly its own
// elements, element by element: compose_rule.hpp's unit rule.  No output byte is written twice, none outside the output is touched.
// Mem: batch_chunk.hpp's (load16 of an aligned unit, load_el<MB> of a pixel; store16 of an aligned unit, store_el<ES> of an element).
// MB 3 and 4 (include/llcomp_mi.h "Wide id maps"): lists of uint32_t ids through label_finder32; a 3-byte pixel belongs to the unit
// that holds its first byte (batch_chunk.hpp: chunk_pixels3, chunk_read3); the output side does not know the map's width.
#pragma once
#include <cstdint>
#include <type_traits>

#include "batch_chunk.hpp"
#include "label_lists.hpp"

namespace llcomp_mi {

constexpr uint32_t kTargetSegment = 4096;     // pixels of a workgroup's segment (llcomp_mi_label_targets_segment)
constexpr uint32_t kTargetThreads = 256;      // of a workgroup
constexpr uint32_t kTargetMaxPlanes = 4096;   // of a sample (llcomp_mi_label_targets_max_planes): a plane index fits the uint16_t of the LDS
constexpr uint32_t kTargetPlaneChunk = 32;    // planes of a workgroup: what one look-up of the segment is shared by
constexpr uint32_t kTargetNoPlane = 0xFFFFu;  // PLANES: the value selects no plane
constexpr uint32_t kTargetIdBytes = 2 + 4;    // of LDS per listed id, map_bytes 2: the id and its value
constexpr uint32_t kTarget32IdBytes = 4 + 4;  // ... map_bytes 3 and 4

// The element's size in bytes, 0 for a kind or dtype that is none
LLMI_HD constexpr uint32_t target_esize(uint32_t kind, uint32_t dtype) {
    return kind == LLCOMP_MI_TARGET_PLANES ? batch_esize(dtype)
           : kind != LLCOMP_MI_TARGET_INDEX ? 0u
           : dtype == LLCOMP_MI_TARGET_U8 ? 1u : dtype == LLCOMP_MI_TARGET_I32 ? 4u : dtype == LLCOMP_MI_TARGET_I64 ? 8u : 0u;
}

// What a checked call is, but for its device pointers
struct TargetCall {
    uint32_t esize = 0, longest = 0, total = 0;
    uint32_t n_work = 0;       // samples that get workgroups: all for INDEX, those with a plane for PLANES
    uint32_t most_planes = 0;  // of a sample
    uint64_t out_bytes = 0;
};

// A whole call but for its device pointers: label_boxes16_check_call's check of the shape and of the lists (the bounds before any id
// is read), then the values, the planes and the output's size
// (T: llcomp_mi_label_targets, map_bytes 1 or 2, or llcomp_mi_label_targets32, map_bytes 3 or 4 -- the same fields but for the ids' type)
template <class T>
inline int label_targets_check_any(uint32_t n, uint32_t ow, uint32_t oh, const T* t, TargetCall& c) {
    constexpr bool kWide = std::is_same<T, llcomp_mi_label_targets32>::value;
    if (!t || t->struct_size < sizeof(T) || !t->values) return LLCOMP_MI_BAD_ARGS;
    if (kWide ? t->map_bytes != 3 && t->map_bytes != 4 : t->map_bytes != 1 && t->map_bytes != 2) return LLCOMP_MI_BAD_ARGS;
    c.esize = target_esize(t->kind, t->dtype);
    if (!c.esize) return LLCOMP_MI_BAD_ARGS;
    if constexpr (kWide) {
        if (int rc = label_boxes32_check_call(t->map_bytes, n, ow, oh, t->ids, t->first, &c.longest, nullptr)) return rc;
    } else {
        if (int rc = label_boxes16_check_call(n, ow, oh, t->ids, t->first, &c.longest, nullptr)) return rc;
    }
    c.total = t->first[n];
    if (t->map_bytes == 1)
        for (uint32_t i = 0; i < n; ++i)  // (ascending: the last id of a list is its largest)
            if (t->first[i + 1] != t->first[i] && t->ids[t->first[i + 1] - 1] > 255) return LLCOMP_MI_BAD_ARGS;
    uint64_t planes = n;
    if (t->kind == LLCOMP_MI_TARGET_INDEX) {
        if (t->dtype == LLCOMP_MI_TARGET_U8) {
            if (t->default_value < 0 || t->default_value > 255) return LLCOMP_MI_BAD_ARGS;
            for (uint32_t j = 0; j < c.total; ++j)
                if (t->values[j] < 0 || t->values[j] > 255) return LLCOMP_MI_BAD_ARGS;
        }
        c.n_work = n;
    } else {
        const uint32_t* pf = t->plane_first;
        if (!pf || pf[0] != 0) return LLCOMP_MI_BAD_ARGS;
        if (c.esize < 4 && ((t->on_bits | t->off_bits) >> (8 * c.esize)) != 0) return LLCOMP_MI_BAD_ARGS;  // (bits above the element)
        for (uint32_t i = 0; i < n; ++i) {
            if (pf[i + 1] < pf[i] || pf[i + 1] - pf[i] > kTargetMaxPlanes) return LLCOMP_MI_BAD_ARGS;
            const uint32_t cnt = pf[i + 1] - pf[i];
            c.most_planes = cnt > c.most_planes ? cnt : c.most_planes, c.n_work += cnt != 0;
        }
        planes = pf[n];
    }
    c.out_bytes = planes * ow * oh * c.esize;  // (below 2^28 * 2^32 * 2^3: no overflow)
    return (c.out_bytes >> 62) != 0 ? LLCOMP_MI_BAD_ARGS : LLCOMP_MI_OK;
}

inline int label_targets_check_call(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* t, TargetCall& c) {
    return label_targets_check_any(n, ow, oh, t, c);
}
inline int label_targets32_check_call(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* t, TargetCall& c) {
    return label_targets_check_any(n, ow, oh, t, c);
}

// The table of a call in device memory: first[n + 1], the n_work samples that get workgroups, ascending, plane_first[n + 1] (PLANES),
// the values, the ids, of id_bytes each
struct TargetTable {
    uint64_t first_at, samples_at, planes_at, values_at, ids_at, bytes;
    TargetTable(uint64_t n, uint64_t n_work, uint64_t total, bool planes, uint64_t id_bytes = 2)
        : first_at(0), samples_at(4 * (n + 1)), planes_at(samples_at + 4 * n_work), values_at(planes_at + (planes ? 4 * (n + 1) : 0)),
          ids_at(values_at + 4 * total), bytes(ids_at + id_bytes * total) {}
};
inline uint64_t target_table_bound(uint64_t n, uint64_t total_ids) { return TargetTable(n, n, total_ids, true).bytes; }
inline uint64_t target32_table_bound(uint64_t n, uint64_t total_ids) { return TargetTable(n, n, total_ids, true, 4).bytes; }

struct TargetGeom {
    uint64_t maps, map_bytes;  // the maps' first byte and their size
    uint64_t out;              // the output's first byte
    uint32_t pixels;           // P = ow * oh of a sample
    uint32_t segments;         // of a sample
};
LLMI_HD inline TargetGeom target_geom(uint64_t maps, uint64_t out, uint32_t n, uint32_t ow, uint32_t oh, uint32_t mb) {
    const uint64_t P = uint64_t(ow) * oh;
    return TargetGeom{maps, n * P * mb, out, uint32_t(P), uint32_t((P + kTargetSegment - 1) / kTargetSegment)};
}
// what does not depend on the sample
struct TargetParams {
    uint32_t kind, esize;
    int32_t default_value;
    uint32_t on_bits, off_bits;
};

// the pixels [s0, s1) of a sample that segment `seg` holds
LLMI_HD inline void target_segment(const TargetGeom& g, uint32_t seg, uint32_t& s0, uint32_t& s1) {
    s0 = seg * kTargetSegment;
    s1 = g.pixels - s0 < kTargetSegment ? g.pixels : s0 + kTargetSegment;
}

// What a listed value, or the default, is in a workgroup's table: itself for INDEX; for PLANES the plane it selects, or kTargetNoPlane
LLMI_HD inline uint32_t target_table_value(uint32_t kind, int32_t value, uint32_t planes) {
    return kind == LLCOMP_MI_TARGET_INDEX ? uint32_t(value) : uint32_t(value) < planes ? uint32_t(value) : kTargetNoPlane;
}

// Thread t's part of the workgroup's table, in two steps with a barrier behind each.  MB 1: vals is the dense table of 256 ids, the
// default everywhere (step 0), then the listed ids' values (step 1).  MB 2: list and vals are the sample's cnt ids and their values
// (step 0; nothing in step 1).  ids and values: the sample's list in the call's table.
template <uint32_t MB, class Ids, class Values, class List, class Vals>
LLMI_HD inline void label_targets_table_thread(uint32_t step, uint32_t t, const TargetParams& a, uint32_t planes, const Ids& ids, const Values& values,
                                               uint32_t cnt, List& list, Vals& vals) {
    if constexpr (MB == 1) {
        if (step == 0)
            for (uint32_t j = t; j < 256; j += kTargetThreads) vals[j] = target_table_value(a.kind, a.default_value, planes);
        else
            for (uint32_t j = t; j < cnt; j += kTargetThreads) vals[uint32_t(ids[j]) & 255u] = target_table_value(a.kind, values[j], planes);  // (checked: at most 255)
    } else {
        if (step == 0)
            for (uint32_t j = t; j < cnt; j += kTargetThreads) list[j] = ids[j], vals[j] = target_table_value(a.kind, values[j], planes);
    }
}

// v(i, p) of a pixel's id, as the table has it: MB 1 by the dense table, MB 2 and above by LabelFinder in the list
template <uint32_t MB, class List, class Vals>
struct TargetLookup {
    LabelFinder<List> finder;  // (MB 3 and 4: label_finder32's)
    Vals vals;
    uint32_t dflt;  // target_table_value of the default
    LLMI_HD inline uint32_t operator()(uint32_t id) {
        if constexpr (MB == 1) {
            return uint32_t(vals[id]);
        } else {
            const uint32_t j = finder.find(id);
            return j == kLabel16None ? dflt : uint32_t(vals[j]);
        }
    }
};

// The unit at the aligned address u, which holds pixels of the segment whose map bytes are [lo, hi): the values of its pixels of the
// segment into v, v[0] the segment's first pixel.  The unit is read whole where it lies inside the maps, pixel by pixel where it sticks
// out (chunk_read).  (MB 2: lo and hi are even.)
template <uint32_t MB, class Mem, class Lookup, class V>
LLMI_HD inline void label_targets_read_unit(const TargetGeom& g, uint64_t lo, uint64_t hi, uint64_t u, Mem& mem, Lookup& look, V& v) {
    if constexpr (MB == 3) {  // (the pixels that BELONG to the unit, the straddling one's last bytes from the next: batch_chunk.hpp)
        uint32_t s;
        const uint32_t npx = chunk_pixels3(lo, hi, u, s), b1 = s + 3 * npx, phase = s % 3;
        if (!npx) return;
        const WideChunk c = chunk_read3(g.maps, g.map_bytes, u, s, b1, mem);
        uint32_t at = uint32_t(u + s - lo) / 3;  // of the unit's first pixel in the segment (whose bytes are 3 * kTargetSegment at most)
        LLMI_UNROLL
        for (uint32_t b = 0; b < 16; ++b)  // (b is a constant in every turn: a pixel's first byte)
            if (b % 3 == phase && b >= s && b < b1) v[at++] = look(chunk_get3(c.w, b));
    } else {
        constexpr uint32_t PER = 16 / MB;
        const uint32_t p0 = (u < lo ? uint32_t(lo - u) : 0u) / MB, p1 = (u + 16 > hi ? uint32_t(hi - u) : 16u) / MB;
        if (p0 >= p1) return;
        const BatchChunk c = chunk_read<MB>(g.maps, g.map_bytes, u, p0, p1, mem);
        const uint32_t at = u < lo ? 0u : uint32_t((u - lo) / MB);  // of pixel p0 in the segment
        LLMI_UNROLL
        for (uint32_t p = 0; p < PER; ++p)  // (p is a constant in every turn: the unit's words are never indexed by a variable)
            if (p >= p0 && p < p1) v[at + p - p0] = look(chunk_get<MB>(c.w, p));
    }
}
// Thread t of the workgroup of segment [s0, s1) of sample i: the aligned units t, t + 256, ... of its map bytes
template <uint32_t MB, class Mem, class Lookup, class V>
LLMI_HD inline void label_targets_read_thread(const TargetGeom& g, uint32_t i, uint32_t s0, uint32_t s1, uint32_t t, Mem& mem, Lookup& look, V& v) {
    const uint64_t sample = g.maps + uint64_t(i) * g.pixels * MB, lo = sample + uint64_t(s0) * MB, hi = sample + uint64_t(s1) * MB;
    for (uint64_t u = (lo & ~uint64_t(15)) + 16 * uint64_t(t); u < hi; u += 16 * uint64_t(kTargetThreads)) label_targets_read_unit<MB>(g, lo, hi, u, mem, look, v);
}

// The bits of the element of plane k (PLANES) for the table value vv of its pixel
template <uint32_t KIND, uint32_t ES>
LLMI_HD inline uint64_t target_element(uint32_t vv, uint32_t k, const TargetParams& a) {
    if constexpr (KIND == LLCOMP_MI_TARGET_PLANES) return vv == k ? a.on_bits : a.off_bits;
    else if constexpr (ES == 8) return uint64_t(int64_t(int32_t(vv)));  // (sign-extended)
    else if constexpr (ES == 1) return vv & 0xFFu;                      // (checked: 0..255)
    else return vv;
}
template <uint32_t ES, class W>
LLMI_CHUNK_FN void target_unit_put(W& w, uint32_t e, uint64_t bits) {  // (into a unit of zeros)
    if constexpr (ES == 8) w[2 * e] = uint32_t(bits), w[2 * e + 1] = uint32_t(bits >> 32);
    else chunk_or<ES>(w, e, uint32_t(bits));
}

// The elements at [a0, a1) of output memory -- of the index tensor or of plane k -- whose pixels' table values are v[0], v[1], ...:
// thread t's aligned units t, t + 256, ...  A unit inside [a0, a1) is built whole and stored once; one that sticks out gets its own
// elements.  (a0 and a1 are multiples of ES.)
template <uint32_t KIND, uint32_t ES, class V, class Sink>
LLMI_HD inline void label_targets_write_thread(uint64_t a0, uint64_t a1, uint32_t t, uint32_t k, const TargetParams& a, const V& v, Sink& sink) {
    constexpr uint32_t PER = 16 / ES;
    for (uint64_t u = (a0 & ~uint64_t(15)) + 16 * uint64_t(t); u < a1; u += 16 * uint64_t(kTargetThreads)) {
        const uint32_t e0 = u < a0 ? uint32_t(a0 - u) / ES : 0u, e1 = u + 16 > a1 ? uint32_t(a1 - u) / ES : PER;
        const uint32_t at = u < a0 ? 0u : uint32_t((u - a0) / ES);  // of element e0 in the segment
        if (e0 == 0 && e1 == PER) {
            BatchChunk c{{0u, 0u, 0u, 0u}};
            LLMI_UNROLL
            for (uint32_t e = 0; e < PER; ++e) target_unit_put<ES>(c.w, e, target_element<KIND, ES>(uint32_t(v[at + e]), k, a));
            sink.store16(u, c);
        } else {
            LLMI_UNROLL
            for (uint32_t e = 0; e < PER; ++e)
                if (e >= e0 && e < e1) sink.template store_el<ES>(u + ES * e, target_element<KIND, ES>(uint32_t(v[at + e - e0]), k, a));
        }
    }
}
// Thread t of the workgroup of segment [s0, s1) of sample i: the segment of the index tensor, or of the planes [k0, k1) of the
// sample, whose first plane is plane `plane0` of the call
template <uint32_t KIND, uint32_t ES, class V, class Sink>
LLMI_HD inline void label_targets_write_segment(const TargetGeom& g, uint32_t i, uint32_t s0, uint32_t s1, uint32_t plane0, uint32_t k0, uint32_t k1, uint32_t t,
                                                const TargetParams& a, const V& v, Sink& sink) {
    const uint64_t len = uint64_t(s1 - s0) * ES;
    if constexpr (KIND == LLCOMP_MI_TARGET_INDEX) {
        const uint64_t a0 = g.out + (uint64_t(i) * g.pixels + s0) * ES;
        label_targets_write_thread<KIND, ES>(a0, a0 + len, t, 0u, a, v, sink);
    } else {
        for (uint32_t k = k0; k < k1; ++k) {
            const uint64_t a0 = g.out + ((uint64_t(plane0) + k) * g.pixels + s0) * ES;
            label_targets_write_thread<KIND, ES>(a0, a0 + len, t, k, a, v, sink);
        }
    }
}
// ... with the element's size a switch: the sizes of the kind
template <uint32_t KIND, class V, class Sink>
LLMI_HD inline void label_targets_write_any(const TargetGeom& g, uint32_t i, uint32_t s0, uint32_t s1, uint32_t plane0, uint32_t k0, uint32_t k1, uint32_t t,
                                            const TargetParams& a, const V& v, Sink& sink) {
    constexpr uint32_t WIDE = KIND == LLCOMP_MI_TARGET_INDEX ? 8 : 2;  // (INDEX: 1, 4, 8; PLANES: 1, 2, 4)
    if (a.esize == 1) label_targets_write_segment<KIND, 1>(g, i, s0, s1, plane0, k0, k1, t, a, v, sink);
    else if (a.esize == 4) label_targets_write_segment<KIND, 4>(g, i, s0, s1, plane0, k0, k1, t, a, v, sink);
    else label_targets_write_segment<KIND, WIDE>(g, i, s0, s1, plane0, k0, k1, t, a, v, sink);
}

// The kernel's workgroup (segment seg of sample i, plane chunk z) on the host, its phases one after the other and its threads one
// after the other within a phase: the lists and the planes as the call's table has them, the workgroup's LDS arrays list, vals (of
// the capacity the call runs at) and v (of kTargetSegment) the caller's -- llcomp_mi_label_targets_reference's plain ones, the
// stand-alone check's checking ones.
template <class Id, class Mem, class Sink, class List, class Vals, class V>
inline void label_targets_host_workgroup(const TargetGeom& g, const TargetParams& a, uint32_t mb, const uint32_t* first, const uint32_t* plane_first, const int32_t* values,
                                         const Id* ids, uint32_t i, uint32_t seg, uint32_t z, Mem& mem, Sink& sink, List& list, Vals& vals, V& v) {
    const bool planar = a.kind == LLCOMP_MI_TARGET_PLANES;
    const uint32_t planes = planar ? plane_first[i + 1] - plane_first[i] : 0u, plane0 = planar ? plane_first[i] : 0u;
    const uint32_t k0 = z * kTargetPlaneChunk, k1 = planes - k0 < kTargetPlaneChunk ? planes : k0 + kTargetPlaneChunk;
    if (planar && k0 >= planes) return;
    const uint32_t at = first[i], cnt = first[i + 1] - at;
    uint32_t s0, s1;
    target_segment(g, seg, s0, s1);
    for (uint32_t step = 0; step < 2; ++step)
        for (uint32_t t = 0; t < kTargetThreads; ++t) {
            if (mb == 1) label_targets_table_thread<1>(step, t, a, planes, ids + at, values + at, cnt, list, vals);
            else label_targets_table_thread<2>(step, t, a, planes, ids + at, values + at, cnt, list, vals);  // (the list: the same for 2, 3 and 4)
        }
    const uint32_t dflt = target_table_value(a.kind, a.default_value, planes);
    for (uint32_t t = 0; t < kTargetThreads; ++t) {
        if (mb == 1) {
            TargetLookup<1, List&, Vals&> look{{list, cnt}, vals, dflt};
            label_targets_read_thread<1>(g, i, s0, s1, t, mem, look, v);
        } else if (mb == 2) {
            TargetLookup<2, List&, Vals&> look{{list, cnt}, vals, dflt};
            label_targets_read_thread<2>(g, i, s0, s1, t, mem, look, v);
        } else if (mb == 3) {
            TargetLookup<3, List&, Vals&> look{label_finder32<List&>(list, cnt), vals, dflt};
            label_targets_read_thread<3>(g, i, s0, s1, t, mem, look, v);
        } else {
            TargetLookup<4, List&, Vals&> look{label_finder32<List&>(list, cnt), vals, dflt};
            label_targets_read_thread<4>(g, i, s0, s1, t, mem, look, v);
        }
    }
    for (uint32_t t = 0; t < kTargetThreads; ++t) {
        if (planar) label_targets_write_any<LLCOMP_MI_TARGET_PLANES>(g, i, s0, s1, plane0, k0, k1, t, a, v, sink);
        else label_targets_write_any<LLCOMP_MI_TARGET_INDEX>(g, i, s0, s1, 0u, 0u, 0u, t, a, v, sink);
    }
}
// the plane chunks of a call's grid
inline uint32_t target_plane_chunks(uint32_t kind, uint32_t most_planes) {
    return kind == LLCOMP_MI_TARGET_PLANES ? (most_planes + kTargetPlaneChunk - 1) / kTargetPlaneChunk : 1u;
}

}  // namespace llcomp_mi
