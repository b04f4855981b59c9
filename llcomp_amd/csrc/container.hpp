// container.hpp -- wire-format helpers (host only, no GPU): the reference's 6-byte legacy header
// (/root/reference/llcomp.hpp:375-378, 463-470) and this project's sliced container (include/llcomp_mi.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "geometry.hpp"

struct llcomp_mi_view_group;  // include/llcomp_mi.h
struct llcomp_mi_info;

namespace llcomp_mi {

inline void put_u32le(uint8_t* p, uint32_t v) {
    p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); p[2] = uint8_t(v >> 16); p[3] = uint8_t(v >> 24);
}
inline uint32_t get_u32le(const uint8_t* p) {
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

void write_legacy_header(uint8_t* out6, uint32_t w, uint32_t h, uint32_t c);
void write_sliced_header(uint8_t* out24, const Geometry& g);  // g.frames must be 1

// The payload bytes [begin, end) that hold the slices of tile box {tx0, ty0, tx1, ty1} of a probed container of `len` bytes: from the
// first covered slice's first byte to the last one's end (slices run tile row, tile column, plane, so the span also holds what lies
// between them), both ends clamped to the payload that is there.  A LEGACY stream is one slice: [0, payload).
struct PayloadSpan {
    uint64_t begin, end;
};
PayloadSpan covered_span(const llcomp_mi_info& info, const uint8_t* data, size_t len, const uint32_t box[4]);

// Regions gather (llcomp_mi_regions_gather, and the host path of llcomp_mi_codec_decode_regions_host): which bytes of which container a
// regions decode needs.  A run is one window tile row of one frame: `count` consecutive table entries from entry `first` of container
// `frame`, and the payload bytes [src, src + bytes) of that container (offsets from its first byte).  Runs are in output order: class by
// class, frame order inside a class, tile rows top down.
struct GatherRun {
    uint32_t frame, first, count;
    uint64_t src, bytes;
};
struct RegionsGather {
    Geometry g{};                 // container 0's geometry, one frame
    uint32_t n_classes = 0, n_slices = 0;
    uint64_t payload_bytes = 0;
    std::vector<GatherRun> runs;
};
// every check of llcomp_mi_regions_gather; nothing is copied
int regions_gather_plan(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* xy, uint32_t rw, uint32_t rh,
                        RegionsGather& p);
// ... of a rectangle of its own size per frame (rects = {x, y, rw, rh} per frame), every window sized for wmax x hmax
// (regions_window_sized; llcomp_mi_codec_decode_resized_regions_host).  used != nullptr (llcomp_mi_codec_decode_views_host): only the
// n_used frames it lists, in its order, take part -- data / lens / rects are still indexed by frame, no other frame's container is
// looked at (it may be NULL), and `g` is the first listed container's geometry.
int regions_gather_plan_sized(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* rects, uint32_t wmax, uint32_t hmax,
                              RegionsGather& p, const uint32_t* used = nullptr, uint32_t n_used = 0);
// the planned bytes: payload (p.payload_bytes), slice_len (p.n_slices entries) and, when slice_off is not null, the offset of every
// slice in `payload`
void regions_gather_copy(const RegionsGather& p, const uint8_t* const* data, uint8_t* payload, uint32_t* slice_len, uint64_t* slice_off);

// Views (llcomp_mi_views_plan, llcomp_mi_codec_decode_views): every check of the plan, and per frame the union rectangle (bounding box)
// of its views over all groups -- rects[4f .. 4f + 3] = {x, y, rw, rh}, four zeros for a frame without a view -- the used frames in
// frame order, the largest union's sides and the number of views.
struct ViewsUnion {
    std::vector<uint32_t> rects;  // 4 * frames
    std::vector<uint32_t> used;
    uint32_t wmax = 0, hmax = 0;
    uint64_t total_views = 0;
};
// group i of an array of groups (its stride is the groups' struct_size, which views_union has checked)
const llcomp_mi_view_group* view_group_at(const llcomp_mi_view_group* groups, uint32_t i);
int views_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_view_group* groups, uint32_t n_groups, ViewsUnion& u);

}  // namespace llcomp_mi
