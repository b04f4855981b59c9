// update.hpp -- launchers of the region update's kernels (update_kernels.hip; codec.hip: llcomp_mi_codec_encode_region /
// llcomp_mi_codec_update_region; DESIGN.md "Region update").  All launches are asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "geometry.hpp"

namespace llcomp_mi {

// The caller's rectangle d_rect[frames][rh][rw][c] -> the box pixels d_box[frames][bh][bw][c] at (x0, y0) of every frame.  The caller
// guarantees x0 + rw <= bw and y0 + rh <= bh; nothing outside the rectangle is written, nothing past either buffer is read.
hipError_t launch_paste_rect(const uint8_t* d_rect, uint8_t* d_box, uint32_t frames, uint32_t c, uint32_t rw, uint32_t rh, uint32_t bw,
                             uint32_t bh, uint32_t x0, uint32_t y0, hipStream_t stream);
// The new table of the full batch: d_new_len[i] = d_sub_len[region_sub_id(i)] for a covered slice, d_old_len[i] for every other one
// (elementwise).
hipError_t launch_merge_table(const Geometry& full, const Geometry& sub, const RegionBox& box, const uint32_t* d_old_len,
                              const uint32_t* d_sub_len, uint32_t* d_new_len, hipStream_t stream);
// Every slice of the full batch to its place in the new payload: a covered slice from the encoder's scratch (d_units: 16-byte units in
// the SUB-geometry's stream lane order, kernels.hpp), every other one from the old payload.  d_old_goff / d_new_goff: the group offsets
// of the full geometry for the old and the new table (launch_group_sums + launch_scan_groups).  A slice that would end past payload_cap
// is not written (kStOverflow, as launch_pack_payload); an uncovered slice whose bytes run past old_bytes is not read (kStTruncated).
hipError_t launch_splice_slices(const Geometry& full, const Geometry& sub, const RegionBox& box, const uint8_t* d_old_payload, uint64_t old_bytes,
                                const uint32_t* d_old_len, const uint64_t* d_old_goff, const uint8_t* d_units, const uint32_t* d_new_len,
                                const uint64_t* d_new_goff, uint8_t* d_payload, uint64_t payload_cap, uint32_t* d_status, hipStream_t stream);

}  // namespace llcomp_mi
