// warp.hpp -- the launcher of the gather kernel of the warped views (warp_kernels.hip; codec.hip: windows_warp; DESIGN.md "Views under an
// affine map").  What the host decides -- entries, index tables, fills, output tables: warp_plan.hpp.  The rule: warp_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "warp_plan.hpp"

namespace llcomp_mi {

// d_box [boxes][bh][bw][c] -> d_out [views][oh][ow][c] in format o (o.plain: u8 HWC; otherwise d_table is output_table's table in device
// memory, aligned to the element size, and d_out is aligned to it too): view v is the rule of warp_rule.hpp for entry d_ws[v] on its
// frame (w x h), read through the frame's box, with the group's c fill bytes at d_fill.  The caller guarantees that every entry's box lies
// inside d_box and holds the entry's source rectangle; the kernel clamps every read into the box all the same.
hipError_t launch_warp(const uint8_t* d_box, const WarpEntry* d_ws, const int32_t* d_tabs, const uint8_t* d_fill, const void* d_table,
                       const OutFormat& o, void* d_out, uint32_t views, uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow,
                       uint32_t oh, hipStream_t stream);
// The same for the views of a perspective call (entries d_ps, no index tables): a kernel of its own, so that the affine instantiations
// keep their registers.
hipError_t launch_persp(const uint8_t* d_box, const PerspEntry* d_ps, const uint8_t* d_fill, const void* d_table, const OutFormat& o, void* d_out,
                        uint32_t views, uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, hipStream_t stream);

}  // namespace llcomp_mi
