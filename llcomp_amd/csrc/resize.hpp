// resize.hpp -- the launchers of the resampling of a resized regions decode (resize_kernels.hip; codec.hip: windows_resample;
// DESIGN.md "Crops of different sizes, resized to one shape").  What the host decides -- weights, entries, output format: resize_plan.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resize_plan.hpp"

namespace llcomp_mi {

// d_box [boxes][bh][bw][c] -> d_mid [entries][mh][ow][c] (rows [0, rh) of every entry: the horizontal pass, rounded to u8) -> d_px
// [entries][oh][ow][c] (the vertical pass, then the mirror).  The caller guarantees ox + rw <= bw, oy + rh <= bh, rh <= mh and a box
// inside d_box for every entry.  bias (a padded call with a constant fill other than 0): the kernels' bias forms, which start every
// accumulator at bias * fill -- every entry then names its bias arrays and the call's fill values in its pad[] (resize_plan.hpp).
hipError_t launch_resize(const uint8_t* d_box, uint8_t* d_mid, uint8_t* d_px, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t entries,
                         uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow, uint32_t oh, hipStream_t stream, bool bias = false);

// launch_resize with the vertical pass writing fmt's table entries in its layout (o.plain is launch_resize itself): d_table is the
// table of output_table in device memory, 4-byte aligned; d_out is aligned to o.esize.
hipError_t launch_resize_out(const uint8_t* d_box, uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const void* d_table,
                             const OutFormat& o, uint32_t entries, uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow,
                             uint32_t oh, hipStream_t stream, bool bias = false);

}  // namespace llcomp_mi
