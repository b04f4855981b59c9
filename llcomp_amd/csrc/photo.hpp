// photo.hpp -- the launcher of one step of the photometric chains (photo_kernels.hip; codec.hip: windows_photo; DESIGN.md "Photometric
// chains").  What the host decides -- chunks, steps, the block of chains: photo_plan.hpp.  The rule: photo_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "photo_plan.hpp"

namespace llcomp_mi {

// Step `step` of the chains d_chains[views] on d_px [views][oh][ow][c] u8, in place: a view whose chain ends with this step -- or is
// empty, at step 0 -- is written to d_out [views][oh][ow][c] in format o instead (o.plain: u8 HWC; otherwise d_table is output_table's
// table in device memory, aligned to the element size, and d_out is aligned to it too); a view whose chain has ended sits out.
// stats: some view's op of this step reads statistics -- d_stats (views * photo_stats_stride(c) bytes, 8-byte aligned) is zeroed on the
// stream and filled by k_photo_stats first.  table: some view's op is a table -- k_photo_lut builds d_luts (views *
// photo_lut_stride(c) bytes) from the parameters and d_stats.  area: some view's op is the blur -- those views sit out of the per-pixel
// pass, and k_photo_blur_rows and k_photo_blur_cols run them, three passes each inside LDS and in place on d_px (the column kernel
// writes d_out where the blur ends the chain): no buffer beside d_px, and a view of any width and height.  sharp_rows, not 0: some
// view's op is the sharpness -- those views sit out of the per-pixel pass too, and k_photo_sharp runs them in bands of sharp_rows rows
// (photo_plan.hpp: PhotoGroup::sharp_rows), after k_photo_sharp_save has copied the rows between the bands to d_halo: views *
// photo_sharp_halo_bytes(ow, oh, c, sharp_rows) bytes, which the planner carved from the staging buffer behind the chunk's views (null
// where that is 0).  c is 1 or 3.
hipError_t launch_photo_step(uint8_t* d_px, const llcomp_mi_photo_chain* d_chains, void* d_stats, uint8_t* d_luts, const void* d_table,
                             const OutFormat& o, void* d_out, uint32_t views, uint32_t c, uint32_t ow, uint32_t oh, uint32_t step, bool stats,
                             bool table, bool area, uint8_t* d_halo, uint32_t sharp_rows, hipStream_t stream);

}  // namespace llcomp_mi
