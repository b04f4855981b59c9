// photo.hpp -- the launcher of one step of the photometric chains (photo_kernels.hip; codec.hip: windows_photo; DESIGN.md "Photometric
// chains").  What the host decides -- chunks, steps, the block of chains: photo_plan.hpp.  The rule: photo_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "photo_plan.hpp"

namespace llcomp_mi {

// One step of the chains of a chunk's views, in place on the views: a view whose chain ends with this step -- or is empty, at step 0 --
// is written to d_out instead; a view whose chain has ended sits out.
struct PhotoStep {
    uint8_t* d_px;                          // the views, [views][oh][ow][c] u8
    const llcomp_mi_photo_chain* d_chains;  // their chains, [views]
    uint8_t* d_stats;  // views * photo_stats_stride(c) bytes, 8-byte aligned: zeroed on the stream and filled by k_photo_stats where info.stats
    uint8_t* d_luts;   // views * photo_lut_stride(c) bytes: k_photo_lut builds them from the parameters and d_stats where info has kTable
    uint8_t* d_halo;   // views * photo_sharp_halo_bytes(ow, oh, c, sharp_rows) bytes at PhotoGroup::halo_at of the staging buffer, null
                       // where that is 0: k_photo_sharp_save copies the rows between the bands there where info has kSharp
    OutFormat out;     // of d_out [views][oh][ow][c].  plain: u8 HWC; otherwise d_table is output_table's table in device memory,
    const void* d_table;  // aligned to the element size, and d_out is aligned to it too
    void* d_out;
    uint32_t views, c, ow, oh, step;  // c is 1 or 3; a view of any width and height
    uint32_t sharp_rows;              // PhotoGroup::sharp_rows, the rows of a band of k_photo_sharp: read where info has kSharp
    PhotoStepInfo info;  // PhotoGroup::step[step]: it decides what is launched.  The views of kBlur and of kSharp sit out of the per-pixel
                         // pass: the row and the column kernel, or the band kernel, run them, in place too and with no buffer beside d_px
};
hipError_t launch_photo_step(const PhotoStep& p, hipStream_t stream);

}  // namespace llcomp_mi
