// mix.hpp -- the launcher of the batch mixing's kernels (mix_kernels.hip; codec.hip: llcomp_mi_codec_mix_batch; DESIGN.md "Batch
// mixing").  What the host decides -- the checks, the segments, the table: mix_plan.hpp.  The rule: mix_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mix_plan.hpp"

namespace llcomp_mi {

// One call, in place on d_batch: k_mix_save copies the n_saved heads into d_saved (n_saved slots of mix_slot_stride bytes; null where
// there is none), then k_mix walks every segment.  d_table: the call's table (mix_table_put) in device memory, 4-byte aligned.
struct MixLaunch {
    uint8_t* d_batch;  // aligned to the element
    uint8_t* d_saved;  // 16-byte aligned
    const uint8_t* d_table;
    uint32_t n, c, ow, oh, dtype, layout;  // checked (mix_check_call)
    uint32_t n_segments, n_saved;
};
hipError_t launch_mix(const MixLaunch& m, hipStream_t stream);

}  // namespace llcomp_mi
