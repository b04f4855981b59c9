// compose.hpp -- the launcher of the batch composition's kernel (compose_kernels.hip; codec.hip: llcomp_mi_codec_compose_batch; DESIGN.md
// "Batch composition").  What the host decides -- the checks, the sort by dst, the table: compose_plan.hpp.  The rule: compose_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "compose_plan.hpp"

namespace llcomp_mi {

// One call: k_compose, one workgroup per tile, per plane (CHW) and per entry of the table's samples.  d_table: the call's table in
// device memory (ComposeTable), 4-byte aligned.  d_src may be NULL with n_src = 0.
struct ComposeLaunch {
    const uint8_t* d_src;
    uint8_t* d_dst;  // both aligned to the element
    const uint8_t* d_table;
    uint32_t n_samples, n_recs;  // of the table: the dst samples with workgroups, the pieces with w and h above 0
    uint32_t n_src, iw, ih, ow, oh, c, dtype, layout, keep;  // checked (compose_check_call)
};
hipError_t launch_compose(const ComposeLaunch& o, hipStream_t stream);

}  // namespace llcomp_mi
