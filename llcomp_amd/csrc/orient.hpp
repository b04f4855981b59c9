// orient.hpp -- the launcher of the batch orientation's kernel (orient_kernels.hip; codec.hip: llcomp_mi_codec_orient_batch; DESIGN.md
// "Batch orientation").  What the host decides -- the checks, the table: orient_plan.hpp.  The rule: orient_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orient_plan.hpp"

namespace llcomp_mi {

// One call, in place on d_batch: k_orient, one workgroup per tile of the code's fundamental domain, per plane (CHW) or piece of a pixel
// (HWC) and per entry of the table.  d_table: n_entries OrientEntry in device memory, 4-byte aligned.  code_set: bit `code` for every
// code among the entries (it sizes the grid).
struct OrientLaunch {
    uint8_t* d_batch;  // aligned to the element
    const uint8_t* d_table;
    uint32_t n_entries, code_set;
    uint32_t c, ow, oh, dtype, layout;  // checked (orient_check_call)
};
hipError_t launch_orient(const OrientLaunch& o, hipStream_t stream);

}  // namespace llcomp_mi
