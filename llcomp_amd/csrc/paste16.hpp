// paste16.hpp -- the launcher of the kernel of the batch copy-paste by 16-bit ids (paste16_kernels.hip; codec.hip:
// llcomp_mi_codec_paste_batch16; DESIGN.md "Batch copy-paste by 16-bit ids").  What the host decides -- the checks, the sort by dst, the
// table: paste16_plan.hpp.  The rule: paste16_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "paste.hpp"
#include "paste16_plan.hpp"

namespace llcomp_mi {

// One call: k_paste16, one workgroup per tile, per plane (CHW) and per entry of the table's samples.  o: PasteLaunch with d_mask
// n_src * ih * iw uint16_t aligned to 2 bytes and d_table the call's table in device memory (PasteTable16), 4-byte aligned.
hipError_t launch_paste16(const PasteLaunch& o, hipStream_t stream);

}  // namespace llcomp_mi
