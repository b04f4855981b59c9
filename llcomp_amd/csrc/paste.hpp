// paste.hpp -- the launcher of the batch copy-paste's kernel (paste_kernels.hip; codec.hip: llcomp_mi_codec_paste_batch and
// llcomp_mi_codec_paste_batch16; DESIGN.md "Batch copy-paste", "Batch copy-paste by 16-bit ids").  What the host decides -- the checks,
// the sort by dst, the table: paste_plan.hpp.  The rule: paste_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "paste_plan.hpp"

namespace llcomp_mi {

// One call: k_paste<MB, ES>, one workgroup per tile, per plane (CHW) and per entry of the table's samples.  d_table: the call's table in
// device memory (PasteTable<MB>), 4-byte aligned.
struct PasteLaunch {
    const uint8_t* d_src;
    const uint8_t* d_mask;  // n_src * ih * iw pixels of mask_bytes bytes, aligned to that
    uint8_t* d_dst;         // src and dst aligned to the element
    const uint8_t* d_table;
    uint32_t n_samples, n_recs;  // of the table: the dst samples with workgroups, the pieces that are not ignored
    uint32_t n_src, iw, ih, ow, oh, c, dtype, layout;  // checked (paste_check_call)
};
// mask_bytes: 1, 2, 3 or 4, the MB of the table's records (3: a mask at any address)
hipError_t launch_paste(const PasteLaunch& o, uint32_t mask_bytes, hipStream_t stream);

}  // namespace llcomp_mi
