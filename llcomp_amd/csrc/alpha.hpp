// alpha.hpp -- the launcher of the batch alpha paste's kernel (alpha_kernels.hip; codec.hip: llcomp_mi_codec_alpha_paste_batch;
// DESIGN.md "Batch alpha paste").  What the host decides -- the checks, the sort by dst, the table: alpha_plan.hpp.  The rule:
// alpha_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "alpha_plan.hpp"

namespace llcomp_mi {

// One call: k_alpha_paste<AB, DT>, one workgroup per tile, per plane (CHW) and per entry of the table's samples.  d_table: the call's
// table in device memory (AlphaTable), 4-byte aligned.
struct AlphaLaunch {
    const uint8_t* d_src;    // NULL: every piece is a VALUE piece
    const uint8_t* d_alpha;  // n_src * ih * iw pixels of alpha_px_bytes bytes at any address; NULL: every piece is an OVER piece
    uint8_t* d_dst;          // src and dst aligned to the element, with an OVER piece to 4 bytes
    const uint8_t* d_table;
    uint32_t n_samples, n_recs;  // of the table: the dst samples with workgroups, the pieces that are not ignored
    uint32_t alpha_px_bytes, alpha_byte;
    uint32_t n_src, iw, ih, n_dst, ow, oh, c, dtype, layout;  // checked (alpha_check_call)
    bool over;                                                // a piece has OVER: the instantiation that carries the rule
};
hipError_t launch_alpha_paste(const AlphaLaunch& o, hipStream_t stream);

}  // namespace llcomp_mi
