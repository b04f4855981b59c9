// alpha_plan.hpp -- the host half of the batch alpha paste (include/llcomp_mi.h: llcomp_mi_codec_alpha_paste_batch): the checks of a
// call, the plan and the table the call's one copy carries.  The stable sort of the pieces by dst sample into ComposeSample runs, the
// shape and rectangle checks and the count of workgroups are the copy-paste's (paste_plan.hpp: paste_plan_by, PastePlan,
// paste_check_shapes, paste_piece_fits, paste_workgroups); what is written here is what differs: the flags, the values, which of src
// and alpha a call reads, and the 36-byte records.  Plain C++, like paste_plan.cpp: it builds and runs under a host sanitizer
// (tests/helpers/alpha_paste_check.cpp).  The rule itself: alpha_rule.hpp.  The kernel: alpha_kernels.hip (alpha.hpp).  The driver:
// codec.hip, alpha_paste_batch_call.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "paste_plan.hpp"

namespace llcomp_mi {

// What travels in the call's one copy: the samples and the pieces as the kernel reads them (alpha_rule.hpp: AlphaRec, 36 bytes)
struct AlphaTable {
    uint64_t samples_at, recs_at, bytes;
    AlphaTable(uint64_t n_samples, uint64_t n_recs) : samples_at(0), recs_at(n_samples * sizeof(ComposeSample)), bytes(recs_at + n_recs * 36) {}
};
inline uint64_t alpha_table_bound(uint64_t n_dst, uint64_t n_pieces) { return AlphaTable(n_dst, n_pieces).bytes; }

// What a checked call reads: src (a piece without VALUE), alpha (a piece without OVER); over: a piece with OVER
struct AlphaUses {
    bool src, alpha, over;
};
// A whole call but for its pointers into memory: include/llcomp_mi.h lists the refusals
int alpha_check_call(uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh,
                     uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, AlphaUses& uses);
// ... and its pointers: a NULL dst, a NULL src or alpha that the call reads, src or dst not aligned to the element (with OVER: to 4
// bytes), a dst that overlaps src or alpha
int alpha_check_memory(const void* src, uint64_t src_bytes, const void* alpha, uint64_t alpha_bytes, const void* dst, uint64_t dst_bytes, uint32_t esize,
                       const AlphaUses& uses);
// The plan of a checked call: the copy-paste's sort, a piece with w or h of 0 ignored
void alpha_plan(uint32_t n_dst, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, PastePlan& p);
// The table of a checked call into `at`, AlphaTable(p.samples.size(), p.order.size()).bytes bytes
void alpha_table_put(const llcomp_mi_alpha_piece* pieces, const PastePlan& p, uint32_t c, uint32_t layout, uint8_t* at);

}  // namespace llcomp_mi
