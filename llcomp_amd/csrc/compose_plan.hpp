// compose_plan.hpp -- the host half of the batch composition (include/llcomp_mi.h: llcomp_mi_codec_compose_batch): the checks of a call,
// the stable sort of the pieces by dst sample, the samples that get workgroups with their runs of pieces (a CSR), and the table the
// call's one copy carries.  Plain C++ (compose_plan.cpp), like mix_plan.cpp and orient_plan.cpp: it builds and runs under a host sanitizer
// (tests/helpers/compose_plan_check.cpp).  The rule itself: compose_rule.hpp.  The kernel: compose_kernels.hip (compose.hpp).  The driver:
// codec.hip, llcomp_mi_codec_compose_batch.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"

namespace llcomp_mi {

// One dst sample with workgroups: a layer of the kernel's grid.  Its pieces are recs[first .. first + count) of the table, in the
// call's order.  Under KEEP a sample without pieces has no entry; otherwise every sample has one.
struct ComposeSample {
    uint32_t dst, first, count;
};
struct ComposePlan {
    std::vector<ComposeSample> samples;
    std::vector<uint32_t> order;  // the pieces with w and h above 0, by dst sample, each sample's in the call's order
};

// What travels in the call's one copy: the samples, the pieces as the kernel reads them (compose_rule.hpp: ComposeRec, 32 bytes) and the
// fill values in the dtype (one u32 per channel)
struct ComposeTable {
    uint64_t samples_at, recs_at, fill_at, bytes;
    ComposeTable(uint64_t n_samples, uint64_t n_recs, uint32_t c)
        : samples_at(0), recs_at(n_samples * sizeof(ComposeSample)), fill_at(recs_at + n_recs * 32), bytes(fill_at + 4 * uint64_t(c)) {}
};
inline uint64_t compose_table_bound(uint64_t n_dst, uint64_t n_pieces, uint32_t c) { return ComposeTable(n_dst, n_pieces, c).bytes; }

// A whole call but for its pointers into memory: include/llcomp_mi.h lists the refusals.  The fill values come back in the dtype in
// fill_bits[c] (NULL fill_value: zeros).
int compose_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, const float* fill_value, uint32_t flags,
                       std::vector<uint32_t>& fill_bits);
// ... and its pointers: src NULL with n_src above 0, a pointer not aligned to the element, byte ranges that overlap
int compose_check_memory(const void* src, uint64_t src_bytes, const void* dst, uint64_t dst_bytes, uint32_t esize);
// The plan of a checked call
void compose_plan(uint32_t n_dst, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, uint32_t flags, ComposePlan& p);
// The workgroups of a plan's call
uint64_t compose_workgroups(const ComposePlan& p, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout);
// The table of a checked call into `at`, ComposeTable(p.samples.size(), p.order.size(), c).bytes bytes
void compose_table_put(const llcomp_mi_compose_piece* pieces, const ComposePlan& p, const std::vector<uint32_t>& fill_bits, uint32_t layout, uint8_t* at);

// The rule on host memory (llcomp_mi_compose_reference)
int compose_reference(const void* src, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow, uint32_t oh,
                      uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, const float* fill_value,
                      uint32_t flags, void* out);

}  // namespace llcomp_mi
