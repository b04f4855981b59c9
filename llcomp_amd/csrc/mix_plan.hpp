// mix_plan.hpp -- the host half of the batch mixing (include/llcomp_mi.h: llcomp_mi_codec_mix_batch): the checks of a call, the partner
// permutation cut into the segments the kernel's threads walk, which heads are saved first, and the table the call's one copy carries.
// Plain C++ (mix_plan.cpp), like photo_plan.cpp: it builds and runs under a host sanitizer (tests/helpers/mix_plan_check.cpp).  The rule
// itself: mix_rule.hpp.  The kernels: mix_kernels.hip (mix.hpp).  The driver: codec.hip, llcomp_mi_codec_mix_batch.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"

namespace llcomp_mi {

// The samples one thread of k_mix walks for its chunk (DESIGN.md "Batch mixing" has the measurement behind the number): a cycle of the
// partners of more than this many samples is cut into segments of at most this many, as equal as they come.
#ifndef LLMI_MIX_SEGMENT  // (csrc/Makefile `mixseg`: the builds tools/ubench/mix_batch.py compares the lengths on)
#define LLMI_MIX_SEGMENT 8
#endif
constexpr uint32_t kMixSegment = LLMI_MIX_SEGMENT;
static_assert(kMixSegment >= 2, "a segment of one sample would save every sample of a cycle");
constexpr uint32_t kMixNoSlot = 0xFFFFFFFFu;

// One segment: samples order[first .. first + count), each the partner of the one before it.  The partner of the LAST one is the head of
// the cycle's next segment, which that segment's threads may have overwritten: it is read from slot tail_slot of the saved heads -- or,
// tail_slot = kMixNoSlot, the segment is a whole cycle and that partner is its own head, which the thread still holds.  slot_sample
// belongs to the entry's INDEX, not to its segment: the sample saved in slot `index`, for index < n_saved.
struct MixSeg {
    uint32_t first, count, tail_slot, slot_sample;
};
struct MixPlan {
    std::vector<uint32_t> order;
    std::vector<MixSeg> segs;
    uint32_t n_saved = 0;
};

// The most heads a call of n samples saves: a cycle of L > kMixSegment samples has ceil(L / kMixSegment) segments, at most 2 L / (kMixSegment + 1)
inline uint64_t mix_saved_bound(uint64_t n) { return n > kMixSegment ? 2 * n / (kMixSegment + 1) : 0; }
// A slot of the saved heads: the sample's bytes at the sample's own offset from a multiple of 16, so that a chunk is aligned in the one
// where it is in the other
inline uint64_t mix_slot_stride(uint64_t sample_bytes) { return (sample_bytes + 15) / 16 * 16 + 16; }

// What travels in the call's one copy: the records, the order, the segments and the erase values in the dtype (one u32 per channel)
struct MixTable {
    uint64_t recs_at, order_at, segs_at, erase_at, bytes;
    MixTable(uint64_t n, uint64_t n_segments, uint32_t c)
        : recs_at(0), order_at(n * sizeof(llcomp_mi_mix_sample)), segs_at(order_at + 4 * n), erase_at(segs_at + n_segments * sizeof(MixSeg)),
          bytes(erase_at + 4 * uint64_t(c)) {}
};
inline uint64_t mix_table_bound(uint64_t n, uint32_t c) { return MixTable(n, n, c).bytes; }

// The records by themselves: BAD_ARGS for n = 0 or above kBatchMaxSamples (batch_ops.hpp), a partner >= n, partners that are no
// permutation, flag bits above 0, a weight that is not finite
int mix_check_records(uint32_t n, const llcomp_mi_mix_sample* samples);
// ... and a whole call: the batch (batch_ops.hpp: batch_check_shape), the rectangles within ow x oh, BLEND on U8, and the erase values,
// which come back in the dtype in erase_bits[c] (NULL erase_value: zeros)
int mix_check_call(uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_mix_sample* samples,
                   const float* erase_value, std::vector<uint32_t>& erase_bits);
// The plan of checked records
void mix_plan(uint32_t n, const llcomp_mi_mix_sample* samples, MixPlan& p);
// The table of a checked call into `at`, MixTable(n, p.segs.size(), c).bytes bytes
void mix_table_put(uint32_t n, const llcomp_mi_mix_sample* samples, const MixPlan& p, const std::vector<uint32_t>& erase_bits, uint8_t* at);

// The rule on host memory (llcomp_mi_mix_reference)
int mix_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                  const llcomp_mi_mix_sample* samples, const float* erase_value, void* out);

}  // namespace llcomp_mi
