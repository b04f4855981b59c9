// orient_plan.hpp -- the host half of the batch orientation (include/llcomp_mi.h: llcomp_mi_codec_orient_batch): the checks of a call and
// the table the call's one copy carries.  Plain C++ (orient_plan.cpp), like mix_plan.cpp: it builds and runs under a host sanitizer
// (tests/helpers/orient_plan_check.cpp).  The rule itself: orient_rule.hpp.  The kernel: orient_kernels.hip (orient.hpp).  The driver:
// codec.hip, llcomp_mi_codec_orient_batch.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"

namespace llcomp_mi {

// The side in pixels of the kernel's tile (llcomp_mi_orient_tile): a tile is this wide and, by the bytes of a pixel, 8 to this many
// rows tall (orient_kernels.hip)
constexpr uint32_t kOrientTile = 64;

// One oriented sample: a layer of the kernel's grid.  A sample with code 0 has no entry.
struct OrientEntry {
    uint32_t sample, code;
};
inline uint64_t orient_table_bound(uint64_t n) { return n * sizeof(OrientEntry); }

// A whole call but for its pointers into memory: BAD_ARGS for a NULL codes, a batch that is none (batch_ops.hpp: batch_check_shape), a
// code above 7, a transposing code with ow != oh
int orient_check_call(uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const uint8_t* codes);
// The table of a checked call: the samples whose code is not 0, in order
void orient_table(uint32_t n, const uint8_t* codes, std::vector<OrientEntry>& table);

// The rule on host memory (llcomp_mi_orient_reference)
int orient_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const uint8_t* codes,
                     void* out);

}  // namespace llcomp_mi
