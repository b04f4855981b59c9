// paste16_plan.hpp -- the host half of the batch copy-paste by 16-bit ids (include/llcomp_mi.h: llcomp_mi_codec_paste_batch16): the
// checks of a call, the stable sort of the pieces by dst sample (paste_plan.hpp's PastePlan), and the table the call's one copy
// carries.  Plain C++ (paste16_plan.cpp): it builds and runs under a host sanitizer (tests/helpers/paste16_check.cpp).  The rule
// itself: paste16_rule.hpp.  The kernel: paste16_kernels.hip (paste16.hpp).  The driver: codec.hip, llcomp_mi_codec_paste_batch16.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "paste_plan.hpp"

namespace llcomp_mi {

// What travels in the call's one copy: the samples and the pieces as the kernel reads them (paste16_rule.hpp: PasteRec16, 72 bytes)
struct PasteTable16 {
    uint64_t samples_at, recs_at, bytes;
    PasteTable16(uint64_t n_samples, uint64_t n_recs) : samples_at(0), recs_at(n_samples * sizeof(ComposeSample)), bytes(recs_at + n_recs * 72) {}
};
inline uint64_t paste16_table_bound(uint64_t n_dst, uint64_t n_pieces) { return PasteTable16(n_dst, n_pieces).bytes; }

// A whole call but for its pointers into memory: include/llcomp_mi.h lists the refusals
int paste16_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces);
// ... and its pointers: paste_check_memory's cases, and a mask not aligned to 2 bytes
int paste16_check_memory(const void* src, uint64_t src_bytes, const void* mask, uint64_t mask_bytes, const void* dst, uint64_t dst_bytes,
                         uint32_t esize, uint32_t n_pieces);
// The plan of a checked call
void paste16_plan(uint32_t n_dst, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, PastePlan& p);
// The table of a checked call into `at`, PasteTable16(p.samples.size(), p.order.size()).bytes bytes
void paste16_table_put(const llcomp_mi_paste_piece16* pieces, const PastePlan& p, uint32_t c, uint32_t layout, uint8_t* at);

// The rule on host memory (llcomp_mi_paste16_reference)
int paste16_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                      uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, void* out);

}  // namespace llcomp_mi
