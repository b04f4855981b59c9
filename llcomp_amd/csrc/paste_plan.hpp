// paste_plan.hpp -- the host half of the batch copy-paste for both widths of id map (include/llcomp_mi.h: llcomp_mi_codec_paste_batch,
// llcomp_mi_codec_paste_batch16): the checks of a call, the stable sort of the pieces by dst sample, the samples that get workgroups
// with their runs of pieces (a CSR, compose_plan.hpp's ComposeSample), and the table the call's one copy carries.  Written once over
// the piece type P, llcomp_mi_paste_piece or llcomp_mi_paste_piece16 (paste_plan.cpp instantiates both).  Plain C++, like
// compose_plan.cpp: it builds and runs under a host sanitizer (tests/helpers/paste_check.cpp).  The rule itself: paste_rule.hpp.  The
// kernel: paste_kernels.hip (paste.hpp).  The driver: codec.hip, paste_batch_call.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "compose_plan.hpp"

namespace llcomp_mi {

// The dst samples with a piece that is not ignored, ascending, and the pieces by dst sample, each sample's in the call's order
struct PastePlan {
    std::vector<ComposeSample> samples;
    std::vector<uint32_t> order;
};

// What travels in the call's one copy: the samples and the pieces as the kernel reads them (paste_rule.hpp: PasteRec<MB>, 68 or 72 bytes)
template <uint32_t MB>
struct PasteTable {
    uint64_t samples_at, recs_at, bytes;
    PasteTable(uint64_t n_samples, uint64_t n_recs) : samples_at(0), recs_at(n_samples * sizeof(ComposeSample)), bytes(recs_at + n_recs * (MB == 1 ? 68 : 72)) {}
};
template <uint32_t MB>
inline uint64_t paste_table_bound(uint64_t n_dst, uint64_t n_pieces) { return PasteTable<MB>(n_dst, n_pieces).bytes; }

// What the checks of a call share with the alpha paste's (alpha_plan.cpp): the two batches' shapes, the count of the pieces and the
// kernel's grid ...
int paste_check_shapes(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       bool has_pieces, uint32_t n_pieces);  // has_pieces: the caller's array of pieces is not NULL
// ... and a piece's samples and rectangles inside the batches
template <class P>
inline bool paste_piece_fits(const P& p, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh) {
    if (p.dst >= n_dst || p.src >= n_src) return false;
    if (p.dx > ow || p.w > ow - p.dx || p.dy > oh || p.h > oh - p.dy) return false;
    return !(p.sx > iw || p.w > iw - p.sx || p.sy > ih || p.h > ih - p.sy);
}

// (P: llcomp_mi_paste_piece, llcomp_mi_paste_piece16, or paste_rule.hpp's PastePiece3 / PastePiece4 for the wide call.)
// A whole call but for its pointers into memory: include/llcomp_mi.h lists the refusals.  The pieces' values come back in the dtype's
// bits in value_bits[n_pieces] (0 without VALUE).
template <class P>
int paste_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                     const P* pieces, uint32_t n_pieces, std::vector<uint32_t>& value_bits);
// ... and its pointers: a NULL dst, a NULL src or mask with pieces, src or dst not aligned to the element, a mask not aligned to
// mask_px (a power of two: paste_mask_align), a dst that overlaps src or mask
int paste_check_memory(const void* src, uint64_t src_bytes, const void* mask, uint64_t mask_bytes, const void* dst, uint64_t dst_bytes,
                       uint32_t esize, uint32_t mask_px, uint32_t n_pieces);
// The plan of a checked call
template <class P>
void paste_plan(uint32_t n_dst, const P* pieces, uint32_t n_pieces, PastePlan& p);
// ... written over what "ignored" means for a piece, so that the alpha paste (alpha_plan.cpp) sorts its own pieces the same way: a
// counting sort by dst sample, stable
template <class P, class Idle>
inline void paste_plan_by(uint32_t n_dst, const P* pieces, uint32_t n_pieces, PastePlan& p, Idle idle) {
    p = PastePlan{};
    std::vector<uint32_t> at(size_t(n_dst) + 1, 0u);
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!idle(pieces[i])) ++at[pieces[i].dst + 1];
    for (uint32_t d = 0; d < n_dst; ++d) {
        if (at[d + 1]) p.samples.push_back(ComposeSample{d, at[d], at[d + 1]});
        at[d + 1] += at[d];
    }
    p.order.resize(at[n_dst]);
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!idle(pieces[i])) p.order[at[pieces[i].dst]++] = i;
}
// The workgroups of a plan's call
uint64_t paste_workgroups(const PastePlan& p, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout);
// The table of a checked call into `at`, PasteTable<MB>(p.samples.size(), p.order.size()).bytes bytes
template <class P>
void paste_table_put(const P* pieces, const PastePlan& p, const std::vector<uint32_t>& value_bits, uint32_t c, uint32_t layout, uint8_t* at);

// The rule on host memory (llcomp_mi_paste_reference, llcomp_mi_paste16_reference)
template <class P>
int paste_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                    uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const P* pieces, uint32_t n_pieces, void* out);

}  // namespace llcomp_mi
