// batch_chunk.hpp -- sixteen bytes of a batch as the batch kernels hold them (mix_kernels.hip, orient_kernels.hip, compose_kernels.hip;
// DESIGN.md "Batch calls: what the three share"): four words, PER = 16 / ES elements, element e in word e * ES / 4.  The words are
// anything with a [] of uint32_t: the kernels' vector type Chunk below, and the array of compose_rule.hpp's ComposeChunk, which the
// host check walks too -- so the element's word and shift are stated here once, for the device and for g++.
#pragma once
#include <cstdint>

#include "geometry.hpp"

#define LLMI_CHUNK_FN LLMI_HD inline __attribute__((always_inline))

namespace llcomp_mi {

#if defined(__HIPCC__)
typedef uint32_t Chunk __attribute__((ext_vector_type(4)));
#endif
template <uint32_t ES> struct ElemOf;
template <> struct ElemOf<1> { using T = uint8_t; };
template <> struct ElemOf<2> { using T = uint16_t; };
template <> struct ElemOf<4> { using T = uint32_t; };

template <uint32_t ES, class W>
LLMI_CHUNK_FN uint32_t chunk_get(const W& v, uint32_t e) {
    if constexpr (ES == 4) return v[e];
    else if constexpr (ES == 2) return (v[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
    else return (v[e >> 2] >> (8 * (e & 3))) & 0xFFu;
}
template <uint32_t ES, class W>
LLMI_CHUNK_FN void chunk_set(W& v, uint32_t e, uint32_t bits) {
    if constexpr (ES == 4) v[e] = bits;
    else if constexpr (ES == 2) v[e >> 1] = (v[e >> 1] & ~(0xFFFFu << (16 * (e & 1)))) | (bits << (16 * (e & 1)));
    else v[e >> 2] = (v[e >> 2] & ~(0xFFu << (8 * (e & 3)))) | (bits << (8 * (e & 3)));
}
template <uint32_t ES, class W>
LLMI_CHUNK_FN void chunk_or(W& v, uint32_t e, uint32_t bits) {  // (into a chunk of zeros)
    if constexpr (ES == 4) v[e] = bits;
    else if constexpr (ES == 2) v[e >> 1] |= bits << (16 * (e & 1));
    else v[e >> 2] |= bits << (8 * (e & 3));
}

}  // namespace llcomp_mi
