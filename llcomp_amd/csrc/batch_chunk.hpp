// batch_chunk.hpp -- sixteen bytes of a batch as the batch kernels hold them (mix_kernels.hip, orient_kernels.hip, compose_kernels.hip;
// DESIGN.md "Batch calls: what the three share"): four words, PER = 16 / ES elements, element e in word e * ES / 4.  The words are
// anything with a [] of uint32_t: the kernels' vector type Chunk below, and the array of BatchChunk, the unit of the rules that the host
// checks walk too (compose_rule.hpp, paste_rule.hpp, label_boxes_rule.hpp, label_targets_rule.hpp) -- so the element's word and shift
// are stated here once, for the device and for g++.  And the two memories those rules run on: DeviceMem, global memory as it is, and
// PlainMem, host memory as it is (the references); the host checks bring checking ones of the same four functions.
#pragma once
#include <cstdint>
#include <cstring>

#include "geometry.hpp"

#define LLMI_CHUNK_FN LLMI_HD inline __attribute__((always_inline))
#if defined(__clang__)
#define LLMI_UNROLL _Pragma("unroll")
#else
#define LLMI_UNROLL
#endif

namespace llcomp_mi {

#if defined(__HIPCC__)
typedef uint32_t Chunk __attribute__((ext_vector_type(4)));
#endif
template <uint32_t ES> struct ElemOf;
template <> struct ElemOf<1> { using T = uint8_t; };
template <> struct ElemOf<2> { using T = uint16_t; };
template <> struct ElemOf<4> { using T = uint32_t; };
template <> struct ElemOf<8> { using T = uint64_t; };

// 16 bytes, for the host checks as for the kernels; the names the composition's and the label calls' rules and checks know it by
struct BatchChunk {
    uint32_t w[4];
};
using ComposeChunk = BatchChunk;
using LabelChunk = BatchChunk;

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

// The memory of the rules: load16 / store16 of aligned 16-byte units, load_el<N> / store_el<N> of an N-byte element at an address
// aligned to N (the bits in the low N bytes)
#if defined(__HIPCC__)
struct DeviceMem {
    __device__ inline __attribute__((always_inline)) BatchChunk load16(uint64_t a) const {
        const Chunk v = *reinterpret_cast<const Chunk*>(__builtin_assume_aligned(reinterpret_cast<const void*>(a), 16));
        return BatchChunk{{v[0], v[1], v[2], v[3]}};
    }
    __device__ inline __attribute__((always_inline)) void store16(uint64_t a, const BatchChunk& c) const {
        *reinterpret_cast<Chunk*>(__builtin_assume_aligned(reinterpret_cast<void*>(a), 16)) = Chunk{c.w[0], c.w[1], c.w[2], c.w[3]};
    }
    template <uint32_t N>
    __device__ inline __attribute__((always_inline)) uint32_t load_el(uint64_t a) const {
        if constexpr (N == 3) {  // (a 3-byte pixel, at any address: three byte loads)
            const uint8_t* p = reinterpret_cast<const uint8_t*>(a);
            return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16;
        } else {
            return *reinterpret_cast<const typename ElemOf<N>::T*>(a);
        }
    }
    template <uint32_t N>
    __device__ inline __attribute__((always_inline)) void store_el(uint64_t a, uint64_t bits) const {
        *reinterpret_cast<typename ElemOf<N>::T*>(a) = static_cast<typename ElemOf<N>::T>(bits);
    }
};
#endif
// The aligned unit at u of a batch of N-byte pixels at [base, base + bytes), of which the pixels [p0, p1) are wanted: read whole where
// it lies inside the batch, pixel by pixel where it sticks out (the other pixels: zeros).  What the label calls read their maps with.
template <uint32_t N, class Mem>
LLMI_CHUNK_FN BatchChunk chunk_read(uint64_t base, uint64_t bytes, uint64_t u, uint32_t p0, uint32_t p1, Mem& mem) {
    if (u >= base && u + 16 <= base + bytes) return mem.load16(u);
    BatchChunk v{{0u, 0u, 0u, 0u}};
    LLMI_UNROLL
    for (uint32_t p = 0; p < 16 / N; ++p)
        if (p >= p0 && p < p1) chunk_or<N>(v.w, p, mem.template load_el<N>(u + N * p));
    return v;
}

// 3-byte pixels (the wide id maps, include/llcomp_mi.h "Wide id maps") lie at any byte address, so one may straddle two units: a pixel
// BELONGS to the unit that holds its first byte, and that unit's thread reads the pixel's other bytes, at most two, from the next
// unit.  WideChunk: a unit's four words and the next unit's first, bytes 0 .. 19 of a run of memory.
struct WideChunk {
    uint32_t w[5];
};
// the 3-byte pixel whose first byte is byte b <= 15 of the run (b a constant after unrolling: the words are never indexed by a variable)
template <class W>
LLMI_CHUNK_FN uint32_t chunk_get3(const W& w, uint32_t b) {
    const uint32_t k = b >> 2, sh = 8 * (b & 3);
    uint32_t v = w[k] >> sh;
    if (sh > 8) v |= w[k + 1] << (32 - sh);
    return v & 0xFFFFFFu;
}
// The bytes [b0, b1) of the run at the aligned address u, b0 < 16 and b1 <= 18, all of them inside the batch at [base, base + bytes):
// the unit read whole where it lies inside the batch, byte by byte where it sticks out, and the bytes 16 and 17 one by one (the
// other bytes: zeros, or the batch's)
template <class Mem>
LLMI_CHUNK_FN WideChunk chunk_read3(uint64_t base, uint64_t bytes, uint64_t u, uint32_t b0, uint32_t b1, Mem& mem) {
    WideChunk v{{0u, 0u, 0u, 0u, 0u}};
    if (u >= base && u + 16 <= base + bytes) {
        const BatchChunk c = mem.load16(u);
        v.w[0] = c.w[0], v.w[1] = c.w[1], v.w[2] = c.w[2], v.w[3] = c.w[3];
    } else {
        LLMI_UNROLL
        for (uint32_t b = 0; b < 16; ++b)
            if (b >= b0 && b < b1) chunk_or<1>(v.w, b, mem.template load_el<1>(u + b));
    }
    if (b1 > 16) v.w[4] = mem.template load_el<1>(u + 16);
    if (b1 > 17) v.w[4] |= mem.template load_el<1>(u + 17) << 8;
    return v;
}
// The 3-byte pixels of the byte range [lo, hi) -- lo a pixel's first byte, hi - lo a multiple of 3 -- that belong to the unit at u:
// their count, 0 to 6; s: the first one's first byte in the unit.  The pixels' bytes are [s, s + 3 * count) of the unit's run.
LLMI_CHUNK_FN uint32_t chunk_pixels3(uint64_t lo, uint64_t hi, uint64_t u, uint32_t& s) {
    const uint64_t a0 = u <= lo ? lo : u + (3u - uint32_t((u - lo) % 3u)) % 3u, end = u + 16 < hi ? u + 16 : hi;
    s = uint32_t(a0 - u);
    return a0 < end ? (uint32_t(end - a0) + 2u) / 3u : 0u;
}

struct PlainMem {  // (little-endian hosts, like the containers)
    BatchChunk load16(uint64_t a) const {
        BatchChunk v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), 16);
        return v;
    }
    void store16(uint64_t a, const BatchChunk& c) const { std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &c, 16); }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) const {
        uint32_t v = 0;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);
        return v;
    }
    template <uint32_t N>
    void store_el(uint64_t a, uint64_t bits) const {
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &bits, N);
    }
};

}  // namespace llcomp_mi
