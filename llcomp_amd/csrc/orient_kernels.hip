// orient_kernels.hip -- the batch orientation on the GPU (include/llcomp_mi.h: "Batch orientation"; DESIGN.md "Batch orientation"): flips,
// quarter turns and transpositions per sample, in place on a dense batch with no scratch in device memory.  The rule, the fundamental
// domains and the images of rectangles are orient_rule.hpp's, the functions llcomp_mi_orient_reference is compiled from; the table is
// orient_plan.hpp's, the 16-byte chunk batch_chunk.hpp's.
//
// A workgroup owns one tile of its code's fundamental domain: kOrientTile pixels wide, orient_tile_rows() tall, clipped to the domain's
// box; a pixel of the tile outside the domain (under a diagonal, right of the middle of a half turn's middle row) is masked out.  The
// tile's pixels p and their images s(p), s(s(p)), ... under the code's map s (out(q) = in(s(q))) are whole orbits, K = 2 or 4 rectangles
// of the sample (orient_rect_src) that no other workgroup touches.  The workgroup reads rectangle k into slot k of LDS, row by row as
// it lies in memory, waits at ONE barrier, and writes every rectangle k, again row by row, each pixel q from where s(q) lies in slot
// k + 1.  It reads everything before it writes anything, and different workgroups own disjoint orbits: that is the in-place argument.
// A pixel that is its own image is in no domain and in no image of one, so it is neither read nor written -- but for the diagonal of a
// transposition, whose square tiles are their own images and move whole (k_orient).
#include "orient.hpp"

#include <hip/hip_runtime.h>

#include "batch_chunk.hpp"
#include "orient_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kOrientThreads = 256;
// The most bytes of a pixel that a workgroup moves at once.  A CHW pixel is one element; an HWC pixel of up to 16 bytes moves whole,
// and a longer one in pieces of 16 / esize channels, a workgroup each (more than 4 float32 channels, 8 of 16 bits, 16 bytes).
constexpr uint32_t kOrientPieceBytes = 16;
// The rows of a tile for pieces of g bytes: the power of two that keeps kOrientTile * rows * g within 8 KiB, at most kOrientTile
__host__ __device__ constexpr uint32_t orient_tile_rows(uint32_t g) {
    uint32_t r = kOrientTile;
    while (r * g > 128) r /= 2;
    return r;
}
// A slot's row in LDS: the row's bytes at the offset from a multiple of 16 that they have in memory (up to 15 bytes of lead), rounded
// up to 16, and of 16 (mod 32) bytes in all, so that the rows a transposed read walks down start 4 banks apart and not 8 or 0
__host__ __device__ constexpr uint32_t orient_row_stride(uint32_t row_bytes) {
    const uint32_t rs = (row_bytes + 15) / 16 * 16 + 16;
    return rs % 32 == 16 ? rs : rs + 16;
}
constexpr uint32_t kOrientSlotBytes = kOrientTile * 128 + kOrientTile * 48;  // 11 KiB; four slots: 44 KiB, three workgroups to a CU
constexpr uint32_t kOrientTurns = 3;  // the most 16-byte units of a rectangle to a thread
constexpr bool orient_slots_fit() {
    for (uint32_t g = 1; g <= kOrientPieceBytes; ++g) {
        const uint32_t r = orient_tile_rows(g);
        if (r < 1 || r * orient_row_stride(kOrientTile * g) > kOrientSlotBytes || kOrientTile * orient_row_stride(r * g) > kOrientSlotBytes) return false;
        if (r * ((kOrientTile * g + 15) / 16 + 1) > kOrientTurns * kOrientThreads || kOrientTile * ((r * g + 15) / 16 + 1) > kOrientTurns * kOrientThreads) return false;
    }
    return true;
}
// The width of a tile: kOrientTile, but as many pixels as the tile has rows under the two transpositions, whose domains are triangles:
// square tiles from the corner the diagonal starts in are above it, below it or cut by it corner to corner
__host__ __device__ constexpr uint32_t orient_tile_width(uint32_t code, uint32_t rows) {
    return code == LLCOMP_MI_ORIENT_TRANSPOSE || code == LLCOMP_MI_ORIENT_TRANSVERSE ? rows : kOrientTile;
}
static_assert(orient_slots_fit(), "a tile and its transposed image must fit a slot, and their units the threads' turns, for every piece size");

struct OrientArgs {
    uint8_t* batch;
    const OrientEntry* table;
    uint64_t sample_bytes, plane_bytes;
    uint32_t ow, oh;
    uint32_t planes;   // CHW: c planes of one-element pixels; HWC: 1
    uint32_t cstride;  // elements from a pixel to the next: CHW 1, HWC c
    uint32_t cpiece;   // elements of a pixel in a piece (the last piece of a pixel may have fewer)
    uint32_t pieces;   // pieces to a pixel
    uint32_t rows;     // of a tile
};

// What a workgroup knows of its tile, the same in every thread
struct OrientTile {
    uint8_t* base;  // channel c0 of pixel (0, 0) of the sample's plane: element (x, y, ch) at ((y * ow + x) * cstride + ch) * ES
    uint32_t code, order, ow, oh, cstride, cg;
    OrientRect d;  // the tile
    bool whole;    // every pixel of the tile is in the domain
    bool wide;     // the pieces are whole pixels: a rectangle's row is one run of bytes

    // rectangle k: the image of the tile under the map applied k times
    __device__ __forceinline__ OrientRect rect(uint32_t k) const { return k ? orient_rect_src(orient_power(code, k), ow, oh, d) : d; }
    // does the pixel q of rectangle k move?  (its pixel of the tile, the map applied order - k times more, has to be in the domain)
    __device__ __forceinline__ bool moves(uint32_t k, uint32_t qx, uint32_t qy) const {
        if (whole) return true;
        const OrientXY p = k ? orient_src(orient_power(code, order - k), ow, oh, qx, qy) : OrientXY{qx, qy};
        return orient_in_domain(code, ow, oh, p.x, p.y);
    }
    __device__ __forceinline__ uint64_t row_offset(uint32_t x, uint32_t y) const { return (uint64_t(y) * ow + x) * cstride; }  // in elements
    // where channel ch of the pixel (x, y) of rectangle r lies in the rectangle's slot, in bytes from the slot
    template <uint32_t ES>
    __device__ __forceinline__ uint32_t in_slot(const OrientRect& r, uint32_t x, uint32_t y, uint32_t ch) const {
        const uint32_t stride = orient_row_stride((r.x1 - r.x0) * cg * ES);
        const uint32_t lead = wide ? uint32_t(reinterpret_cast<uintptr_t>(base + row_offset(r.x0, y) * ES) & 15u) : 0u;
        return (y - r.y0) * stride + lead + ((x - r.x0) * cg + ch) * ES;
    }
};

// One pass over rectangle k: STORE false, memory -> slot k; STORE true, slot k + 1 -> memory, the pixel q from where s(q) lies
template <uint32_t ES, bool STORE>
__device__ __forceinline__ void orient_pass(const OrientTile& t, uint32_t k, uint8_t* lds) {
    using T = typename ElemOf<ES>::T;
    constexpr uint32_t PER = 16 / ES;
    const OrientRect r = t.rect(k);
    const uint32_t bw = r.x1 - r.x0, bh = r.y1 - r.y0, row_el = bw * t.cg;
    uint8_t* const own = lds + k * kOrientSlotBytes;
    const uint32_t k2 = k + 1 == t.order ? 0u : k + 1;
    const OrientRect r2 = t.rect(k2);
    const uint8_t* const from = lds + k2 * kOrientSlotBytes;
    auto source = [&](uint32_t qx, uint32_t qy, uint32_t ch) -> uint32_t {  // the element that (qx, qy, ch) takes, from slot k2
        const OrientXY s = orient_src(t.code, t.ow, t.oh, qx, qy);
        return *reinterpret_cast<const T*>(from + t.in_slot<ES>(r2, s.x, s.y, ch));
    };
    if (!t.wide) {  // a piece of a longer pixel: element by element, the channels of the piece innermost
        for (uint32_t i = threadIdx.x; i < bh * row_el; i += kOrientThreads) {
            const uint32_t row = i / row_el, ei = i - row * row_el, lx = ei / t.cg, ch = ei - lx * t.cg;
            const uint32_t qx = r.x0 + lx, qy = r.y0 + row;
            if (!t.moves(k, qx, qy)) continue;
            T* g = reinterpret_cast<T*>(t.base + (t.row_offset(qx, qy) + ch) * ES);
            if constexpr (STORE) *g = T(source(qx, qy, ch));
            else *reinterpret_cast<T*>(own + t.in_slot<ES>(r, qx, qy, ch)) = *g;
        }
        return;
    }
    // a row is row_el * ES bytes from its address on: the 16-byte units of memory it lies in, whole where the row covers a unit and every
    // element of it moves, otherwise the unit's elements that belong to the row and move, one by one
    const uint32_t row_bytes = row_el * ES, units = (row_bytes + 15) / 16 + 1, total = bh * units;
    // At most kOrientTurns units to a thread (orient_slots_fit).  Reading, a thread asks for all its whole units before it puts the
    // first into LDS, so that its loads are in flight together.
    Chunk held[kOrientTurns];
    uint8_t* held_for[kOrientTurns];
#pragma unroll
    for (uint32_t turn = 0; turn < kOrientTurns; ++turn) {
        held_for[turn] = nullptr;
        const uint32_t i = threadIdx.x + turn * kOrientThreads;
        if (i >= total) continue;
        const uint32_t row = i / units, j = i - row * units, qy = r.y0 + row;
        uint8_t* const g_row = t.base + t.row_offset(r.x0, qy) * ES;
        const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(g_row) & 15u);
        const int32_t at = int32_t(16 * j) - int32_t(lead);  // the unit's first byte, from the row's first
        if (at >= int32_t(row_bytes)) continue;
        const bool covered = at >= 0 && at + 16 <= int32_t(row_bytes);
        const int32_t e0 = at / int32_t(ES);  // the unit's first element, from the row's first (below 0: in front of the row)
        uint32_t lx = e0 > 0 ? uint32_t(e0) / t.cg : 0u, ch = e0 > 0 ? uint32_t(e0) - lx * t.cg : 0u;
        uint32_t m = 0;
        Chunk v = {0u, 0u, 0u, 0u};
        if (STORE || !covered || !t.whole) {
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e) {
                const int32_t ei = e0 + int32_t(e);
                if (ei < 0 || ei >= int32_t(row_el)) continue;
                if (t.moves(k, r.x0 + lx, qy)) {
                    m |= 1u << e;
                    if constexpr (STORE) chunk_or<ES>(v, e, source(r.x0 + lx, qy, ch));
                }
                if (++ch == t.cg) ch = 0, ++lx;
            }
        } else {
            m = (1u << PER) - 1u;
        }
        const bool all = covered && m == (1u << PER) - 1u;
        uint8_t* const g = g_row + at;                                         // (a multiple of 16)
        uint8_t* const l = own + row * orient_row_stride(row_bytes) + 16 * j;  // = the slot's row + lead + at
        if constexpr (STORE) {
            if (all) {
                *reinterpret_cast<Chunk*>(__builtin_assume_aligned(g, 16)) = v;
            } else {
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e)
                    if ((m >> e) & 1u) reinterpret_cast<T*>(g)[e] = T(chunk_get<ES>(v, e));
            }
        } else {
            if (all) {
                held[turn] = *reinterpret_cast<const Chunk*>(__builtin_assume_aligned(g, 16));
                held_for[turn] = l;
            } else {
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e)
                    if ((m >> e) & 1u) reinterpret_cast<T*>(l)[e] = reinterpret_cast<const T*>(g)[e];
            }
        }
    }
    if constexpr (!STORE) {
#pragma unroll
        for (uint32_t turn = 0; turn < kOrientTurns; ++turn)
            if (held_for[turn]) *reinterpret_cast<Chunk*>(__builtin_assume_aligned(held_for[turn], 16)) = held[turn];
    }
}

template <uint32_t ES>
__global__ __launch_bounds__(kOrientThreads) void k_orient(OrientArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kOrientSlotBytes];
    const OrientEntry en = a.table[blockIdx.z];
    OrientTile t;
    t.code = en.code, t.order = orient_order(en.code), t.ow = a.ow, t.oh = a.oh, t.cstride = a.cstride;
    const OrientXY box = orient_domain_box(t.code, a.ow, a.oh);
    const uint32_t tile_w = orient_tile_width(t.code, a.rows);
    const uint32_t tiles_x = (box.x + tile_w - 1) / tile_w, tiles_y = (box.y + a.rows - 1) / a.rows;
    if (uint64_t(blockIdx.x) >= uint64_t(tiles_x) * tiles_y) return;  // (the grid is the largest domain's among the call's codes)
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    t.d.x0 = tx * tile_w, t.d.y0 = ty * a.rows;
    t.d.x1 = box.x - t.d.x0 < tile_w ? box.x : t.d.x0 + tile_w;
    t.d.y1 = box.y - t.d.y0 < a.rows ? box.y : t.d.y0 + a.rows;
    if (t.code == LLCOMP_MI_ORIENT_TRANSVERSE) {  // its tiles count from the right edge: the antidiagonal then cuts them corner to corner
        const uint32_t from_right = t.d.x0;
        t.d.x0 = a.ow - t.d.x1, t.d.x1 = a.ow - from_right;
    }
    const uint32_t cover = orient_rect_in_domain(t.code, a.ow, a.oh, t.d);
    if (!cover) return;  // (a tile under the diagonal)
    t.whole = cover == 2;
    if ((t.code == LLCOMP_MI_ORIENT_TRANSPOSE || t.code == LLCOMP_MI_ORIENT_TRANSVERSE) && tx == ty) {
        // A square tile on the diagonal of a transposition is its own image.  It is ONE rectangle: read whole, written whole, every
        // pixel from where its source lies in the same slot; the pixels of the diagonal itself are written with what they held.
        t.order = 1, t.whole = true;
    }
    const uint32_t plane = blockIdx.y / a.pieces, piece = blockIdx.y - plane * a.pieces, c0 = piece * a.cpiece;
    t.cg = a.cstride - c0 < a.cpiece ? a.cstride - c0 : a.cpiece;
    t.wide = t.cg == a.cstride;
    t.base = a.batch + uint64_t(en.sample) * a.sample_bytes + uint64_t(plane) * a.plane_bytes + uint64_t(c0) * ES;
    for (uint32_t k = 0; k < t.order; ++k) orient_pass<ES, false>(t, k, lds);
    __syncthreads();
    for (uint32_t k = 0; k < t.order; ++k) orient_pass<ES, true>(t, k, lds);
}

// The tiles of the largest domain among the codes of the set
uint64_t orient_grid_tiles(uint32_t code_set, uint32_t ow, uint32_t oh, uint32_t rows) {
    uint64_t most = 0;
    for (uint32_t code = 1; code < kOrientCodes; ++code) {
        if (!((code_set >> code) & 1u)) continue;
        const OrientXY box = orient_domain_box(code, ow, oh);
        const uint32_t tile_w = orient_tile_width(code, rows);
        const uint64_t tiles = uint64_t((box.x + tile_w - 1) / tile_w) * ((box.y + rows - 1) / rows);
        most = tiles > most ? tiles : most;
    }
    return most;
}

}  // namespace

hipError_t launch_orient(const OrientLaunch& o, hipStream_t stream) {
    const uint32_t es = batch_esize(o.dtype);
    const bool chw = o.layout == LLCOMP_MI_LAYOUT_CHW;
    OrientArgs a{};
    a.batch = o.d_batch, a.table = reinterpret_cast<const OrientEntry*>(o.d_table);
    a.sample_bytes = uint64_t(o.c) * o.ow * o.oh * es, a.plane_bytes = chw ? uint64_t(o.ow) * o.oh * es : 0;
    a.ow = o.ow, a.oh = o.oh;
    a.planes = chw ? o.c : 1u, a.cstride = chw ? 1u : o.c;
    a.cpiece = a.cstride * es <= kOrientPieceBytes ? a.cstride : kOrientPieceBytes / es;
    a.pieces = (a.cstride + a.cpiece - 1) / a.cpiece;
    a.rows = orient_tile_rows(a.cpiece * es);
    const uint64_t tiles = orient_grid_tiles(o.code_set, o.ow, o.oh, a.rows), layers = uint64_t(a.planes) * a.pieces;
    if (!tiles || !o.n_entries) return hipSuccess;  // (samples of one column under a mirror: nothing moves)
    if (tiles > 0x7FFFFFFFu || layers > 65535u || o.n_entries > 65535u) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(tiles), uint32_t(layers), o.n_entries);
    switch (es) {
        case 1: k_orient<1><<<grid, kOrientThreads, 0, stream>>>(a); break;
        case 2: k_orient<2><<<grid, kOrientThreads, 0, stream>>>(a); break;
        case 4: k_orient<4><<<grid, kOrientThreads, 0, stream>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llcomp_mi
