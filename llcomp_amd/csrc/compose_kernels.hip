// compose_kernels.hip -- the batch composition on the GPU (include/llcomp_mi.h: "Batch composition"; DESIGN.md "Batch composition"):
// rectangles of a src batch into a dst batch, the rest a fill or kept, in ONE kernel with no scratch in device memory.  The rule, the
// address functions, the units a tile owns and what a thread does with one unit (compose_decide, compose_finish: the shifted copy) are compose_rule.hpp's,
// the functions the host check walks without a GPU; the table is compose_plan.hpp's, the 16-byte chunk batch_chunk.hpp's.
//
// A workgroup owns one tile of one plane of one dst sample (blockIdx.z: an entry of the table's samples, so the sample and its run of
// pieces are the same in every thread and the records are read through uniform addresses).  Its first wavefront filters the sample's
// pieces against the tile into a short list in LDS, in order (a ballot and a count of the lanes below: no atomics, no second barrier),
// while the other threads build the fill patterns; ONE barrier; then every thread takes (row, unit) pairs of the tile, lanes along the
// row, and resolves each against the short list from the back.  Under KEEP a tile whose list is empty ends there.  The short list has
// room for kComposeListCap pieces: a dst sample with more of them (up to the cap of the call, kComposeMaxPiecesPerSample) is not
// filtered, its threads resolve against the sample's whole run in the table -- right, and slower.
#include "compose.hpp"

#include <hip/hip_runtime.h>

#include "batch_chunk.hpp"
#include "compose_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kComposeThreads = 256;
// LDS: the short list, the fill patterns and the list's length
constexpr uint32_t kComposeLdsBytes = kComposeListCap * sizeof(ComposeRec) + kComposePatterns * sizeof(ComposeChunk) + 16;
static_assert(kComposeLdsBytes == 8720 && 8 * kComposeLdsBytes <= 160 * 1024 && kComposeListCap % 64 == 0,
              "8.5 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Batch composition\")");

struct ComposeArgs {
    ComposeGeom g;
    const ComposeSample* samples;
    const ComposeRec* recs;
    const uint32_t* fill;
};

// the memory of compose_rule.hpp's functions: global memory as it is (batch_chunk.hpp: DeviceMem), with the element's size bound --
// the rule's load_el / store_el name no size, and its host check's memory is written to that
template <uint32_t ES>
struct ComposeMem : DeviceMem {
    __device__ __forceinline__ uint32_t load_el(uint64_t a) const { return DeviceMem::load_el<ES>(a); }
    __device__ __forceinline__ void store_el(uint64_t a, uint32_t bits) const { DeviceMem::store_el<ES>(a, bits); }
};

template <uint32_t ES>
__global__ __launch_bounds__(kComposeThreads) void k_compose(ComposeArgs a) {
    __shared__ __attribute__((aligned(16))) ComposeRec list[kComposeListCap];
    __shared__ __attribute__((aligned(16))) ComposeChunk patterns[kComposePatterns];
    __shared__ uint32_t n_list;
    const ComposeGeom& g = a.g;
    const ComposeSample sm = a.samples[blockIdx.z];
    const ComposeTileBox box = compose_tile_box(g, ES, blockIdx.x);
    const uint32_t pl = blockIdx.y;
    const uint32_t cmod = g.cs;  // CHW: 1
    const uint32_t* fill = a.fill + (g.planes > 1 ? pl : 0u);
    const ComposeRec* recs = a.recs + sm.first;
    const bool filtered = sm.count <= kComposeListCap;
    if (threadIdx.x < 64) {
        uint32_t kept = 0;
        if (!filtered) kept = sm.count;
        for (uint32_t i0 = 0; filtered && i0 < sm.count; i0 += 64) {
            const uint32_t i = i0 + threadIdx.x;
            ComposeRec r{};
            bool hit = false;
            if (i < sm.count) {
                r = recs[i];
                hit = compose_hits(r, box);
            }
            const uint64_t mask = __ballot(hit);
            if (hit) list[kept + __popcll(mask & ((1ull << threadIdx.x) - 1ull))] = r;
            kept += __popcll(mask);
        }
        if (threadIdx.x == 0) n_list = kept;
    } else if (cmod <= kComposePatterns && threadIdx.x - 64 < cmod) {
        patterns[threadIdx.x - 64] = compose_pattern<ES>(fill, cmod, threadIdx.x - 64);
    }
    __syncthreads();
    ComposeWork k;
    k.list = list, k.n_list = n_list, k.fill = fill, k.cmod = cmod, k.patterns = patterns, k.d = sm.dst, k.pl = pl;
    if (!k.n_list && g.keep) return;
    k.solo = filtered && compose_solo(list, k.n_list, box);
    ComposeMem<ES> mem;
    if (filtered) {
        compose_tile_pass<ES>(g, k, box, threadIdx.x, kComposeThreads, mem);
    } else {  // (the same pass with the records in global memory)
        k.list = recs;
        compose_tile_pass<ES>(g, k, box, threadIdx.x, kComposeThreads, mem);
    }
}

}  // namespace

hipError_t launch_compose(const ComposeLaunch& o, hipStream_t stream) {
    const uint32_t es = batch_esize(o.dtype);
    const ComposeTable t(o.n_samples, o.n_recs, o.c);
    ComposeArgs a{};
    a.g = compose_geom(reinterpret_cast<uintptr_t>(o.d_dst), reinterpret_cast<uintptr_t>(o.d_src), o.n_src, o.iw, o.ih, o.ow, o.oh, o.c, es,
                       o.layout == LLCOMP_MI_LAYOUT_CHW, o.keep != 0);
    a.samples = reinterpret_cast<const ComposeSample*>(o.d_table + t.samples_at);
    a.recs = reinterpret_cast<const ComposeRec*>(o.d_table + t.recs_at);
    a.fill = reinterpret_cast<const uint32_t*>(o.d_table + t.fill_at);
    const uint64_t tiles = uint64_t(a.g.tiles_x) * a.g.tiles_y;
    if (!o.n_samples) return hipSuccess;
    if (tiles > 0x7FFFFFFFu || a.g.planes > 65535u || o.n_samples > 65535u) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(tiles), a.g.planes, o.n_samples);
    switch (es) {
        case 1: k_compose<1><<<grid, kComposeThreads, 0, stream>>>(a); break;
        case 2: k_compose<2><<<grid, kComposeThreads, 0, stream>>>(a); break;
        case 4: k_compose<4><<<grid, kComposeThreads, 0, stream>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llcomp_mi
