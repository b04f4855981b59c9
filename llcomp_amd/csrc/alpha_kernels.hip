// alpha_kernels.hip -- the batch alpha paste on the GPU (include/llcomp_mi.h and DESIGN.md: "Batch alpha paste"): the pieces of a src
// batch blended into a dst batch under a per-pixel alpha byte, in place, in ONE kernel with no scratch in device memory.  The two rules,
// the alpha fetch and what a thread does with one unit (alpha_decide, alpha_finish) are alpha_rule.hpp's, on top of the composition's
// tiles, units and shifted copy (compose_rule.hpp) and the copy-paste's mask units (paste_rule.hpp) -- the functions the host check
// walks without a GPU; the table is alpha_plan.hpp's.
//
// The grid and the short list are k_paste's: a workgroup owns one tile of one plane of one dst sample (blockIdx.z: an entry of the
// table's samples); its first wavefront filters the sample's pieces against the tile into a short list in LDS, in order; the other
// threads copy the 256 weights there meanwhile; ONE barrier; then every thread takes (row, unit) pairs of the tile, lanes along the
// row, reads its unit of dst once, walks the short list FORWARDS and stores the unit once.  A tile whose list is empty ends there.
// OVER pieces are for U8 only and carry a 32-bit division per pixel: calls with one run k_alpha_paste<AB, U8, true>, the others an
// instantiation without the branch.
#include "alpha.hpp"

#include <hip/hip_runtime.h>

#include "alpha_rule.hpp"
#include "batch_chunk.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kAlphaThreads = 256;
// LDS the kernel declares: the short list, the weights and the list's length, 10244 bytes.  hipcc adds 12 bytes per thread to the U8
// instantiations, a private array that it keeps in LDS (13316 bytes in its own figures: DESIGN.md "Batch alpha paste"); eight
// workgroups to a CU fit either way.
constexpr uint32_t kAlphaLdsBytes = kPasteMaxPiecesPerSample * sizeof(AlphaRec) + 256 * sizeof(float) + sizeof(uint32_t);
static_assert(kAlphaLdsBytes == 10244 && 8 * (kAlphaLdsBytes + 12 * kAlphaThreads) <= 160 * 1024 && kPasteMaxPiecesPerSample % 64 == 0,
              "the list, the weights and the compiler's 12 bytes per thread: eight workgroups to a CU as far as LDS goes");

// the rule's weights, divided by the compiler
__device__ __constant__ AlphaWeights d_alpha_weights = alpha_weights();

struct AlphaArgs {
    AlphaGeom ag;
    const ComposeSample* samples;
    const AlphaRec* recs;
};

template <uint32_t AB, uint32_t DT, bool OVER>
__global__ __launch_bounds__(kAlphaThreads) void k_alpha_paste(AlphaArgs a) {
    constexpr uint32_t ES = batch_esize(DT);
    __shared__ __attribute__((aligned(16))) AlphaRec list[kPasteMaxPiecesPerSample];
    __shared__ float weights[256];
    __shared__ uint32_t n_list;
    const AlphaGeom& ag = a.ag;
    const ComposeSample sm = a.samples[blockIdx.z];
    const ComposeTileBox box = compose_tile_box(ag.pg.g, ES, blockIdx.x);
    const AlphaRec* recs = a.recs + sm.first;
    const uint32_t count = sm.count < kPasteMaxPiecesPerSample ? sm.count : kPasteMaxPiecesPerSample;  // (the checks keep it there)
    if constexpr (DT != LLCOMP_MI_DTYPE_U8) weights[threadIdx.x] = d_alpha_weights.w[threadIdx.x];
    if (threadIdx.x < 64) {
        uint32_t kept = 0;
        for (uint32_t i0 = 0; i0 < count; i0 += 64) {
            const uint32_t i = i0 + threadIdx.x;
            bool hit = false;
            if (i < count) hit = compose_hits(recs[i].r, box);
            const uint64_t mask = __ballot(hit);
            if (hit) {
                const uint32_t* from = reinterpret_cast<const uint32_t*>(recs + i);
                uint32_t* to = reinterpret_cast<uint32_t*>(list + kept + __popcll(mask & ((1ull << threadIdx.x) - 1ull)));
                LLMI_UNROLL
                for (uint32_t w = 0; w < sizeof(AlphaRec) / 4; ++w) to[w] = from[w];
            }
            kept += __popcll(mask);
        }
        if (threadIdx.x == 0) n_list = kept;
    }
    __syncthreads();
    AlphaWork k;
    k.list = list, k.n_list = n_list, k.d = sm.dst, k.pl = blockIdx.y, k.w = weights;
    if (!k.n_list) return;
    DeviceMem mem;  // (batch_chunk.hpp: global memory as it is)
    alpha_tile_pass<AB, DT, OVER>(ag, k, box, threadIdx.x, kAlphaThreads, mem);
}

template <uint32_t AB>
hipError_t launch_width(const AlphaLaunch& o, hipStream_t stream) {
    const uint32_t es = batch_esize(o.dtype);
    const AlphaTable t(o.n_samples, o.n_recs);
    AlphaArgs a{};
    a.ag = alpha_geom<AB>(reinterpret_cast<uintptr_t>(o.d_dst), reinterpret_cast<uintptr_t>(o.d_src), reinterpret_cast<uintptr_t>(o.d_alpha), o.alpha_byte,
                          o.n_src, o.iw, o.ih, o.n_dst, o.ow, o.oh, o.c, es, o.layout == LLCOMP_MI_LAYOUT_CHW);
    a.samples = reinterpret_cast<const ComposeSample*>(o.d_table + t.samples_at);
    a.recs = reinterpret_cast<const AlphaRec*>(o.d_table + t.recs_at);
    const ComposeGeom& g = a.ag.pg.g;
    const uint64_t tiles = uint64_t(g.tiles_x) * g.tiles_y;
    if (!o.n_samples) return hipSuccess;
    if (tiles > 0x7FFFFFFFu || g.planes > 65535u || o.n_samples > 65535u) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(tiles), g.planes, o.n_samples);
    switch (o.dtype) {
        case LLCOMP_MI_DTYPE_U8:
            if (o.over) k_alpha_paste<AB, LLCOMP_MI_DTYPE_U8, true><<<grid, kAlphaThreads, 0, stream>>>(a);
            else k_alpha_paste<AB, LLCOMP_MI_DTYPE_U8, false><<<grid, kAlphaThreads, 0, stream>>>(a);
            break;
        case LLCOMP_MI_DTYPE_F32: k_alpha_paste<AB, LLCOMP_MI_DTYPE_F32, false><<<grid, kAlphaThreads, 0, stream>>>(a); break;
        case LLCOMP_MI_DTYPE_F16: k_alpha_paste<AB, LLCOMP_MI_DTYPE_F16, false><<<grid, kAlphaThreads, 0, stream>>>(a); break;
        case LLCOMP_MI_DTYPE_BF16: k_alpha_paste<AB, LLCOMP_MI_DTYPE_BF16, false><<<grid, kAlphaThreads, 0, stream>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_alpha_paste(const AlphaLaunch& o, hipStream_t stream) {
    if (o.over && o.dtype != LLCOMP_MI_DTYPE_U8) return hipErrorInvalidValue;
    switch (o.alpha_px_bytes) {
        case 1: return launch_width<1>(o, stream);
        case 2: return launch_width<2>(o, stream);
        case 3: return launch_width<3>(o, stream);
        case 4: return launch_width<4>(o, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace llcomp_mi
