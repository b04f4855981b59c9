// paste16_kernels.hip -- the batch copy-paste by 16-bit ids on the GPU (include/llcomp_mi.h: "Batch copy-paste by 16-bit ids"; DESIGN.md
// "Batch copy-paste by 16-bit ids"): the pieces of a src batch that a 16-bit id map selects into a dst batch, in place, in ONE kernel
// with no scratch in device memory.  The rule, the mask fetch and what a thread does with one unit (paste16_decide, paste16_finish) are
// paste16_rule.hpp's, on top of the 8-bit paste's and the composition's tiles, units and shifted copy -- the functions the host check
// walks without a GPU; the table is paste16_plan.hpp's.
//
// A workgroup owns one tile of one plane of one dst sample (blockIdx.z: an entry of the table's samples).  Its first wavefront filters
// the sample's pieces against the tile into a short list in LDS, in order (a ballot and a count of the lanes below); ONE barrier; then
// every thread takes (row, unit) pairs of the tile, lanes along the row, and walks the short list from the back.  A tile whose list is
// empty ends there.  A dst sample has at most kPasteMaxPiecesPerSample pieces, which is the list's room: there is no unfiltered path.
#include "paste16.hpp"

#include <hip/hip_runtime.h>

#include "batch_chunk.hpp"
#include "paste16_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kPaste16Threads = 256;
// LDS: the short list and its length
constexpr uint32_t kPaste16LdsBytes = kPasteMaxPiecesPerSample * sizeof(PasteRec16) + 16;
static_assert(sizeof(PasteRec16) == 72 && kPaste16LdsBytes == 18448 && 8 * kPaste16LdsBytes <= 160 * 1024 && kPasteMaxPiecesPerSample % 64 == 0,
              "18 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Batch copy-paste by 16-bit ids\")");

struct Paste16Args {
    PasteGeom pg;
    const ComposeSample* samples;
    const PasteRec16* recs;
};

// the memory of paste16_rule.hpp's functions: global memory as it is
template <uint32_t ES>
struct Paste16DeviceMem {
    using T = typename ElemOf<ES>::T;
    __device__ __forceinline__ ComposeChunk load16(uint64_t a) const {
        const Chunk v = *reinterpret_cast<const Chunk*>(__builtin_assume_aligned(reinterpret_cast<const void*>(a), 16));
        return ComposeChunk{{v[0], v[1], v[2], v[3]}};
    }
    __device__ __forceinline__ void store16(uint64_t a, const ComposeChunk& c) const {
        *reinterpret_cast<Chunk*>(__builtin_assume_aligned(reinterpret_cast<void*>(a), 16)) = Chunk{c.w[0], c.w[1], c.w[2], c.w[3]};
    }
    template <uint32_t N>
    __device__ __forceinline__ uint32_t load_el(uint64_t a) const {
        return *reinterpret_cast<const typename ElemOf<N>::T*>(a);
    }
    __device__ __forceinline__ void store_el(uint64_t a, uint32_t bits) const { *reinterpret_cast<T*>(a) = T(bits); }
};

template <uint32_t ES>
__global__ __launch_bounds__(kPaste16Threads) void k_paste16(Paste16Args a) {
    __shared__ __attribute__((aligned(16))) PasteRec16 list[kPasteMaxPiecesPerSample];
    __shared__ uint32_t n_list;
    const PasteGeom& pg = a.pg;
    const ComposeSample sm = a.samples[blockIdx.z];
    const ComposeTileBox box = compose_tile_box(pg.g, ES, blockIdx.x);
    const PasteRec16* recs = a.recs + sm.first;
    const uint32_t count = sm.count < kPasteMaxPiecesPerSample ? sm.count : kPasteMaxPiecesPerSample;  // (the checks keep it there)
    if (threadIdx.x < 64) {
        uint32_t kept = 0;
        for (uint32_t i0 = 0; i0 < count; i0 += 64) {
            const uint32_t i = i0 + threadIdx.x;
            bool hit = false;
            if (i < count) hit = compose_hits(recs[i].r, box);
            const uint64_t mask = __ballot(hit);
            if (hit) {  // (word by word: the record's id words stay out of a copy in private memory)
                const uint32_t* from = reinterpret_cast<const uint32_t*>(recs + i);
                uint32_t* to = reinterpret_cast<uint32_t*>(list + kept + __popcll(mask & ((1ull << threadIdx.x) - 1ull)));
                LLMI_UNROLL
                for (uint32_t w = 0; w < sizeof(PasteRec16) / 4; ++w) to[w] = from[w];
            }
            kept += __popcll(mask);
        }
        if (threadIdx.x == 0) n_list = kept;
    }
    __syncthreads();
    PasteWork16 k;
    k.list = list, k.n_list = n_list, k.d = sm.dst, k.pl = blockIdx.y;
    if (!k.n_list) return;
    Paste16DeviceMem<ES> mem;
    paste16_tile_pass<ES>(pg, k, box, threadIdx.x, kPaste16Threads, mem);
}

}  // namespace

hipError_t launch_paste16(const PasteLaunch& o, hipStream_t stream) {
    const uint32_t es = batch_esize(o.dtype);
    const PasteTable16 t(o.n_samples, o.n_recs);
    Paste16Args a{};
    a.pg = paste16_geom(reinterpret_cast<uintptr_t>(o.d_dst), reinterpret_cast<uintptr_t>(o.d_src), reinterpret_cast<uintptr_t>(o.d_mask), o.n_src, o.iw,
                        o.ih, o.ow, o.oh, o.c, es, o.layout == LLCOMP_MI_LAYOUT_CHW);
    a.samples = reinterpret_cast<const ComposeSample*>(o.d_table + t.samples_at);
    a.recs = reinterpret_cast<const PasteRec16*>(o.d_table + t.recs_at);
    const uint64_t tiles = uint64_t(a.pg.g.tiles_x) * a.pg.g.tiles_y;
    if (!o.n_samples) return hipSuccess;
    if (tiles > 0x7FFFFFFFu || a.pg.g.planes > 65535u || o.n_samples > 65535u) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(tiles), a.pg.g.planes, o.n_samples);
    switch (es) {
        case 1: k_paste16<1><<<grid, kPaste16Threads, 0, stream>>>(a); break;
        case 2: k_paste16<2><<<grid, kPaste16Threads, 0, stream>>>(a); break;
        case 4: k_paste16<4><<<grid, kPaste16Threads, 0, stream>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llcomp_mi
