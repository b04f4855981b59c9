// paste_kernels.hip -- the batch copy-paste on the GPU, for the four widths of id map (include/llcomp_mi.h: "Batch copy-paste", "Batch
// copy-paste by 16-bit ids", "Wide id maps"; DESIGN.md under the same names): the pieces of a src batch that an id map selects into a dst batch, in
// place, in ONE kernel with no scratch in device memory.  The rule, the mask fetch and what a thread does with one unit (paste_decide,
// paste_finish) are paste_rule.hpp's, on top of the composition's tiles, units and shifted copy (compose_rule.hpp) -- the functions the
// host check walks without a GPU; the table is paste_plan.hpp's.
//
// A workgroup owns one tile of one plane of one dst sample (blockIdx.z: an entry of the table's samples).  Its first wavefront filters
// the sample's pieces against the tile into a short list in LDS, in order (a ballot and a count of the lanes below); ONE barrier; then
// every thread takes (row, unit) pairs of the tile, lanes along the row, and walks the short list from the back.  A tile whose list is
// empty ends there.  A dst sample has at most kPasteMaxPiecesPerSample pieces, which is the list's room: there is no unfiltered path.
#include "paste.hpp"

#include <hip/hip_runtime.h>

#include "batch_chunk.hpp"
#include "paste_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kPasteThreads = 256;
// LDS: the short list and its length
template <uint32_t MB>
constexpr uint32_t kPasteLdsBytes = kPasteMaxPiecesPerSample * sizeof(PasteRec<MB>) + 16;
static_assert(kPasteLdsBytes<1> == 17424 && 8 * kPasteLdsBytes<1> <= 160 * 1024 && kPasteMaxPiecesPerSample % 64 == 0,
              "17 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Batch copy-paste\")");
static_assert(kPasteLdsBytes<2> == 18448 && 8 * kPasteLdsBytes<2> <= 160 * 1024,
              "18 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Batch copy-paste by 16-bit ids\")");

static_assert(kPasteLdsBytes<3> == 18448 && kPasteLdsBytes<4> == 18448, "the wide masks: the 16-bit call's LDS");

template <uint32_t MB>
struct PasteArgs {
    PasteGeom pg;
    const ComposeSample* samples;
    const PasteRec<MB>* recs;
};

template <uint32_t MB, uint32_t ES>
__global__ __launch_bounds__(kPasteThreads) void k_paste(PasteArgs<MB> a) {
    __shared__ __attribute__((aligned(16))) PasteRec<MB> list[kPasteMaxPiecesPerSample];
    __shared__ uint32_t n_list;
    const PasteGeom& pg = a.pg;
    const ComposeSample sm = a.samples[blockIdx.z];
    const ComposeTileBox box = compose_tile_box(pg.g, ES, blockIdx.x);
    const PasteRec<MB>* recs = a.recs + sm.first;
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
                for (uint32_t w = 0; w < sizeof(PasteRec<MB>) / 4; ++w) to[w] = from[w];
            }
            kept += __popcll(mask);
        }
        if (threadIdx.x == 0) n_list = kept;
    }
    __syncthreads();
    PasteWork<MB> k;
    k.list = list, k.n_list = n_list, k.d = sm.dst, k.pl = blockIdx.y;
    if (!k.n_list) return;
    DeviceMem mem;  // (batch_chunk.hpp: global memory as it is)
    paste_tile_pass<MB, ES>(pg, k, box, threadIdx.x, kPasteThreads, mem);
}

template <uint32_t MB>
hipError_t launch_width(const PasteLaunch& o, hipStream_t stream) {
    const uint32_t es = batch_esize(o.dtype);
    const PasteTable<MB> t(o.n_samples, o.n_recs);
    PasteArgs<MB> a{};
    a.pg = paste_geom<MB>(reinterpret_cast<uintptr_t>(o.d_dst), reinterpret_cast<uintptr_t>(o.d_src), reinterpret_cast<uintptr_t>(o.d_mask), o.n_src, o.iw,
                      o.ih, o.ow, o.oh, o.c, es, o.layout == LLCOMP_MI_LAYOUT_CHW);
    a.samples = reinterpret_cast<const ComposeSample*>(o.d_table + t.samples_at);
    a.recs = reinterpret_cast<const PasteRec<MB>*>(o.d_table + t.recs_at);
    const uint64_t tiles = uint64_t(a.pg.g.tiles_x) * a.pg.g.tiles_y;
    if (!o.n_samples) return hipSuccess;
    if (tiles > 0x7FFFFFFFu || a.pg.g.planes > 65535u || o.n_samples > 65535u) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(tiles), a.pg.g.planes, o.n_samples);
    switch (es) {
        case 1: k_paste<MB, 1><<<grid, kPasteThreads, 0, stream>>>(a); break;
        case 2: k_paste<MB, 2><<<grid, kPasteThreads, 0, stream>>>(a); break;
        case 4: k_paste<MB, 4><<<grid, kPasteThreads, 0, stream>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_paste(const PasteLaunch& o, uint32_t mask_bytes, hipStream_t stream) {
    return mask_bytes == 1 ? launch_width<1>(o, stream) : mask_bytes == 2 ? launch_width<2>(o, stream) : mask_bytes == 3 ? launch_width<3>(o, stream)
           : mask_bytes == 4 ? launch_width<4>(o, stream) : hipErrorInvalidValue;
}

}  // namespace llcomp_mi
