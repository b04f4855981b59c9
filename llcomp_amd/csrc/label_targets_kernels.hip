// label_targets_kernels.hip -- the label targets on the GPU (include/llcomp_mi.h: "Label targets"; DESIGN.md "Label targets"): the
// class-index tensor, the one-hot planes or the instance masks of a batch of id maps, from a small table per sample.  The check, the
// table, the look-up and what a thread does with one 16-byte unit of map memory and of output memory are label_targets_rule.hpp's, the
// functions llcomp_mi_label_targets_reference walks on the host.
//
// k_label_targets<MB, K, KIND>: a workgroup of 256 threads owns one segment of kTargetSegment pixels of one sample that gets
// workgroups and, for PLANES, one chunk of kTargetPlaneChunk of its planes -- grid (segments, samples, plane chunks).  The sample's
// table goes into LDS: for 1-byte maps a dense table of 256 values (the default, one barrier, the listed ids' values, one barrier),
// for 2-byte maps the list and its values, 6 bytes per id at capacity K (one barrier).  The threads read the segment's map pixels in
// aligned 16-byte units, lanes along memory, look every pixel up -- 2-byte maps through LabelFinder: a comparison with the thread's
// previous id, then binary search -- and leave the values in LDS: uint32_t for INDEX, the plane index as uint16_t (0xFFFF: none) for
// PLANES.  ONE barrier behind them.  Then the threads take the aligned 16-byte units of OUTPUT memory that the segment covers, in the
// index tensor or in each plane of the chunk, build each from LDS and store it with one 16-byte store; a unit covered in part gets
// exactly its own elements.  A workgroup whose chunk lies behind its sample's planes leaves before the first barrier.
// k_label_targets32<MB, K, KIND>: the same for maps of 3 or 4 bytes per pixel, the list's ids 4 bytes each (8 bytes of LDS per id).
#include "label_targets.hpp"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace llcomp_mi {
namespace {

template <uint32_t KIND>
using TargetV = std::conditional_t<KIND == LLCOMP_MI_TARGET_INDEX, uint32_t, uint16_t>;
// a workgroup's LDS: the table and the segment's values
template <uint32_t MB, uint32_t K, uint32_t KIND>
struct TargetLds {
    uint32_t vals[K];
    TargetV<KIND> v[kTargetSegment];
    uint16_t list[K];
    __device__ __forceinline__ uint16_t* ids() { return list; }
};
template <uint32_t K, uint32_t KIND>
struct TargetLds<1, K, KIND> {
    uint32_t vals[256];
    TargetV<KIND> v[kTargetSegment];
    __device__ __forceinline__ uint16_t* ids() { return nullptr; }
};
constexpr uint32_t kIndex = LLCOMP_MI_TARGET_INDEX, kPlanes = LLCOMP_MI_TARGET_PLANES, kLds = 160 * 1024;
// (derived from the arrays above, not measured; a CU holds 32 wavefronts, eight workgroups of 256 threads)
static_assert(sizeof(TargetLds<1, 256, kIndex>) == 17408 && 8 * sizeof(TargetLds<1, 256, kIndex>) <= kLds, "INDEX, 1-byte maps: 17 KiB of LDS, eight workgroups, all 32 wavefronts, to a CU");
static_assert(sizeof(TargetLds<2, 256, kIndex>) == 17920 && 8 * sizeof(TargetLds<2, 256, kIndex>) <= kLds, "INDEX, 256 ids: 17.5 KiB, eight workgroups to a CU");
static_assert(sizeof(TargetLds<2, 1024, kIndex>) == 22528 && 7 * sizeof(TargetLds<2, 1024, kIndex>) <= kLds && 8 * sizeof(TargetLds<2, 1024, kIndex>) > kLds,
              "INDEX, 1024 ids: 22 KiB, seven workgroups, 28 wavefronts, to a CU");
static_assert(sizeof(TargetLds<2, 4096, kIndex>) == 40960 && 4 * sizeof(TargetLds<2, 4096, kIndex>) <= kLds && 5 * sizeof(TargetLds<2, 4096, kIndex>) > kLds,
              "INDEX, 4096 ids: 40 KiB, four workgroups, 16 wavefronts, to a CU");
static_assert(sizeof(TargetLds<1, 256, kPlanes>) == 9216 && sizeof(TargetLds<2, 256, kPlanes>) == 9728 && sizeof(TargetLds<2, 1024, kPlanes>) == 14336 &&
                  8 * sizeof(TargetLds<2, 1024, kPlanes>) <= kLds,
              "PLANES, 1-byte maps, 256 and 1024 ids: 9, 9.5 and 14 KiB, eight workgroups to a CU");
static_assert(sizeof(TargetLds<2, 4096, kPlanes>) == 32768 && 5 * sizeof(TargetLds<2, 4096, kPlanes>) <= kLds && 6 * sizeof(TargetLds<2, 4096, kPlanes>) > kLds,
              "PLANES, 4096 ids: 32 KiB, five workgroups, 20 wavefronts, to a CU");
static_assert(kLabel16Capacities[0] == 256 && kLabel16Capacities[1] == 1024 && kLabel16Capacities[2] == 4096 && kLabel16MaxIds == 4096, "the three capacities compiled below");
static_assert(kTargetMaxPlanes < kTargetNoPlane, "a plane index fits the LDS's uint16_t");

// first[n + 1], samples[gridDim.y], plane_first[n + 1] (PLANES), values and ids: the call's table (TargetTable)
template <uint32_t MB, uint32_t K, uint32_t KIND>
__global__ __launch_bounds__(kTargetThreads) void k_label_targets(TargetGeom g, TargetParams a, const uint32_t* __restrict__ first, const uint32_t* __restrict__ samples,
                                                                   const uint32_t* __restrict__ plane_first, const int32_t* __restrict__ values,
                                                                   const uint16_t* __restrict__ ids) {
    __shared__ TargetLds<MB, K, KIND> lds;
    const uint32_t t = threadIdx.x;
    const uint32_t i = samples[blockIdx.y];
    uint32_t planes = 0, plane0 = 0, k0 = 0, k1 = 0;
    if constexpr (KIND == kPlanes) {
        plane0 = plane_first[i], planes = plane_first[i + 1] - plane0;
        planes = planes < kTargetMaxPlanes ? planes : kTargetMaxPlanes;  // (checked on the host: never more)
        k0 = blockIdx.z * kTargetPlaneChunk;
        if (k0 >= planes) return;  // (the whole workgroup, before any barrier: a sample with fewer planes than the call's most)
        k1 = planes - k0 < kTargetPlaneChunk ? planes : k0 + kTargetPlaneChunk;
    }
    const uint32_t at = first[i];
    uint32_t cnt = first[i + 1] - at;
    cnt = cnt < K ? cnt : K;  // (checked on the host: never more)
    uint32_t* vals = lds.vals;
    uint16_t* list = lds.ids();
    TargetV<KIND>* v = lds.v;
    const uint16_t* my_ids = ids + at;
    const int32_t* my_values = values + at;
    label_targets_table_thread<MB>(0u, t, a, planes, my_ids, my_values, cnt, list, vals);
    __syncthreads();
    if constexpr (MB == 1) {
        label_targets_table_thread<MB>(1u, t, a, planes, my_ids, my_values, cnt, list, vals);
        __syncthreads();
    }
    uint32_t s0, s1;
    target_segment(g, blockIdx.x, s0, s1);
    DeviceMem mem;  // (batch_chunk.hpp: global memory as it is, for the maps and for the output)
    TargetLookup<MB, const uint16_t*, const uint32_t*> look{{list, cnt}, vals, target_table_value(a.kind, a.default_value, planes)};
    label_targets_read_thread<MB>(g, i, s0, s1, t, mem, look, v);
    __syncthreads();
    const TargetV<KIND>* cv = v;
    label_targets_write_any<KIND>(g, i, s0, s1, plane0, k0, k1, t, a, cv, mem);
}

template <uint32_t MB, uint32_t K>
hipError_t launch_kind(const dim3& grid, const TargetGeom& g, const TargetParams& a, const uint32_t* first, const uint32_t* samples, const uint32_t* plane_first,
                       const int32_t* values, const uint16_t* ids, hipStream_t stream) {
    if (a.kind == kPlanes) k_label_targets<MB, K, kPlanes><<<grid, kTargetThreads, 0, stream>>>(g, a, first, samples, plane_first, values, ids);
    else k_label_targets<MB, K, kIndex><<<grid, kTargetThreads, 0, stream>>>(g, a, first, samples, plane_first, values, ids);
    return hipGetLastError();
}

// The wide id maps (include/llcomp_mi.h "Wide id maps"): MB 3 or 4, the list's ids 4 bytes each, 8 bytes of LDS per id
template <uint32_t K, uint32_t KIND>
struct TargetLds32 {
    uint32_t vals[K], list[K];
    TargetV<KIND> v[kTargetSegment];
};
static_assert(sizeof(TargetLds32<256, kIndex>) == 18432 && 8 * sizeof(TargetLds32<256, kIndex>) <= kLds, "wide INDEX, 256 ids: 18 KiB, eight workgroups to a CU");
static_assert(sizeof(TargetLds32<1024, kIndex>) == 24576 && 6 * sizeof(TargetLds32<1024, kIndex>) <= kLds && 7 * sizeof(TargetLds32<1024, kIndex>) > kLds,
              "wide INDEX, 1024 ids: 24 KiB, six workgroups, 24 wavefronts, to a CU");
static_assert(sizeof(TargetLds32<4096, kIndex>) == 49152 && 3 * sizeof(TargetLds32<4096, kIndex>) <= kLds && 4 * sizeof(TargetLds32<4096, kIndex>) > kLds,
              "wide INDEX, 4096 ids: 48 KiB, three workgroups, 12 wavefronts, to a CU");
static_assert(sizeof(TargetLds32<4096, kPlanes>) == 40960 && 4 * sizeof(TargetLds32<4096, kPlanes>) <= kLds, "wide PLANES, 4096 ids: 40 KiB, four workgroups to a CU");
static_assert(sizeof(TargetLds32<4096, kIndex>) == 4096 * kTarget32IdBytes + 4 * kTargetSegment, "8 bytes of LDS per listed id");

// k_label_targets with the phases of a 2-byte map: the list and its values (one barrier), the look-ups (one barrier), the stores
template <uint32_t MB, uint32_t K, uint32_t KIND>
__global__ __launch_bounds__(kTargetThreads) void k_label_targets32(TargetGeom g, TargetParams a, const uint32_t* __restrict__ first, const uint32_t* __restrict__ samples,
                                                                     const uint32_t* __restrict__ plane_first, const int32_t* __restrict__ values,
                                                                     const uint32_t* __restrict__ ids) {
    static_assert(MB == 3 || MB == 4, "the wide maps");
    __shared__ TargetLds32<K, KIND> lds;
    const uint32_t t = threadIdx.x;
    const uint32_t i = samples[blockIdx.y];
    uint32_t planes = 0, plane0 = 0, k0 = 0, k1 = 0;
    if constexpr (KIND == kPlanes) {
        plane0 = plane_first[i], planes = plane_first[i + 1] - plane0;
        planes = planes < kTargetMaxPlanes ? planes : kTargetMaxPlanes;  // (checked on the host: never more)
        k0 = blockIdx.z * kTargetPlaneChunk;
        if (k0 >= planes) return;  // (the whole workgroup, before any barrier)
        k1 = planes - k0 < kTargetPlaneChunk ? planes : k0 + kTargetPlaneChunk;
    }
    const uint32_t at = first[i];
    uint32_t cnt = first[i + 1] - at;
    cnt = cnt < K ? cnt : K;  // (checked on the host: never more)
    uint32_t* vals = lds.vals;
    uint32_t* list = lds.list;
    TargetV<KIND>* v = lds.v;
    label_targets_table_thread<MB>(0u, t, a, planes, ids + at, values + at, cnt, list, vals);
    __syncthreads();
    uint32_t s0, s1;
    target_segment(g, blockIdx.x, s0, s1);
    DeviceMem mem;
    TargetLookup<MB, const uint32_t*, const uint32_t*> look{label_finder32<const uint32_t*>(list, cnt), vals, target_table_value(a.kind, a.default_value, planes)};
    label_targets_read_thread<MB>(g, i, s0, s1, t, mem, look, v);
    __syncthreads();
    const TargetV<KIND>* cv = v;
    label_targets_write_any<KIND>(g, i, s0, s1, plane0, k0, k1, t, a, cv, mem);
}

template <uint32_t MB, uint32_t K>
hipError_t launch_kind32(const dim3& grid, const TargetGeom& g, const TargetParams& a, const uint32_t* first, const uint32_t* samples, const uint32_t* plane_first,
                         const int32_t* values, const uint32_t* ids, hipStream_t stream) {
    if (a.kind == kPlanes) k_label_targets32<MB, K, kPlanes><<<grid, kTargetThreads, 0, stream>>>(g, a, first, samples, plane_first, values, ids);
    else k_label_targets32<MB, K, kIndex><<<grid, kTargetThreads, 0, stream>>>(g, a, first, samples, plane_first, values, ids);
    return hipGetLastError();
}
template <uint32_t MB>
hipError_t launch_capacity32(uint32_t capacity, const dim3& grid, const TargetGeom& g, const TargetParams& a, const uint32_t* first, const uint32_t* samples,
                             const uint32_t* plane_first, const int32_t* values, const uint32_t* ids, hipStream_t stream) {
    switch (capacity) {
        case 256: return launch_kind32<MB, 256>(grid, g, a, first, samples, plane_first, values, ids, stream);
        case 1024: return launch_kind32<MB, 1024>(grid, g, a, first, samples, plane_first, values, ids, stream);
        default: return launch_kind32<MB, 4096>(grid, g, a, first, samples, plane_first, values, ids, stream);
    }
}

}  // namespace

hipError_t launch_label_targets32(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32& t, const TargetCall& c,
                                  const uint8_t* d_table, uint8_t* d_out, hipStream_t stream) {
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps);
    const TargetGeom g = target_geom(m, reinterpret_cast<uintptr_t>(d_out), n, ow, oh, t.map_bytes);
    const uint32_t chunks = target_plane_chunks(t.kind, c.most_planes);
    if (!g.segments || n > kBatchMaxSamples || !c.n_work || c.n_work > n || c.total > kLabel16MaxTotal || c.longest > kLabel16MaxIds || !chunks || chunks > 65535u ||
        (t.map_bytes != 3 && t.map_bytes != 4) || label_map32_misaligned(m, t.map_bytes) || c.esize != target_esize(t.kind, t.dtype) || !c.esize)
        return hipErrorInvalidValue;
    const bool planes = t.kind == kPlanes;
    const TargetTable tab(n, c.n_work, c.total, planes, 4);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(d_table + tab.first_at);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(d_table + tab.samples_at);
    const uint32_t* plane_first = planes ? reinterpret_cast<const uint32_t*>(d_table + tab.planes_at) : nullptr;
    const int32_t* values = reinterpret_cast<const int32_t*>(d_table + tab.values_at);
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(d_table + tab.ids_at);
    const TargetParams a{t.kind, c.esize, t.default_value, t.on_bits, t.off_bits};
    const dim3 grid(g.segments, c.n_work, chunks);
    const uint32_t capacity = label16_capacity(c.longest);
    return t.map_bytes == 3 ? launch_capacity32<3>(capacity, grid, g, a, first, samples, plane_first, values, ids, stream)
                            : launch_capacity32<4>(capacity, grid, g, a, first, samples, plane_first, values, ids, stream);
}

hipError_t launch_label_targets(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets& t, const TargetCall& c,
                                const uint8_t* d_table, uint8_t* d_out, hipStream_t stream) {
    const TargetGeom g = target_geom(reinterpret_cast<uintptr_t>(d_maps), reinterpret_cast<uintptr_t>(d_out), n, ow, oh, t.map_bytes);
    const uint32_t chunks = target_plane_chunks(t.kind, c.most_planes);
    if (!g.segments || n > kBatchMaxSamples || !c.n_work || c.n_work > n || c.total > kLabel16MaxTotal || c.longest > kLabel16MaxIds || !chunks || chunks > 65535u ||
        (t.map_bytes != 1 && t.map_bytes != 2) || c.esize != target_esize(t.kind, t.dtype) || !c.esize)
        return hipErrorInvalidValue;
    const bool planes = t.kind == kPlanes;
    const TargetTable tab(n, c.n_work, c.total, planes);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(d_table + tab.first_at);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(d_table + tab.samples_at);
    const uint32_t* plane_first = planes ? reinterpret_cast<const uint32_t*>(d_table + tab.planes_at) : nullptr;
    const int32_t* values = reinterpret_cast<const int32_t*>(d_table + tab.values_at);
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(d_table + tab.ids_at);
    const TargetParams a{t.kind, c.esize, t.default_value, t.on_bits, t.off_bits};
    const dim3 grid(g.segments, c.n_work, chunks);
    if (t.map_bytes == 1) return launch_kind<1, 256>(grid, g, a, first, samples, plane_first, values, ids, stream);
    switch (label16_capacity(c.longest)) {
        case 256: return launch_kind<2, 256>(grid, g, a, first, samples, plane_first, values, ids, stream);
        case 1024: return launch_kind<2, 1024>(grid, g, a, first, samples, plane_first, values, ids, stream);
        default: return launch_kind<2, 4096>(grid, g, a, first, samples, plane_first, values, ids, stream);
    }
}

}  // namespace llcomp_mi
