// label_boxes_kernels.hip -- the label boxes on the GPU, both calls (include/llcomp_mi.h: "Label boxes", "Label boxes of listed ids";
// DESIGN.md under the same names): the pixel count and the bounding box of each of the 256 ids of every 8-bit id map of a batch, or of
// every id that the caller lists for a sample of 16-bit id maps.  The identity, the run update and what a thread does with one 16-byte
// unit of map memory are label_boxes_rule.hpp's, the check, the table and the search of a list label_lists.hpp's -- the functions the
// references walk on the host.
//
// k_label_boxes_init writes the identities of a call's records.  Then a workgroup owns a band of kLabelBoxRows rows of one sample and
// keeps the band's records in LDS, five words each; its threads take the band's aligned 16-byte units, lanes along memory: a unit's
// runs of equal ids update the records with LDS atomics; ONE barrier behind them; then thread t merges the records t, t + 256, ...
// that have a pixel into the output with atomicAdd, atomicMin and atomicMax on uint32_t.  All of it is integer arithmetic: the result
// does not depend on the order of the updates.  What differs is how an id finds its record:
//   k_label_boxes       the id IS the record's index: 256 records, a thread per record
//   k_label_boxes16<K>  of one LISTED sample: the sample's id list is in LDS too (22 bytes per id, K ids), and a run's id is looked up
//                       in it -- behind a comparison with the id of the thread's previous run; an id that is not listed updates nothing
//   k_label_boxes32<MB, K>  the same of maps of MB = 3 or 4 bytes per pixel (include/llcomp_mi.h "Wide id maps"): the list's ids
//                       are 4 bytes, 24 bytes of LDS per id; a 3-byte pixel belongs to the unit that holds its first byte
#include "label_boxes.hpp"

#include <hip/hip_runtime.h>

#include "label_boxes_rule.hpp"
#include "label_lists.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kLabelLdsBytes = 5 * kLabelIds * 4;
static_assert(kLabelLdsBytes == 5120 && kLabelThreads == kLabelIds && 8 * kLabelLdsBytes <= 160 * 1024,
              "5 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes; a thread per record (DESIGN.md \"Label boxes\")");
template <uint32_t K>
constexpr uint32_t label16_lds_bytes() { return K * kLabel16IdBytes; }
static_assert(label16_lds_bytes<256>() == 5632 && 8 * label16_lds_bytes<256>() <= 160 * 1024,
              "5.5 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Label boxes of listed ids\")");
static_assert(label16_lds_bytes<1024>() == 22528 && 7 * label16_lds_bytes<1024>() <= 160 * 1024 && 8 * label16_lds_bytes<1024>() > 160 * 1024,
              "22 KiB of LDS: seven workgroups, 28 wavefronts, to a CU");
static_assert(label16_lds_bytes<4096>() == 90112 && label16_lds_bytes<4096>() <= 160 * 1024 && 2 * label16_lds_bytes<4096>() > 160 * 1024,
              "88 KiB of LDS: ONE workgroup, 4 wavefronts, to a CU -- what bounds llcomp_mi_label_boxes16_max_ids()");
template <uint32_t K>
constexpr uint32_t label32_lds_bytes() { return K * kLabel32IdBytes; }
static_assert(label32_lds_bytes<256>() == 6144 && 8 * label32_lds_bytes<256>() <= 160 * 1024, "wide ids: 6 KiB of LDS, eight workgroups to a CU");
static_assert(label32_lds_bytes<1024>() == 24576 && 6 * label32_lds_bytes<1024>() <= 160 * 1024 && 7 * label32_lds_bytes<1024>() > 160 * 1024,
              "wide ids: 24 KiB of LDS, six workgroups, 24 wavefronts, to a CU");
static_assert(label32_lds_bytes<4096>() == 98304 && label32_lds_bytes<4096>() <= 160 * 1024 && 2 * label32_lds_bytes<4096>() > 160 * 1024,
              "wide ids: 96 KiB of LDS, still ONE workgroup to a CU at the top capacity");
static_assert(kLabel16Capacities[0] == 256 && kLabel16Capacities[1] == 1024 && kLabel16Capacities[2] == kLabel16MaxIds && kLabel16MaxIds == 4096, "the three capacities compiled below");

// the dense call's finder: the id is the slot
struct LabelIdentity {
    __device__ __forceinline__ uint32_t find(uint32_t id) const { return id; }
};
// the band's records in LDS; Finder: how an id finds its slot, or kLabel16None
template <class Finder>
struct LdsSink {
    Finder finder;
    uint32_t *count, *x0, *y0, *x1, *y1;
    __device__ __forceinline__ void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        const uint32_t j = finder.find(id);
        if (j == kLabel16None) return;
        atomicAdd(&count[j], length);
        atomicMin(&x0[j], x_first);
        atomicMax(&x1[j], x_end);
        atomicMin(&y0[j], y);
        atomicMax(&y1[j], y + 1);
    }
    // thread t's part of the merge of the band's cnt records into recs
    __device__ __forceinline__ void merge_out(uint32_t t, uint32_t cnt, llcomp_mi_label_box* recs) const {
        for (uint32_t j = t; j < cnt; j += kLabelThreads) {
            if (!count[j]) continue;
            llcomp_mi_label_box* b = recs + j;
            atomicAdd(&b->count, count[j]);
            atomicMin(&b->x0, x0[j]);
            atomicMin(&b->y0, y0[j]);
            atomicMax(&b->x1, x1[j]);
            atomicMax(&b->y1, y1[j]);
        }
    }
};

__global__ __launch_bounds__(kLabelThreads) void k_label_boxes_init(llcomp_mi_label_box* boxes, uint32_t n_recs, uint32_t ow, uint32_t oh) {
    const uint32_t i = blockIdx.x * kLabelThreads + threadIdx.x;
    if (i < n_recs) boxes[i] = label_box_identity(ow, oh);
}

__global__ __launch_bounds__(kLabelThreads) void k_label_boxes(LabelGeom g, llcomp_mi_label_box* boxes) {
    __shared__ uint32_t count[kLabelIds], x0[kLabelIds], y0[kLabelIds], x1[kLabelIds], y1[kLabelIds];
    const uint32_t t = threadIdx.x;
    count[t] = 0, x0[t] = g.ow, y0[t] = g.oh, x1[t] = 0, y1[t] = 0;
    __syncthreads();
    uint64_t sample, lo, hi;
    label_band<1>(g, blockIdx.y, blockIdx.x, sample, lo, hi);
    DeviceMem mem;  // (batch_chunk.hpp: global memory as it is)
    LdsSink<LabelIdentity> sink{{}, count, x0, y0, x1, y1};
    label_boxes_thread<1>(g, sample, lo, hi, t, mem, sink);
    __syncthreads();
    sink.merge_out(t, kLabelIds, boxes + uint64_t(blockIdx.y) * kLabelIds);
}

// first[n + 1], samples[gridDim.y] and ids: the call's table (Label16Table)
template <uint32_t K>
__global__ __launch_bounds__(kLabelThreads) void k_label_boxes16(LabelGeom g, const uint32_t* __restrict__ first, const uint32_t* __restrict__ samples,
                                                                  const uint16_t* __restrict__ ids, llcomp_mi_label_box* boxes) {
    __shared__ uint32_t count[K], x0[K], y0[K], x1[K], y1[K];
    __shared__ uint16_t list[K];
    const uint32_t t = threadIdx.x;
    const uint32_t i = samples[blockIdx.y];
    const uint32_t at = first[i];
    uint32_t cnt = first[i + 1] - at;
    cnt = cnt < K ? cnt : K;  // (checked on the host: never more)
    for (uint32_t j = t; j < cnt; j += kLabelThreads) list[j] = ids[at + j], count[j] = 0, x0[j] = g.ow, y0[j] = g.oh, x1[j] = 0, y1[j] = 0;
    __syncthreads();
    uint64_t sample, lo, hi;
    label_band<2>(g, i, blockIdx.x, sample, lo, hi);
    DeviceMem mem;
    LdsSink<LabelFinder<const uint16_t*>> sink{{list, cnt}, count, x0, y0, x1, y1};
    label_boxes_thread<2>(g, sample, lo, hi, t, mem, sink);
    __syncthreads();
    sink.merge_out(t, cnt, boxes + at);
}

// ... of maps of MB = 3 or 4 bytes per pixel, the table's ids 4 bytes each
template <uint32_t MB, uint32_t K>
__global__ __launch_bounds__(kLabelThreads) void k_label_boxes32(LabelGeom g, const uint32_t* __restrict__ first, const uint32_t* __restrict__ samples,
                                                                  const uint32_t* __restrict__ ids, llcomp_mi_label_box* boxes) {
    __shared__ uint32_t count[K], x0[K], y0[K], x1[K], y1[K], list[K];
    const uint32_t t = threadIdx.x;
    const uint32_t i = samples[blockIdx.y];
    const uint32_t at = first[i];
    uint32_t cnt = first[i + 1] - at;
    cnt = cnt < K ? cnt : K;  // (checked on the host: never more)
    for (uint32_t j = t; j < cnt; j += kLabelThreads) list[j] = ids[at + j], count[j] = 0, x0[j] = g.ow, y0[j] = g.oh, x1[j] = 0, y1[j] = 0;
    __syncthreads();
    uint64_t sample, lo, hi;
    label_band<MB>(g, i, blockIdx.x, sample, lo, hi);
    DeviceMem mem;
    LdsSink<LabelFinder<const uint32_t*>> sink{label_finder32<const uint32_t*>(list, cnt), count, x0, y0, x1, y1};
    label_boxes_thread<MB>(g, sample, lo, hi, t, mem, sink);
    __syncthreads();
    sink.merge_out(t, cnt, boxes + at);
}
template <uint32_t MB>
void launch_boxes32(uint32_t capacity, const dim3& grid, const LabelGeom& g, const uint32_t* first, const uint32_t* samples, const uint32_t* ids,
                    llcomp_mi_label_box* boxes, hipStream_t stream) {
    switch (capacity) {
        case 256: k_label_boxes32<MB, 256><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
        case 1024: k_label_boxes32<MB, 1024><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
        default: k_label_boxes32<MB, 4096><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
    }
}

}  // namespace

hipError_t launch_label_boxes(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, uint8_t* d_boxes, hipStream_t stream) {
    const LabelGeom g = label_geom<1>(reinterpret_cast<uintptr_t>(d_maps), n, ow, oh);
    llcomp_mi_label_box* boxes = reinterpret_cast<llcomp_mi_label_box*>(d_boxes);
    const uint32_t n_recs = n * kLabelIds;  // (n <= 65535)
    if (g.bands > 0x7FFFFFFFu || n > 65535u) return hipErrorInvalidValue;
    k_label_boxes_init<<<(n_recs + kLabelThreads - 1) / kLabelThreads, kLabelThreads, 0, stream>>>(boxes, n_recs, ow, oh);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_label_boxes<<<dim3(g.bands, n), kLabelThreads, 0, stream>>>(g, boxes);
    return hipGetLastError();
}

hipError_t launch_label_boxes16(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const uint8_t* d_table, uint32_t n_listed, uint32_t total,
                                uint32_t longest, uint8_t* d_boxes, hipStream_t stream) {
    const LabelGeom g = label_geom<2>(reinterpret_cast<uintptr_t>(d_maps), n, ow, oh);
    llcomp_mi_label_box* boxes = reinterpret_cast<llcomp_mi_label_box*>(d_boxes);
    if (g.bands > 0x7FFFFFFFu || n > 65535u || n_listed > n || !n_listed || !total || total > kLabel16MaxTotal || longest > kLabel16MaxIds) return hipErrorInvalidValue;
    const Label16Table tab(n, n_listed, total);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(d_table + tab.first_at);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(d_table + tab.samples_at);
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(d_table + tab.ids_at);
    k_label_boxes_init<<<(total + kLabelThreads - 1) / kLabelThreads, kLabelThreads, 0, stream>>>(boxes, total, ow, oh);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 grid(g.bands, n_listed);
    switch (label16_capacity(longest)) {
        case 256: k_label_boxes16<256><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
        case 1024: k_label_boxes16<1024><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
        default: k_label_boxes16<4096><<<grid, kLabelThreads, 0, stream>>>(g, first, samples, ids, boxes); break;
    }
    return hipGetLastError();
}

hipError_t launch_label_boxes32(const uint8_t* d_maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint8_t* d_table, uint32_t n_listed,
                                uint32_t total, uint32_t longest, uint8_t* d_boxes, hipStream_t stream) {
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps);
    const LabelGeom g = map_bytes == 3 ? label_geom<3>(m, n, ow, oh) : label_geom<4>(m, n, ow, oh);
    llcomp_mi_label_box* boxes = reinterpret_cast<llcomp_mi_label_box*>(d_boxes);
    if (g.bands > 0x7FFFFFFFu || n > 65535u || n_listed > n || !n_listed || !total || total > kLabel16MaxTotal || longest > kLabel16MaxIds ||
        (map_bytes != 3 && map_bytes != 4) || label_map32_misaligned(m, map_bytes))
        return hipErrorInvalidValue;
    const Label16Table tab(n, n_listed, total, 4);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(d_table + tab.first_at);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(d_table + tab.samples_at);
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(d_table + tab.ids_at);
    k_label_boxes_init<<<(total + kLabelThreads - 1) / kLabelThreads, kLabelThreads, 0, stream>>>(boxes, total, ow, oh);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 grid(g.bands, n_listed);
    if (map_bytes == 3) launch_boxes32<3>(label16_capacity(longest), grid, g, first, samples, ids, boxes, stream);
    else launch_boxes32<4>(label16_capacity(longest), grid, g, first, samples, ids, boxes, stream);
    return hipGetLastError();
}

}  // namespace llcomp_mi
