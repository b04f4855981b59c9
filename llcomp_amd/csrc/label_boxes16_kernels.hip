// label_boxes16_kernels.hip -- the label boxes of listed ids on the GPU (include/llcomp_mi.h: "Label boxes of listed ids"; DESIGN.md
// "Label boxes of listed ids"): the pixel count and the bounding box of every id that the caller lists for a sample, in 16-bit id maps.
// The check, the table, the search and what a thread does with one 16-byte unit of map memory are label_boxes16_rule.hpp's, the
// functions llcomp_mi_label_boxes16_reference walks on the host.
//
// k_label_boxes16_init writes the identities of all first[n] records.  k_label_boxes16<K>: a workgroup owns a band of kLabelBoxRows rows
// of one LISTED sample, keeps that sample's id list and five words per listed id in LDS (22 bytes per id, K ids), and its threads take
// the band's aligned 16-byte units, 8 pixels each, lanes along memory: a unit's runs of equal ids are looked up in the list -- behind a
// comparison with the id of the thread's previous run -- and update the records with LDS atomics; an id that is not listed updates
// nothing; ONE barrier behind them; then thread t merges the records t, t + 256, ... that have a pixel into the output with atomicAdd,
// atomicMin and atomicMax on uint32_t.  All of it is integer arithmetic: the result does not depend on the order of the updates.
#include "label_boxes16.hpp"

#include <hip/hip_runtime.h>

#include "label_boxes16_rule.hpp"

namespace llcomp_mi {
namespace {

template <uint32_t K>
constexpr uint32_t label16_lds_bytes() { return K * kLabel16IdBytes; }
static_assert(label16_lds_bytes<256>() == 5632 && 8 * label16_lds_bytes<256>() <= 160 * 1024,
              "5.5 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes (DESIGN.md \"Label boxes of listed ids\")");
static_assert(label16_lds_bytes<1024>() == 22528 && 7 * label16_lds_bytes<1024>() <= 160 * 1024 && 8 * label16_lds_bytes<1024>() > 160 * 1024,
              "22 KiB of LDS: seven workgroups, 28 wavefronts, to a CU");
static_assert(label16_lds_bytes<4096>() == 90112 && label16_lds_bytes<4096>() <= 160 * 1024 && 2 * label16_lds_bytes<4096>() > 160 * 1024,
              "88 KiB of LDS: ONE workgroup, 4 wavefronts, to a CU -- what bounds llcomp_mi_label_boxes16_max_ids()");
static_assert(kLabel16Capacities[0] == 256 && kLabel16Capacities[1] == 1024 && kLabel16Capacities[2] == kLabel16MaxIds && kLabel16MaxIds == 4096, "the three capacities compiled below");

struct Label16DeviceMem {
    __device__ __forceinline__ LabelChunk load16(uint64_t a) const {
        typedef uint32_t V4 __attribute__((ext_vector_type(4)));
        const V4 v = *reinterpret_cast<const V4*>(__builtin_assume_aligned(reinterpret_cast<const void*>(a), 16));
        return LabelChunk{{v[0], v[1], v[2], v[3]}};
    }
    template <uint32_t N>
    __device__ __forceinline__ uint32_t load_el(uint64_t a) const {
        return *reinterpret_cast<const uint16_t*>(a);
    }
};
// the band's records of the listed ids in LDS
struct Lds16Sink {
    LabelFinder<const uint16_t*> finder;
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
};

__global__ __launch_bounds__(kLabel16Threads) void k_label_boxes16_init(llcomp_mi_label_box* boxes, uint32_t n_recs, uint32_t ow, uint32_t oh) {
    const uint32_t i = blockIdx.x * kLabel16Threads + threadIdx.x;
    if (i < n_recs) boxes[i] = label_box_identity(ow, oh);
}

// first[n + 1], samples[gridDim.y] and ids: the call's table (Label16Table)
template <uint32_t K>
__global__ __launch_bounds__(kLabel16Threads) void k_label_boxes16(LabelGeom16 g, const uint32_t* __restrict__ first, const uint32_t* __restrict__ samples,
                                                                    const uint16_t* __restrict__ ids, llcomp_mi_label_box* boxes) {
    __shared__ uint32_t count[K], x0[K], y0[K], x1[K], y1[K];
    __shared__ uint16_t list[K];
    const uint32_t t = threadIdx.x;
    const uint32_t i = samples[blockIdx.y];
    const uint32_t at = first[i];
    uint32_t cnt = first[i + 1] - at;
    cnt = cnt < K ? cnt : K;  // (checked on the host: never more)
    for (uint32_t j = t; j < cnt; j += kLabel16Threads) list[j] = ids[at + j], count[j] = 0, x0[j] = g.ow, y0[j] = g.oh, x1[j] = 0, y1[j] = 0;
    __syncthreads();
    uint64_t sample, lo, hi;
    label_band16(g, i, blockIdx.x, sample, lo, hi);
    Label16DeviceMem mem;
    Lds16Sink sink{{list, cnt}, count, x0, y0, x1, y1};
    label_boxes16_thread(g, sample, lo, hi, t, mem, sink);
    __syncthreads();
    for (uint32_t j = t; j < cnt; j += kLabel16Threads) {
        if (!count[j]) continue;
        llcomp_mi_label_box* b = boxes + at + j;
        atomicAdd(&b->count, count[j]);
        atomicMin(&b->x0, x0[j]);
        atomicMin(&b->y0, y0[j]);
        atomicMax(&b->x1, x1[j]);
        atomicMax(&b->y1, y1[j]);
    }
}

}  // namespace

hipError_t launch_label_boxes16(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const uint8_t* d_table, uint32_t n_listed, uint32_t total,
                                uint32_t longest, uint8_t* d_boxes, hipStream_t stream) {
    const LabelGeom16 g = label_geom16(reinterpret_cast<uintptr_t>(d_maps), n, ow, oh);
    llcomp_mi_label_box* boxes = reinterpret_cast<llcomp_mi_label_box*>(d_boxes);
    if (g.bands > 0x7FFFFFFFu || n > 65535u || n_listed > n || !n_listed || !total || total > kLabel16MaxTotal || longest > kLabel16MaxIds) return hipErrorInvalidValue;
    const Label16Table tab(n, n_listed, total);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(d_table + tab.first_at);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(d_table + tab.samples_at);
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(d_table + tab.ids_at);
    k_label_boxes16_init<<<(total + kLabel16Threads - 1) / kLabel16Threads, kLabel16Threads, 0, stream>>>(boxes, total, ow, oh);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 grid(g.bands, n_listed);
    switch (label16_capacity(longest)) {
        case 256: k_label_boxes16<256><<<grid, kLabel16Threads, 0, stream>>>(g, first, samples, ids, boxes); break;
        case 1024: k_label_boxes16<1024><<<grid, kLabel16Threads, 0, stream>>>(g, first, samples, ids, boxes); break;
        default: k_label_boxes16<4096><<<grid, kLabel16Threads, 0, stream>>>(g, first, samples, ids, boxes); break;
    }
    return hipGetLastError();
}

}  // namespace llcomp_mi
