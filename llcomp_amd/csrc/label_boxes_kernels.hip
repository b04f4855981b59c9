// label_boxes_kernels.hip -- the label boxes on the GPU (include/llcomp_mi.h: "Label boxes"; DESIGN.md "Label boxes"): the pixel count
// and the bounding box of each of the 256 ids of every id map of a batch.  The identity, the run update and what a thread does with one
// 16-byte unit of map memory are label_boxes_rule.hpp's, the functions llcomp_mi_label_boxes_reference walks on the host.
//
// k_label_boxes_init writes the identities.  k_label_boxes: a workgroup owns a band of kLabelBoxRows rows of one sample, keeps the 256
// records of the band in LDS (five arrays of 256 words), and its threads take the band's aligned 16-byte units, lanes along memory: a
// unit's runs of equal bytes update the records with LDS atomics; ONE barrier behind them; then thread m merges record m, if the band
// has a pixel of it, into the output with atomicAdd, atomicMin and atomicMax on uint32_t.  All of it is integer arithmetic: the result
// does not depend on the order of the updates.
#include "label_boxes.hpp"

#include <hip/hip_runtime.h>

#include "label_boxes_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kLabelThreads = 256;
constexpr uint32_t kLabelLdsBytes = 5 * kLabelIds * 4;
static_assert(kLabelLdsBytes == 5120 && kLabelThreads == kLabelIds && 8 * kLabelLdsBytes <= 160 * 1024,
              "5 KiB of LDS: eight workgroups, all 32 wavefronts, to a CU as far as LDS goes; a thread per record (DESIGN.md \"Label boxes\")");

struct LabelDeviceMem {
    __device__ __forceinline__ LabelChunk load16(uint64_t a) const {
        typedef uint32_t V4 __attribute__((ext_vector_type(4)));
        const V4 v = *reinterpret_cast<const V4*>(__builtin_assume_aligned(reinterpret_cast<const void*>(a), 16));
        return LabelChunk{{v[0], v[1], v[2], v[3]}};
    }
    template <uint32_t N>
    __device__ __forceinline__ uint32_t load_el(uint64_t a) const {
        return *reinterpret_cast<const uint8_t*>(a);
    }
};
// the band's records in LDS
struct LdsSink {
    uint32_t *count, *x0, *y0, *x1, *y1;
    __device__ __forceinline__ void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        atomicAdd(&count[id], length);
        atomicMin(&x0[id], x_first);
        atomicMax(&x1[id], x_end);
        atomicMin(&y0[id], y);
        atomicMax(&y1[id], y + 1);
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
    label_band(g, blockIdx.y, blockIdx.x, sample, lo, hi);
    LabelDeviceMem mem;
    LdsSink sink{count, x0, y0, x1, y1};
    for (uint64_t u = (lo & ~uint64_t(15)) + 16 * uint64_t(t); u < hi; u += 16 * uint64_t(kLabelThreads)) label_boxes_unit(g, sample, lo, hi, u, mem, sink);
    __syncthreads();
    if (!count[t]) return;
    llcomp_mi_label_box* b = boxes + uint64_t(blockIdx.y) * kLabelIds + t;
    atomicAdd(&b->count, count[t]);
    atomicMin(&b->x0, x0[t]);
    atomicMin(&b->y0, y0[t]);
    atomicMax(&b->x1, x1[t]);
    atomicMax(&b->y1, y1[t]);
}

}  // namespace

hipError_t launch_label_boxes(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, uint8_t* d_boxes, hipStream_t stream) {
    const LabelGeom g = label_geom(reinterpret_cast<uintptr_t>(d_maps), n, ow, oh);
    llcomp_mi_label_box* boxes = reinterpret_cast<llcomp_mi_label_box*>(d_boxes);
    const uint32_t n_recs = n * kLabelIds;  // (n <= 65535)
    if (g.bands > 0x7FFFFFFFu || n > 65535u) return hipErrorInvalidValue;
    k_label_boxes_init<<<(n_recs + kLabelThreads - 1) / kLabelThreads, kLabelThreads, 0, stream>>>(boxes, n_recs, ow, oh);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    k_label_boxes<<<dim3(g.bands, n), kLabelThreads, 0, stream>>>(g, boxes);
    return hipGetLastError();
}

}  // namespace llcomp_mi
