// update_kernels.hip -- the region update's own kernels (DESIGN.md "Region update"): paste the caller's rectangle into the decoded box,
// build the new slice table, and move every slice to its place in the new payload.  All three are copies: HBM-bound, no coding here (the
// covered slices are coded by the encoders of slice_kernels.hip on the box's sub-geometry).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "update.hpp"

namespace llcomp_mi {

__device__ __forceinline__ unsigned long long wave_inclusive_scan_u64(unsigned long long v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= uint32_t(d)) v += o;
    }
    return v;
}

// n bytes s -> d, any alignment of either, by a team of threads of which the caller is thread `tid`; the 16-byte body is dealt in
// strides: the caller takes quads first + tid, first + tid + stride, ...; the team with first == 0 also moves the head and the tail.  The destination is written in aligned 16-byte stores (up to 15
// head and 15 tail bytes one by one); the source is read in aligned 16-byte loads when it has the destination's alignment, else in 16
// bytes of whatever alignment it has.  Reads [s, s + n) and writes [d, d + n) only.
__device__ __forceinline__ void copy_span(uint8_t* d, const uint8_t* s, uint64_t n, uint32_t tid, uint64_t first, uint64_t stride) {
    const uint64_t head = min(n, uint64_t((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
    const uint64_t nq = (n - head) >> 4, tail = (n - head) & 15;
    const bool same = ((reinterpret_cast<uintptr_t>(s) + head) & 15) == 0;
    for (uint64_t q = first + tid; q < nq; q += stride) {
        uint4 v;
        if (same) v = *reinterpret_cast<const uint4*>(s + head + 16 * q);
        else __builtin_memcpy(&v, s + head + 16 * q, 16);
        *reinterpret_cast<uint4*>(d + head + 16 * q) = v;
    }
    if (first == 0) {
        if (tid < head) d[tid] = s[tid];
        if (tid < tail) d[head + 16 * nq + tid] = s[head + 16 * nq + tid];
    }
}

// One wavefront per row of the rectangle (rows are rw * c bytes, a few hundred to a few thousand): row r of frame f goes to row y0 + r
// of the frame's box, x0b bytes in.
__global__ __launch_bounds__(256) void k_paste_rect(const uint8_t* __restrict__ rect, uint8_t* __restrict__ box, uint64_t rows, uint32_t rh,
                                                    uint64_t row_bytes, uint64_t box_row_bytes, uint32_t bh, uint64_t x0b, uint32_t y0) {
    const uint64_t row = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint64_t f = row / rh, r = row - f * rh;
    copy_span(box + (f * bh + y0 + r) * box_row_bytes + x0b, rect + row * row_bytes, row_bytes, threadIdx.x & 63, 0, 64);
}

__global__ __launch_bounds__(256) void k_merge_table(const Geometry full, const Geometry sub, const RegionBox box,
                                                     const uint32_t* old_len, const uint32_t* __restrict__ sub_len, uint32_t* new_len) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= full.n_slices) return;
    const uint32_t j = region_sub_id(full, sub, box, i);
    new_len[i] = j != ~0u ? sub_len[j] : old_len[i];
}

// One workgroup per LANE GROUP of the full batch (blockIdx.y strides over 16-byte pieces when slices are big).  The slices of a lane
// group lie back to back in the old payload and in the new one, so a group without a covered slice -- nearly all of them -- is ONE run:
// group_off[g + 1] - group_off[g] bytes from the old group offset to the new one, moved by the whole workgroup.  (One workgroup per
// slice, the first form of this kernel, spent 0.87 ms on 829 440 slices of 167 bytes: profiles/update_region_kernel_stats_splice_per_slice.csv.)  A group
// that holds covered slices, or whose run would leave either payload, goes slice by slice: offsets = the group's offset + the lengths of
// the group's slices before it (one wavefront scan); a covered slice is read from the encoder's scratch, where unit u of sub-slice j lies
// at units[((group(j) * cap16 + u) << lane_shift) + lane(j)] (stream lane order, kernels.hpp).
constexpr uint32_t kSpliceThreads = 256;
__global__ __launch_bounds__(kSpliceThreads) void k_splice_slices(const Geometry full, const Geometry sub, const RegionBox box,
                                                                  const uint8_t* __restrict__ old_payload, uint64_t old_bytes,
                                                                  const uint32_t* __restrict__ old_len, const uint64_t* __restrict__ old_goff,
                                                                  const uint4* __restrict__ units, const uint32_t* __restrict__ new_len,
                                                                  const uint64_t* __restrict__ new_goff, uint8_t* __restrict__ payload,
                                                                  uint64_t payload_cap, uint32_t* status) {
    __shared__ unsigned long long s_dst[64], s_src[64];
    __shared__ uint32_t s_len[64], s_sub[64];
    const uint32_t g = blockIdx.x, base = g << full.lane_shift;
    const uint32_t cnt = min(1u << full.lane_shift, full.n_slices - base);
    const uint64_t q0 = uint64_t(blockIdx.y) * kSpliceThreads, stride = uint64_t(gridDim.y) * kSpliceThreads;
    const bool first = threadIdx.x == 0 && blockIdx.y == 0;
    const uint32_t mine = threadIdx.x < cnt ? region_sub_id(full, sub, box, base + threadIdx.x) : ~0u;
    const bool any_covered = __syncthreads_or(mine != ~0u);
    if (!any_covered) {
        const uint64_t src = old_goff[g], dst = new_goff[g], n = new_goff[g + 1] - dst;
        if (dst + n <= payload_cap && src + n <= old_bytes) {  // (no covered slice: the group's new lengths are its old ones)
            copy_span(payload + dst, old_payload + src, n, threadIdx.x, q0, stride);
            return;
        }
    }
    if (threadIdx.x < 64) {
        // (old_len is null when every slice of the batch is covered: then no old offset is ever used)
        const bool live = threadIdx.x < cnt;
        const unsigned long long nl = live ? new_len[base + threadIdx.x] : 0;
        const unsigned long long ol = live && old_len ? old_len[base + threadIdx.x] : 0;
        const unsigned long long nsum = wave_inclusive_scan_u64(nl, threadIdx.x), osum = wave_inclusive_scan_u64(ol, threadIdx.x);
        s_dst[threadIdx.x] = new_goff[g] + nsum - nl;
        s_src[threadIdx.x] = (old_len ? old_goff[g] : 0) + osum - ol;
        s_len[threadIdx.x] = uint32_t(nl);
        s_sub[threadIdx.x] = mine;
    }
    __syncthreads();
    const uint32_t cap16 = sub.slice_cap >> 4;
    for (uint32_t t = 0; t < cnt; ++t) {
        const uint64_t n = s_len[t], dst = s_dst[t];
        const uint32_t j = s_sub[t];
        if (dst + n > payload_cap) {  // the slice does not fit the caller's buffer: nothing of it is written
            if (first) atomicOr(status, kStOverflow);
            continue;
        }
        if (j == ~0u) {
            const uint64_t src = s_src[t];
            if (src + n > old_bytes) {  // the old table promises bytes the old payload does not have: nothing is read
                if (first) atomicOr(status, kStTruncated);
                continue;
            }
            copy_span(payload + dst, old_payload + src, n, threadIdx.x, q0, stride);
            continue;
        }
        if (n > sub.slice_cap) {  // (the encoder never reports more than it stored; checked all the same: the scratch is not read past a slice's units)
            if (first) atomicOr(status, kStInternal);
            continue;
        }
        const uint4* u = units + ((size_t(j >> sub.lane_shift) * cap16) << sub.lane_shift) + (j & ((1u << sub.lane_shift) - 1));
        uint8_t* d = payload + dst;
        const uint64_t nu = (n + 15) >> 4;
        for (uint64_t q = q0 + threadIdx.x; q < nu; q += stride) {
            const uint4 v = u[size_t(q) << sub.lane_shift];
            if (16 * q + 16 <= n) {
                __builtin_memcpy(d + 16 * q, &v, 16);  // (a slice's offset in the payload is arbitrary)
            } else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t k = 0; k < uint32_t(n - 16 * q); ++k) d[16 * q + k] = uint8_t(w[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

hipError_t launch_paste_rect(const uint8_t* d_rect, uint8_t* d_box, uint32_t frames, uint32_t c, uint32_t rw, uint32_t rh, uint32_t bw,
                             uint32_t bh, uint32_t x0, uint32_t y0, hipStream_t stream) {
    if (!frames || !c || !rw || !rh || uint64_t(x0) + rw > bw || uint64_t(y0) + rh > bh) return hipErrorInvalidValue;
    const uint64_t rows = uint64_t(frames) * rh, blocks = (rows + 3) / 4;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_paste_rect<<<dim3(uint32_t(blocks)), dim3(256), 0, stream>>>(d_rect, d_box, rows, rh, uint64_t(rw) * c, uint64_t(bw) * c, bh, uint64_t(x0) * c, y0);
    return hipGetLastError();
}

hipError_t launch_merge_table(const Geometry& full, const Geometry& sub, const RegionBox& box, const uint32_t* d_old_len,
                              const uint32_t* d_sub_len, uint32_t* d_new_len, hipStream_t stream) {
    k_merge_table<<<dim3((full.n_slices + 255) / 256), dim3(256), 0, stream>>>(full, sub, box, d_old_len, d_sub_len, d_new_len);
    return hipGetLastError();
}

hipError_t launch_splice_slices(const Geometry& full, const Geometry& sub, const RegionBox& box, const uint8_t* d_old_payload, uint64_t old_bytes,
                                const uint32_t* d_old_len, const uint64_t* d_old_goff, const uint8_t* d_units, const uint32_t* d_new_len,
                                const uint64_t* d_new_goff, uint8_t* d_payload, uint64_t payload_cap, uint32_t* d_status, hipStream_t stream) {
    // pieces of a slice: one workgroup moves 64 KiB in 16 rounds; bigger slices (a LEGACY stream is ONE slice) get more workgroups
    const uint32_t gy = uint32_t(std::min<uint64_t>(std::max<uint64_t>(full.slice_cap / 65536u, 1), 1024));
    k_splice_slices<<<dim3(lane_groups(full), gy), dim3(kSpliceThreads), 0, stream>>>(full, sub, box, d_old_payload, old_bytes, d_old_len, d_old_goff,
                                                                                 reinterpret_cast<const uint4*>(d_units), d_new_len, d_new_goff,
                                                                                 d_payload, payload_cap, d_status);
    return hipGetLastError();
}

}  // namespace llcomp_mi
