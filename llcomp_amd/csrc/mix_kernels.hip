// mix_kernels.hip -- the batch mixing on the GPU (include/llcomp_mi.h: "Batch mixing"; DESIGN.md "Batch mixing"): RandomErasing, MixUp and
// CutMix in place on a dense batch, one read and one write per element at most.  The rule is mix_rule.hpp's, the functions
// llcomp_mi_mix_reference is compiled from; what the host decides -- the segments, the saved heads, the table -- is mix_plan.hpp's; the
// 16-byte chunk is batch_chunk.hpp's.
#include "mix.hpp"

#include <hip/hip_runtime.h>

#include "batch_chunk.hpp"
#include "mix_rule.hpp"

namespace llcomp_mi {
namespace {

constexpr uint32_t kMixThreads = 256;

// The chunk at p: one 16-byte access where it is whole and aligned (vec); otherwise its elements `mask`, one by one (p itself may lie
// outside the sample: the elements outside the mask are never touched)
template <uint32_t ES>
__device__ __forceinline__ Chunk chunk_load(const uint8_t* p, bool vec, uint32_t mask) {
    constexpr uint32_t PER = 16 / ES;
    if (vec) return *reinterpret_cast<const Chunk*>(__builtin_assume_aligned(p, 16));
    Chunk v = {0u, 0u, 0u, 0u};
    const typename ElemOf<ES>::T* el = reinterpret_cast<const typename ElemOf<ES>::T*>(p);
#pragma unroll
    for (uint32_t e = 0; e < PER; ++e)
        if ((mask >> e) & 1u) chunk_set<ES>(v, e, el[e]);
    return v;
}
// ... and the elements `mask` of v to it: in one access where that is all of an aligned chunk
template <uint32_t ES>
__device__ __forceinline__ void chunk_store(uint8_t* p, const Chunk& v, bool vec, uint32_t mask) {
    constexpr uint32_t PER = 16 / ES, ALL = PER == 16 ? 0xFFFFu : (1u << PER) - 1u;
    if (vec && mask == ALL) {
        *reinterpret_cast<Chunk*>(__builtin_assume_aligned(p, 16)) = v;
        return;
    }
    typename ElemOf<ES>::T* el = reinterpret_cast<typename ElemOf<ES>::T*>(p);
#pragma unroll
    for (uint32_t e = 0; e < PER; ++e)
        if ((mask >> e) & 1u) el[e] = typename ElemOf<ES>::T(chunk_get<ES>(v, e));
}

// The heads of the segments of cut cycles, raw, each into its slot at the sample's own offset from a multiple of 16: thread t of row
// `slot` copies the slot's 16-byte unit t -- whole where it lies inside the sample, byte by byte at the sample's two ends.
__global__ __launch_bounds__(kMixThreads) void k_mix_save(const uint8_t* __restrict__ batch, uint8_t* __restrict__ saved,
                                                         const MixSeg* __restrict__ segs, uint64_t sample_bytes, uint64_t slot_stride) {
    const uint32_t slot = blockIdx.y;
    const uint64_t unit = uint64_t(blockIdx.x) * kMixThreads + threadIdx.x;
    const uint8_t* src = batch + uint64_t(segs[slot].slot_sample) * sample_bytes;
    const uint64_t r = reinterpret_cast<uintptr_t>(src) & 15u;
    const uint64_t lo = unit * 16, hi = lo + 16;  // the unit's bytes of the slot; the sample's are [r, r + sample_bytes)
    if (lo >= r + sample_bytes) return;
    uint8_t* d = saved + uint64_t(slot) * slot_stride;
    const uint8_t* s = src - r;  // (a multiple of 16; only its bytes from r on are read)
    if (lo >= r && hi <= r + sample_bytes) {
        *reinterpret_cast<Chunk*>(__builtin_assume_aligned(d + lo, 16)) = *reinterpret_cast<const Chunk*>(__builtin_assume_aligned(s + lo, 16));
        return;
    }
    for (uint64_t b = lo < r ? r : lo; b < hi && b < r + sample_bytes; ++b) d[b] = s[b];
}

// One thread: one 16-byte chunk of the sample plane -- the same elements (ch, y, x) of every sample -- along one segment of the partner
// permutation.  It loads what a sample mixes with before it writes the sample, and that load is the next sample's own value, so every
// element is read once and written once; what a sample does not need is not loaded, what keeps its value is not written.  The chunks
// are laid so that they are 16-byte aligned in every sample where the samples' size is a multiple of 16 (vec): `lead` elements of the
// first chunk lie in front of the sample, and it and the last chunk go element by element.  Otherwise every chunk does.
template <uint32_t DT, bool CHW>
__global__ __launch_bounds__(kMixThreads) void k_mix(uint8_t* __restrict__ batch, const uint8_t* __restrict__ saved,
                                                    const llcomp_mi_mix_sample* __restrict__ recs, const uint32_t* __restrict__ order,
                                                    const MixSeg* __restrict__ segs, const uint32_t* __restrict__ erase_bits, uint64_t el,
                                                    uint64_t n_chunks, uint64_t slot_stride, uint32_t lead, uint32_t vec_ok, uint32_t c, uint32_t ow,
                                                    uint32_t oh) {
    constexpr uint32_t ES = batch_esize(DT), PER = 16 / ES, ALL = (1u << PER) - 1u;
    const uint64_t k = uint64_t(blockIdx.x) * kMixThreads + threadIdx.x;
    if (k >= n_chunks) return;
    const MixSeg seg = segs[blockIdx.y];
    const uint32_t i_head = __builtin_amdgcn_readfirstlane(order[seg.first]);
    llcomp_mi_mix_sample ri = recs[i_head];
    if (ri.partner == i_head && mix_rect_empty(ri.erase)) return;  // a sample by itself with nothing to erase: the whole row of the grid is done
    const uint64_t sample_bytes = el * ES;
    // the chunk's window of the plane: elements [v0 - lead, v0 - lead + PER), of which `valid` exist
    const uint64_t v0 = k * PER;
    const uint64_t first = v0 < lead ? 0 : v0 - lead;
    uint32_t valid = 0;
    uint32_t xs[PER], ys[PER], ev[PER];
    {
        MixAt at = mix_at<CHW>(first, c, ow, oh);
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            const bool in = v0 + e >= lead && v0 + e - lead < el;
            xs[e] = at.x, ys[e] = at.y, ev[e] = 0;
            if (in) {
                valid |= 1u << e;
                ev[e] = erase_bits[at.ch];
                at = mix_next<CHW>(at, c, ow, oh);
            }
        }
    }
    const bool vec = vec_ok && valid == ALL;
    const int64_t at_bytes = (int64_t(v0) - int64_t(lead)) * int64_t(ES);  // the chunk's offset in a sample (below 0 for the lead's chunk)
    auto rect_mask = [&](const uint32_t* r) {
        uint32_t m = 0;
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) m |= uint32_t(mix_in_rect(r, xs[e], ys[e])) << e;
        return m & valid;
    };

    const bool own_tail = seg.tail_slot == kMixNoSlot && seg.count > 1;  // the last sample mixes with the segment's own head
    Chunk cur = {0u, 0u, 0u, 0u}, head = cur;
    bool have = false, head_have = false;
    uint32_t i = i_head;
    for (uint32_t j = 0; j < seg.count; ++j) {
        const bool last = j + 1 == seg.count;
        const uint32_t p = ri.partner;
        const llcomp_mi_mix_sample rp = recs[p];
        const MixWhat what = mix_what(ri, i);
        const uint32_t me = mix_rect_empty(ri.erase) ? 0u : rect_mask(ri.erase);
        const uint32_t mb = !what.mixes || mix_rect_empty(ri.box) ? 0u : rect_mask(ri.box);
        const uint32_t mp = !what.mixes || mix_rect_empty(rp.erase) ? 0u : rect_mask(rp.erase);
        const bool blend = what.mixes && what.blend && DT != LLCOMP_MI_DTYPE_U8;
        const uint32_t written = me | mb | (blend ? valid : 0u);
        const uint32_t from_partner = what.mixes ? (mb | (blend ? valid : 0u)) & ~mp : 0u;  // the elements that read the partner's value as it stood
        const uint32_t from_own = blend ? valid & ~(me | mb) : 0u;
        uint8_t* const own_at = batch + uint64_t(i) * sample_bytes + at_bytes;
        Chunk nxt = {0u, 0u, 0u, 0u};
        bool nxt_have = false;
        if (from_partner) {
            if (!last) {
                nxt = chunk_load<ES>(batch + uint64_t(p) * sample_bytes + at_bytes, vec, valid);
            } else if (!own_tail) {  // the head of the cycle's next segment, from its slot
                const uint64_t r = reinterpret_cast<uintptr_t>(batch + uint64_t(p) * sample_bytes) & 15u;
                nxt = chunk_load<ES>(saved + uint64_t(seg.tail_slot) * slot_stride + r + at_bytes, vec, valid);
            } else {
                nxt = head_have ? head : chunk_load<ES>(batch + uint64_t(i_head) * sample_bytes + at_bytes, vec, valid);
            }
            nxt_have = !last;
        }
        if ((from_own || (j == 0 && own_tail && written)) && !have) {
            cur = chunk_load<ES>(own_at, vec, valid);
            have = true;
        }
        if (j == 0 && own_tail && written) head = cur, head_have = true;  // (what is written here is gone from the batch when the last sample asks for it)
        if (written) {
            Chunk out = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e)
                chunk_set<ES>(out, e,
                              mix_element<DT>(what, ri.w_own, ri.w_partner, chunk_get<ES>(cur, e), chunk_get<ES>(nxt, e), ev[e], (me >> e) & 1u,
                                              (mp >> e) & 1u, (mb >> e) & 1u));
            chunk_store<ES>(own_at, out, vec, written);
        }
        cur = nxt, have = nxt_have;
        i = p, ri = rp;
    }
}

template <uint32_t DT, bool CHW>
hipError_t launch_one(const MixLaunch& m, hipStream_t stream) {
    constexpr uint32_t es = batch_esize(DT), per = 16 / es;
    const uint64_t el = uint64_t(m.c) * m.ow * m.oh, sample_bytes = el * es;
    const MixTable t(m.n, m.n_segments, m.c);
    const MixSeg* segs = reinterpret_cast<const MixSeg*>(m.d_table + t.segs_at);
    const uint64_t stride = mix_slot_stride(sample_bytes);
    if (m.n_saved) {
        const uint64_t units = stride / 16;
        k_mix_save<<<dim3(uint32_t((units + kMixThreads - 1) / kMixThreads), m.n_saved), kMixThreads, 0, stream>>>(m.d_batch, m.d_saved, segs,
                                                                                                                    sample_bytes, stride);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const bool vec_ok = sample_bytes % 16 == 0;
    const uint32_t lead = vec_ok ? uint32_t((reinterpret_cast<uintptr_t>(m.d_batch) & 15u) / es) : 0u;
    const uint64_t n_chunks = (lead + el + per - 1) / per;
    if ((n_chunks + kMixThreads - 1) / kMixThreads > 0x7FFFFFFFu) return hipErrorInvalidValue;
    k_mix<DT, CHW><<<dim3(uint32_t((n_chunks + kMixThreads - 1) / kMixThreads), m.n_segments), kMixThreads, 0, stream>>>(
        m.d_batch, m.d_saved, reinterpret_cast<const llcomp_mi_mix_sample*>(m.d_table + t.recs_at),
        reinterpret_cast<const uint32_t*>(m.d_table + t.order_at), segs, reinterpret_cast<const uint32_t*>(m.d_table + t.erase_at), el, n_chunks,
        stride, lead, vec_ok ? 1u : 0u, m.c, m.ow, m.oh);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mix(const MixLaunch& m, hipStream_t stream) {
    hipError_t e = hipErrorInvalidValue;
    batch_dispatch(m.dtype, m.layout == LLCOMP_MI_LAYOUT_CHW,
                   [&](auto dt, auto chw) { e = launch_one<decltype(dt)::value, decltype(chw)::value>(m, stream); });
    return e;
}

}  // namespace llcomp_mi
