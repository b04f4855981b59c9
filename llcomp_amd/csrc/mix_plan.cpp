// mix_plan.cpp -- the host planner of the batch mixing (mix_plan.hpp) and llcomp_mi_mix_reference.  Plain C++, no GPU.
#include "mix_plan.hpp"

#include <algorithm>
#include <cstring>

#include "mix_rule.hpp"

namespace llcomp_mi {

int mix_check_records(uint32_t n, const llcomp_mi_mix_sample* samples) {
    if (!samples || !n || n > kBatchMaxSamples) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint8_t> taken(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const llcomp_mi_mix_sample& s = samples[i];
        if (s.partner >= n || taken[s.partner]) return LLCOMP_MI_BAD_ARGS;
        taken[s.partner] = 1;
        if (s.flags & ~LLCOMP_MI_MIX_BLEND) return LLCOMP_MI_BAD_ARGS;
        if (!mix_finite(s.w_own) || !mix_finite(s.w_partner)) return LLCOMP_MI_BAD_ARGS;
    }
    return LLCOMP_MI_OK;
}

int mix_check_call(uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_mix_sample* samples,
                   const float* erase_value, std::vector<uint32_t>& erase_bits) {
    if (int rc = batch_check_shape(n, c, ow, oh, dtype, layout)) return rc;
    if (int rc = mix_check_records(n, samples)) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const llcomp_mi_mix_sample& s = samples[i];
        if (!mix_rect_ok(s.box, ow, oh) || !mix_rect_ok(s.erase, ow, oh)) return LLCOMP_MI_BAD_ARGS;
        if ((s.flags & LLCOMP_MI_MIX_BLEND) && dtype == LLCOMP_MI_DTYPE_U8) return LLCOMP_MI_BAD_ARGS;
    }
    return batch_value_bits(dtype, c, erase_value, erase_bits);
}

void mix_plan(uint32_t n, const llcomp_mi_mix_sample* samples, MixPlan& p) {
    p = MixPlan{};
    p.order.reserve(n);
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> slot_sample;
    for (uint32_t i0 = 0; i0 < n; ++i0) {
        if (seen[i0]) continue;
        const uint32_t first = uint32_t(p.order.size());
        for (uint32_t i = i0; !seen[i]; i = samples[i].partner) {
            seen[i] = 1;
            p.order.push_back(i);
        }
        const uint32_t len = uint32_t(p.order.size()) - first, pieces = (len + kMixSegment - 1) / kMixSegment;
        const uint32_t seg0 = uint32_t(p.segs.size()), slot0 = p.n_saved;
        for (uint32_t k = 0, at = first; k < pieces; ++k) {
            const uint32_t count = len / pieces + (k < len % pieces ? 1u : 0u);
            p.segs.push_back(MixSeg{at, count, kMixNoSlot, 0});
            at += count;
        }
        if (pieces == 1) continue;
        for (uint32_t k = 0; k < pieces; ++k) {  // segment k's last sample mixes with the head of segment k + 1, the last one's with the cycle's
            p.segs[seg0 + k].tail_slot = slot0 + (k + 1) % pieces;
            slot_sample.push_back(p.order[p.segs[seg0 + k].first]);
        }
        p.n_saved += pieces;
    }
    for (uint32_t k = 0; k < p.n_saved; ++k) p.segs[k].slot_sample = slot_sample[k];
}

void mix_table_put(uint32_t n, const llcomp_mi_mix_sample* samples, const MixPlan& p, const std::vector<uint32_t>& erase_bits, uint8_t* at) {
    const MixTable t(n, p.segs.size(), uint32_t(erase_bits.size()));
    std::memcpy(at + t.recs_at, samples, size_t(n) * sizeof(llcomp_mi_mix_sample));
    std::memcpy(at + t.order_at, p.order.data(), size_t(n) * 4);
    std::memcpy(at + t.segs_at, p.segs.data(), p.segs.size() * sizeof(MixSeg));
    std::memcpy(at + t.erase_at, erase_bits.data(), erase_bits.size() * 4);
}

namespace {

inline uint32_t get_el(const uint8_t* p, uint64_t e, uint32_t esize) {
    uint32_t v = 0;
    std::memcpy(&v, p + e * esize, esize);  // (little-endian hosts, like the containers)
    return v;
}
inline void put_el(uint8_t* p, uint64_t e, uint32_t esize, uint32_t v) { std::memcpy(p + e * esize, &v, esize); }

template <uint32_t DT, bool CHW>
void reference_body(const uint8_t* src, uint8_t* out, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, const llcomp_mi_mix_sample* samples,
                    const uint32_t* ev) {
    const uint32_t esize = batch_esize(DT);
    const uint64_t el = uint64_t(c) * ow * oh;
    for (uint32_t i = 0; i < n; ++i) {
        const llcomp_mi_mix_sample& s = samples[i];
        const llcomp_mi_mix_sample& sp = samples[s.partner];
        const MixWhat what = mix_what(s, i);
        const uint8_t* own = src + uint64_t(i) * el * esize;
        const uint8_t* partner = src + uint64_t(s.partner) * el * esize;
        uint8_t* o = out + uint64_t(i) * el * esize;
        MixAt at = mix_at<CHW>(0, c, ow, oh);
        for (uint64_t e = 0; e < el; ++e, at = mix_next<CHW>(at, c, ow, oh))
            put_el(o, e, esize,
                   mix_element<DT>(what, s.w_own, s.w_partner, get_el(own, e, esize), get_el(partner, e, esize), ev[at.ch],
                                   mix_in_rect(s.erase, at.x, at.y), mix_in_rect(sp.erase, at.x, at.y), mix_in_rect(s.box, at.x, at.y)));
    }
}

}  // namespace

int mix_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                  const llcomp_mi_mix_sample* samples, const float* erase_value, void* out) {
    if (!batch || !out) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> ev;
    if (int rc = mix_check_call(n, c, ow, oh, dtype, layout, samples, erase_value, ev)) return rc;
    const uint8_t* src = static_cast<const uint8_t*>(batch);
    std::vector<uint8_t> before;
    if (out == batch) {  // every sample from the batch as it stands before the call: a copy of it
        const uint64_t bytes = uint64_t(n) * c * ow * oh * batch_esize(dtype);
        before.assign(src, src + size_t(bytes));
        src = before.data();
    }
    uint8_t* o = static_cast<uint8_t*>(out);
    batch_dispatch(dtype, layout == LLCOMP_MI_LAYOUT_CHW, [&](auto dt, auto chw) {
        reference_body<decltype(dt)::value, decltype(chw)::value>(src, o, n, c, ow, oh, samples, ev.data());
    });
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_mix_segment(void) { return llcomp_mi::kMixSegment; }

int llcomp_mi_mix_plan(uint32_t n, const llcomp_mi_mix_sample* samples, uint32_t* order, uint32_t* seg_first, uint32_t* n_segments,
                       uint32_t* n_saved) {
    if (!n_segments || !n_saved) return LLCOMP_MI_BAD_ARGS;
    if (int rc = llcomp_mi::mix_check_records(n, samples)) return rc;
    llcomp_mi::MixPlan p;
    llcomp_mi::mix_plan(n, samples, p);
    if (order) std::memcpy(order, p.order.data(), size_t(n) * 4);
    if (seg_first) {
        for (size_t s = 0; s < p.segs.size(); ++s) seg_first[s] = p.segs[s].first;
        seg_first[p.segs.size()] = n;
    }
    *n_segments = uint32_t(p.segs.size());
    *n_saved = p.n_saved;
    return LLCOMP_MI_OK;
}

int llcomp_mi_mix_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                            const llcomp_mi_mix_sample* samples, const float* erase_value, void* out) {
    return llcomp_mi::mix_reference(batch, n, c, ow, oh, dtype, layout, samples, erase_value, out);
}

}  // extern "C"
