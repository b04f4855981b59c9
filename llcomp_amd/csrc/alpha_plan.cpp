// alpha_plan.cpp -- the host half of the batch alpha paste (alpha_plan.hpp) and the reference.  Plain C++, no GPU.
#include "alpha_plan.hpp"

#include <cstring>

#include "alpha_rule.hpp"

namespace llcomp_mi {

static_assert(sizeof(llcomp_mi_alpha_piece) == 40 && sizeof(AlphaRec) == 36, "the call's pieces and the table's records");

namespace {
// A piece's own refusals: unknown flags; OVER on anything but U8 HWC with c == 4, or with VALUE; VALUE_PIXEL without VALUE or on
// anything but U8 HWC with c <= 4; value bits without VALUE, at or above the element's size, for VALUE_PIXEL at or above c
bool alpha_piece_ok(const llcomp_mi_alpha_piece& p, uint32_t dtype, uint32_t layout, uint32_t c) {
    const uint32_t es = batch_esize(dtype);
    const bool u8_hwc = dtype == LLCOMP_MI_DTYPE_U8 && layout == LLCOMP_MI_LAYOUT_HWC;
    if (p.flags & ~kAlphaFlagBits) return false;
    if (p.flags & LLCOMP_MI_ALPHA_OVER) return u8_hwc && c == 4 && p.flags == LLCOMP_MI_ALPHA_OVER && !p.value_bits;
    if (!(p.flags & LLCOMP_MI_ALPHA_VALUE)) return !p.value_bits && !(p.flags & LLCOMP_MI_ALPHA_VALUE_PIXEL);
    if (p.flags & LLCOMP_MI_ALPHA_VALUE_PIXEL) return u8_hwc && c <= 4 && (c == 4 || !(p.value_bits >> (8 * c)));
    return es >= 4 || !(p.value_bits >> (8 * es));
}
}  // namespace

int alpha_check_call(uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh,
                     uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, AlphaUses& uses) {
    if (alpha_px_bytes < 1 || alpha_px_bytes > 4 || alpha_byte >= alpha_px_bytes) return LLCOMP_MI_BAD_ARGS;
    if (int rc = paste_check_shapes(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces != nullptr, n_pieces)) return rc;
    std::vector<uint32_t> on_sample(n_dst, 0u);
    AlphaUses u{false, false, false};
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const llcomp_mi_alpha_piece& p = pieces[i];
        if (!paste_piece_fits(p, n_src, iw, ih, n_dst, ow, oh) || !alpha_piece_ok(p, dtype, layout, c)) return LLCOMP_MI_BAD_ARGS;
        if (!alpha_idle(p) && ++on_sample[p.dst] > kPasteMaxPiecesPerSample) return LLCOMP_MI_BAD_ARGS;
        u.src |= !(p.flags & LLCOMP_MI_ALPHA_VALUE), u.alpha |= !(p.flags & LLCOMP_MI_ALPHA_OVER), u.over |= (p.flags & LLCOMP_MI_ALPHA_OVER) != 0;
    }
    uses = u;
    return LLCOMP_MI_OK;
}

int alpha_check_memory(const void* src, uint64_t src_bytes, const void* alpha, uint64_t alpha_bytes, const void* dst, uint64_t dst_bytes, uint32_t esize,
                       const AlphaUses& uses) {
    const uint64_t s = reinterpret_cast<uintptr_t>(src), m = reinterpret_cast<uintptr_t>(alpha), d = reinterpret_cast<uintptr_t>(dst);
    const uint32_t align = uses.over ? 4u : esize;
    if (!dst || (d & (align - 1))) return LLCOMP_MI_BAD_ARGS;
    if ((uses.src && !src) || (uses.alpha && !alpha) || (src && (s & (align - 1)))) return LLCOMP_MI_BAD_ARGS;
    if (src && s < d + dst_bytes && d < s + src_bytes) return LLCOMP_MI_BAD_ARGS;
    if (alpha && m < d + dst_bytes && d < m + alpha_bytes) return LLCOMP_MI_BAD_ARGS;
    return LLCOMP_MI_OK;
}

void alpha_plan(uint32_t n_dst, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, PastePlan& p) {
    paste_plan_by(n_dst, pieces, n_pieces, p, [](const llcomp_mi_alpha_piece& q) { return alpha_idle(q); });
}

void alpha_table_put(const llcomp_mi_alpha_piece* pieces, const PastePlan& p, uint32_t c, uint32_t layout, uint8_t* at) {
    const uint32_t cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    const AlphaTable t(p.samples.size(), p.order.size());
    if (!p.samples.empty()) std::memcpy(at + t.samples_at, p.samples.data(), p.samples.size() * sizeof(ComposeSample));
    for (size_t j = 0; j < p.order.size(); ++j) {
        const AlphaRec r = alpha_rec(pieces[p.order[j]], cs);
        std::memcpy(at + t.recs_at + j * sizeof(r), &r, sizeof(r));
    }
}

namespace {
// the rule, element by element: every piece of the sample that covers the pixel, in order, through the kernel's own address functions
template <uint32_t AB, uint32_t DT>
void alpha_reference(const AlphaGeom& ag, uint32_t n_dst, uint32_t ow, uint32_t oh, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces) {
    constexpr uint32_t ES = batch_esize(DT);
    const ComposeGeom& g = ag.pg.g;
    PlainMem mem;
    for (uint32_t d = 0; d < n_dst; ++d)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t y = 0; y < oh; ++y) {
                const uint64_t row = compose_dst_row(g, ES, d, pl, y);
                for (uint32_t x = 0; x < ow; ++x)
                    for (uint32_t i = 0; i < n_pieces; ++i) {
                        const llcomp_mi_alpha_piece& p = pieces[i];
                        if (p.dst != d || !alpha_covers(p, x, y)) continue;
                        const uint32_t sy = p.sy + (y - p.dy), sx = p.sx + (x - p.dx);
                        const uint64_t s = compose_src_row(g, ES, p.src, pl, sy) + uint64_t(sx) * g.cs * ES, e = row + uint64_t(x) * g.cs * ES;
                        if constexpr (DT == LLCOMP_MI_DTYPE_U8) {
                            if (p.flags & LLCOMP_MI_ALPHA_OVER) {  // (checked: U8 HWC, c == 4, aligned to 4)
                                mem.store_el<4>(e, alpha_over_px(mem.load_el<4>(e), mem.load_el<4>(s)));
                                continue;
                            }
                        }
                        const uint32_t m = mem.load_el<1>(alpha_at<AB>(ag, p.src, sy, sx));
                        for (uint32_t k = 0; k < g.cs; ++k) {
                            uint32_t sv = p.value_bits;
                            if (p.flags & LLCOMP_MI_ALPHA_VALUE_PIXEL) sv = (p.value_bits >> (8 * k)) & 0xFFu;
                            else if (!(p.flags & LLCOMP_MI_ALPHA_VALUE)) sv = mem.load_el<ES>(s + uint64_t(k) * ES);
                            mem.store_el<ES>(e + uint64_t(k) * ES, alpha_paste_el<DT>(mem.load_el<ES>(e + uint64_t(k) * ES), sv, m, kAlphaWeights.w));
                        }
                    }
            }
}
template <uint32_t AB>
void alpha_reference_of(uint32_t dtype, const AlphaGeom& ag, uint32_t n_dst, uint32_t ow, uint32_t oh, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces) {
    switch (dtype) {
        case LLCOMP_MI_DTYPE_U8: return alpha_reference<AB, LLCOMP_MI_DTYPE_U8>(ag, n_dst, ow, oh, pieces, n_pieces);
        case LLCOMP_MI_DTYPE_F32: return alpha_reference<AB, LLCOMP_MI_DTYPE_F32>(ag, n_dst, ow, oh, pieces, n_pieces);
        case LLCOMP_MI_DTYPE_F16: return alpha_reference<AB, LLCOMP_MI_DTYPE_F16>(ag, n_dst, ow, oh, pieces, n_pieces);
        default: return alpha_reference<AB, LLCOMP_MI_DTYPE_BF16>(ag, n_dst, ow, oh, pieces, n_pieces);
    }
}
}  // namespace

}  // namespace llcomp_mi

extern "C" {

int llcomp_mi_alpha_paste_reference(const void* src, const void* alpha, uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw,
                                    uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                                    uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, void* out) {
    using namespace llcomp_mi;
    AlphaUses uses;
    if (int rc = alpha_check_call(alpha_px_bytes, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, uses)) return rc;
    const uint32_t es = batch_esize(dtype);
    const uint64_t dst_bytes = uint64_t(n_dst) * c * ow * oh * es;
    if (!dst_in) return LLCOMP_MI_BAD_ARGS;
    if (int rc = alpha_check_memory(src, uint64_t(n_src) * c * iw * ih * es, alpha, uint64_t(alpha_px_bytes) * n_src * iw * ih, out, dst_bytes, es, uses)) return rc;
    if (out != dst_in) std::memmove(out, dst_in, size_t(dst_bytes));
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const uint64_t o = reinterpret_cast<uintptr_t>(out), s = reinterpret_cast<uintptr_t>(src), a = reinterpret_cast<uintptr_t>(alpha);
    switch (alpha_px_bytes) {
        case 1: alpha_reference_of<1>(dtype, alpha_geom<1>(o, s, a, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, es, chw), n_dst, ow, oh, pieces, n_pieces); break;
        case 2: alpha_reference_of<2>(dtype, alpha_geom<2>(o, s, a, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, es, chw), n_dst, ow, oh, pieces, n_pieces); break;
        case 3: alpha_reference_of<3>(dtype, alpha_geom<3>(o, s, a, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, es, chw), n_dst, ow, oh, pieces, n_pieces); break;
        default: alpha_reference_of<4>(dtype, alpha_geom<4>(o, s, a, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, es, chw), n_dst, ow, oh, pieces, n_pieces); break;
    }
    return LLCOMP_MI_OK;
}

int llcomp_mi_alpha_paste_plan(uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow,
                               uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces,
                               uint32_t* samples, uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    using namespace llcomp_mi;
    if (!n_samples || !n_workgroups) return LLCOMP_MI_BAD_ARGS;
    AlphaUses uses;
    if (int rc = alpha_check_call(alpha_px_bytes, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, uses)) return rc;
    PastePlan p;
    alpha_plan(n_dst, pieces, n_pieces, p);
    for (size_t j = 0; j < p.samples.size(); ++j) {
        if (samples) samples[j] = p.samples[j].dst;
        if (first) first[j] = p.samples[j].first;
    }
    if (first) first[p.samples.size()] = uint32_t(p.order.size());
    if (order && !p.order.empty()) std::memcpy(order, p.order.data(), p.order.size() * 4);
    *n_samples = uint32_t(p.samples.size());
    *n_workgroups = paste_workgroups(p, ow, oh, c, dtype, layout);
    return LLCOMP_MI_OK;
}

}  // extern "C"
