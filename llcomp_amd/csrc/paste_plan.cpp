// paste_plan.cpp -- the host half of the batch copy-paste (paste_plan.hpp) and the references, written once over the piece type and
// instantiated for the 8-bit and the 16-bit call.  Plain C++, no GPU.
#include "paste_plan.hpp"

#include <cstring>

#include "paste_rule.hpp"

namespace llcomp_mi {

static_assert(sizeof(llcomp_mi_paste_piece) == 72 && sizeof(llcomp_mi_paste_piece16) == 76 && sizeof(ComposeSample) == 12, "the table's records");
static_assert(sizeof(llcomp_mi_paste_piece32) == 76 && sizeof(PastePiece3) == 76 && sizeof(PastePiece4) == 76, "one layout, so that an array of the one is an array of the other");

namespace {
// A piece's own refusals, and its value in the dtype's bits.  8-bit: the float value as batch_value_bits converts a fill
bool paste_piece_value(const llcomp_mi_paste_piece& p, uint32_t dtype, uint32_t& bits) {
    if (p.flags & LLCOMP_MI_PASTE_VALUE) return mix_erase_bits(dtype, p.value, bits);
    return p.value == 0.0f;
}
// 16-bit: a base above 65535, value bits above the element
bool paste_piece_value(const llcomp_mi_paste_piece16& p, uint32_t dtype, uint32_t& bits) {
    const uint32_t es = batch_esize(dtype);
    if (p.id_base > 65535u) return false;
    if (!(p.flags & LLCOMP_MI_PASTE_VALUE)) return !p.value_bits;
    bits = p.value_bits;
    return es >= 4 || !(p.value_bits >> (8 * es));
}
// wide: the base within the map's ids, value bits above the element; VALUE_PIXEL with VALUE, on U8 HWC with c <= 4 only, its bytes
// at and above c zero
template <class P>
bool paste_piece_value_wide(const P& p, uint32_t dtype, uint32_t layout, uint32_t c, uint32_t& bits) {
    const uint32_t es = batch_esize(dtype);
    if (kPasteMaskBytesOf<P> == 3 && p.id_base > 0xFFFFFFu) return false;
    if (!(p.flags & LLCOMP_MI_PASTE_VALUE)) return !p.value_bits && !(p.flags & LLCOMP_MI_PASTE_VALUE_PIXEL);
    bits = p.value_bits;
    if (p.flags & LLCOMP_MI_PASTE_VALUE_PIXEL)
        return dtype == LLCOMP_MI_DTYPE_U8 && layout == LLCOMP_MI_LAYOUT_HWC && c <= 4 && (c == 4 || !(p.value_bits >> (8 * c)));
    return es >= 4 || !(p.value_bits >> (8 * es));
}
bool paste_piece_value(const PastePiece3& p, uint32_t dtype, uint32_t layout, uint32_t c, uint32_t& bits) { return paste_piece_value_wide(p, dtype, layout, c, bits); }
bool paste_piece_value(const PastePiece4& p, uint32_t dtype, uint32_t layout, uint32_t c, uint32_t& bits) { return paste_piece_value_wide(p, dtype, layout, c, bits); }
template <class P>
bool paste_piece_value(const P& p, uint32_t dtype, uint32_t, uint32_t, uint32_t& bits) { return paste_piece_value(p, dtype, bits); }
}  // namespace

int paste_check_shapes(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       bool has_pieces, uint32_t n_pieces) {
    if (int rc = batch_check_shape(n_dst, c, ow, oh, dtype, layout)) return rc;
    if (n_src || n_pieces)  // (no src batch is fine for a call without pieces)
        if (int rc = batch_check_shape(n_src, c, iw, ih, dtype, layout)) return rc;
    if (n_pieces > kPasteMaxPieces || (n_pieces && !has_pieces)) return LLCOMP_MI_BAD_ARGS;
    const uint32_t es = batch_esize(dtype), cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    if (uint64_t(ow) * cs >= (1ull << 31) || (n_src && uint64_t(iw) * cs >= (1ull << 31))) return LLCOMP_MI_BAD_ARGS;
    const ComposeGeom g = compose_geom(0, 0, 0, 0, 0, ow, oh, c, es, cs == 1, true);
    if (g.planes > 65535u || uint64_t(g.tiles_x) * g.tiles_y > 0x7FFFFFFFu) return LLCOMP_MI_BAD_ARGS;  // (the kernel's grid)
    return LLCOMP_MI_OK;
}

template <class P>
int paste_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                     const P* pieces, uint32_t n_pieces, std::vector<uint32_t>& value_bits) {
    if (int rc = paste_check_shapes(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces != nullptr, n_pieces)) return rc;
    std::vector<uint32_t> on_sample(n_dst, 0u), bits(n_pieces, 0u);
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const P& p = pieces[i];
        if (!paste_piece_fits(p, n_src, iw, ih, n_dst, ow, oh) || (p.flags & ~kPasteFlagBits<kPasteMaskBytesOf<P>>)) return LLCOMP_MI_BAD_ARGS;
        if (!paste_piece_value(p, dtype, layout, c, bits[i])) return LLCOMP_MI_BAD_ARGS;
        if (!paste_empty(p) && ++on_sample[p.dst] > kPasteMaxPiecesPerSample) return LLCOMP_MI_BAD_ARGS;
    }
    value_bits.swap(bits);
    return LLCOMP_MI_OK;
}

int paste_check_memory(const void* src, uint64_t src_bytes, const void* mask, uint64_t mask_bytes, const void* dst, uint64_t dst_bytes,
                       uint32_t esize, uint32_t mask_px, uint32_t n_pieces) {
    const uint64_t s = reinterpret_cast<uintptr_t>(src), m = reinterpret_cast<uintptr_t>(mask), d = reinterpret_cast<uintptr_t>(dst);
    if (!dst || (d & (esize - 1))) return LLCOMP_MI_BAD_ARGS;
    if (!n_pieces) return LLCOMP_MI_OK;
    if (!src || !mask || (s & (esize - 1)) || (m & (mask_px - 1))) return LLCOMP_MI_BAD_ARGS;
    if (s < d + dst_bytes && d < s + src_bytes) return LLCOMP_MI_BAD_ARGS;
    if (m < d + dst_bytes && d < m + mask_bytes) return LLCOMP_MI_BAD_ARGS;
    return LLCOMP_MI_OK;
}

template <class P>
void paste_plan(uint32_t n_dst, const P* pieces, uint32_t n_pieces, PastePlan& p) {
    paste_plan_by(n_dst, pieces, n_pieces, p, [](const P& q) { return paste_idle(q); });
}

uint64_t paste_workgroups(const PastePlan& p, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout) {
    const ComposeGeom g = compose_geom(0, 0, 0, 0, 0, ow, oh, c, batch_esize(dtype), layout == LLCOMP_MI_LAYOUT_CHW, true);
    return uint64_t(p.samples.size()) * g.planes * g.tiles_x * g.tiles_y;
}

template <class P>
void paste_table_put(const P* pieces, const PastePlan& p, const std::vector<uint32_t>& value_bits, uint32_t c, uint32_t layout, uint8_t* at) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    const uint32_t cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    const PasteTable<MB> t(p.samples.size(), p.order.size());
    static_assert(sizeof(PasteRec<MB>) == (MB == 1 ? 68 : 72), "PasteTable's record");
    if (!p.samples.empty()) std::memcpy(at + t.samples_at, p.samples.data(), p.samples.size() * sizeof(ComposeSample));
    for (size_t j = 0; j < p.order.size(); ++j) {
        const PasteRec<MB> r = paste_rec(pieces[p.order[j]], cs, value_bits[p.order[j]]);
        std::memcpy(at + t.recs_at + j * sizeof(r), &r, sizeof(r));
    }
}

template <class P>
int paste_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                    uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const P* pieces, uint32_t n_pieces, void* out) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    std::vector<uint32_t> value_bits;
    if (int rc = paste_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, value_bits)) return rc;
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const uint32_t es = batch_esize(dtype);
    const uint64_t dst_bytes = uint64_t(n_dst) * c * ow * oh * es;
    if (!dst_in) return LLCOMP_MI_BAD_ARGS;
    if (int rc = paste_check_memory(src, uint64_t(n_src) * c * iw * ih * es, mask, MB * uint64_t(n_src) * iw * ih, out, dst_bytes, es, paste_mask_align(MB), n_pieces)) return rc;
    uint8_t* o = static_cast<uint8_t*>(out);
    if (out != dst_in) std::memmove(o, dst_in, size_t(dst_bytes));
    // the rule, element by element: the last piece that selects its pixel, through the kernel's own address functions
    const PasteGeom pg = paste_geom<MB>(reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(mask), n_src, iw,
                                        ih, ow, oh, c, es, chw);
    const ComposeGeom& g = pg.g;
    PlainMem mem;
    for (uint32_t d = 0; d < n_dst; ++d)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t y = 0; y < oh; ++y) {
                uint8_t* row = reinterpret_cast<uint8_t*>(uintptr_t(compose_dst_row(g, es, d, pl, y)));
                for (uint32_t x = 0; x < ow; ++x) {
                    uint32_t last = n_pieces;
                    for (uint32_t i = n_pieces; i-- > 0 && last == n_pieces;)
                        if (pieces[i].dst == d && paste_selects<MB>(pg, pieces[i], x, y, mem)) last = i;
                    if (last == n_pieces) continue;
                    const P& p = pieces[last];
                    for (uint32_t k = 0; k < g.cs; ++k) {
                        uint8_t* e = row + (uint64_t(x) * g.cs + k) * es;
                        if (p.flags & LLCOMP_MI_PASTE_VALUE_PIXEL) {  // (the wide call's, checked: U8 HWC)
                            *e = uint8_t(value_bits[last] >> (8 * k));
                        } else if (p.flags & LLCOMP_MI_PASTE_VALUE) {
                            std::memcpy(e, &value_bits[last], es);
                        } else {
                            const uint64_t s = compose_src_row(g, es, p.src, pl, p.sy + (y - p.dy)) + (uint64_t(p.sx + (x - p.dx)) * g.cs + k) * es;
                            std::memcpy(e, reinterpret_cast<const uint8_t*>(uintptr_t(s)), es);
                        }
                    }
                }
            }
    return LLCOMP_MI_OK;
}

namespace {
// llcomp_mi_paste_plan and llcomp_mi_paste16_plan
template <class P>
int paste_plan_out(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                   const P* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    if (!n_samples || !n_workgroups) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> bits;
    if (int rc = paste_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, bits)) return rc;
    PastePlan p;
    paste_plan(n_dst, pieces, n_pieces, p);
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
}  // namespace

#define LLMI_PASTE_INSTANTIATE(P)                                                                                                                  \
    template int paste_check_call<P>(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const P*, uint32_t, \
                                     std::vector<uint32_t>&);                                                                                     \
    template void paste_plan<P>(uint32_t, const P*, uint32_t, PastePlan&);                                                                        \
    template void paste_table_put<P>(const P*, const PastePlan&, const std::vector<uint32_t>&, uint32_t, uint32_t, uint8_t*);                     \
    template int paste_reference<P>(const void*, const void*, uint32_t, uint32_t, uint32_t, const void*, uint32_t, uint32_t, uint32_t, uint32_t,  \
                                    uint32_t, uint32_t, const P*, uint32_t, void*);
LLMI_PASTE_INSTANTIATE(llcomp_mi_paste_piece)
LLMI_PASTE_INSTANTIATE(llcomp_mi_paste_piece16)
LLMI_PASTE_INSTANTIATE(PastePiece3)
LLMI_PASTE_INSTANTIATE(PastePiece4)
#undef LLMI_PASTE_INSTANTIATE

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_paste_max_pieces_per_sample(void) { return llcomp_mi::kPasteMaxPiecesPerSample; }

int llcomp_mi_paste_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                         uint32_t layout, const llcomp_mi_paste_piece* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first,
                         uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    return llcomp_mi::paste_plan_out(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, samples, first, order, n_samples, n_workgroups);
}
int llcomp_mi_paste16_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first,
                           uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    return llcomp_mi::paste_plan_out(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, samples, first, order, n_samples, n_workgroups);
}

int llcomp_mi_paste32_plan(uint32_t map_bytes, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_paste_piece32* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first, uint32_t* order,
                           uint32_t* n_samples, uint64_t* n_workgroups) {
    using namespace llcomp_mi;
    if (map_bytes == 3)
        return paste_plan_out(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, static_cast<const PastePiece3*>(pieces), n_pieces, samples, first, order, n_samples, n_workgroups);
    if (map_bytes == 4)
        return paste_plan_out(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, static_cast<const PastePiece4*>(pieces), n_pieces, samples, first, order, n_samples, n_workgroups);
    return LLCOMP_MI_BAD_ARGS;
}
int llcomp_mi_paste32_reference(const void* src, const void* mask, uint32_t map_bytes, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                                uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece32* pieces, uint32_t n_pieces,
                                void* out) {
    using namespace llcomp_mi;
    if (map_bytes == 3) return paste_reference(src, mask, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, static_cast<const PastePiece3*>(pieces), n_pieces, out);
    if (map_bytes == 4) return paste_reference(src, mask, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, static_cast<const PastePiece4*>(pieces), n_pieces, out);
    return LLCOMP_MI_BAD_ARGS;
}

int llcomp_mi_paste_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                              uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece* pieces,
                              uint32_t n_pieces, void* out) {
    return llcomp_mi::paste_reference(src, mask, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, out);
}
int llcomp_mi_paste16_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                                uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces,
                                uint32_t n_pieces, void* out) {
    return llcomp_mi::paste_reference(src, mask, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, out);
}

}  // extern "C"
