// paste16_plan.cpp -- the host half of the batch copy-paste by 16-bit ids (paste16_plan.hpp) and llcomp_mi_paste16_reference.  Plain
// C++, no GPU.  The workgroups of a plan are the 8-bit call's (paste_plan.cpp: paste_workgroups).
#include "paste16_plan.hpp"

#include <cstring>

#include "paste16_rule.hpp"

namespace llcomp_mi {

static_assert(sizeof(llcomp_mi_paste_piece16) == 76 && sizeof(PasteRec16) == 72 && sizeof(PasteRec) == 68 && sizeof(ComposeSample) == 12, "the table's records");

int paste16_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces) {
    if (int rc = batch_check_shape(n_dst, c, ow, oh, dtype, layout)) return rc;
    if (n_src || n_pieces)  // (no src batch is fine for a call without pieces)
        if (int rc = batch_check_shape(n_src, c, iw, ih, dtype, layout)) return rc;
    if (n_pieces > kPasteMaxPieces || (n_pieces && !pieces)) return LLCOMP_MI_BAD_ARGS;
    const uint32_t es = batch_esize(dtype), cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    if (uint64_t(ow) * cs >= (1ull << 31) || (n_src && uint64_t(iw) * cs >= (1ull << 31))) return LLCOMP_MI_BAD_ARGS;
    const ComposeGeom g = compose_geom(0, 0, 0, 0, 0, ow, oh, c, es, cs == 1, true);
    if (g.planes > 65535u || uint64_t(g.tiles_x) * g.tiles_y > 0x7FFFFFFFu) return LLCOMP_MI_BAD_ARGS;  // (the kernel's grid)
    std::vector<uint32_t> on_sample(n_dst, 0u);
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const llcomp_mi_paste_piece16& p = pieces[i];
        if (p.dst >= n_dst || p.src >= n_src || (p.flags & ~LLCOMP_MI_PASTE_VALUE) || p.id_base > 65535u) return LLCOMP_MI_BAD_ARGS;
        if (p.dx > ow || p.w > ow - p.dx || p.dy > oh || p.h > oh - p.dy) return LLCOMP_MI_BAD_ARGS;
        if (p.sx > iw || p.w > iw - p.sx || p.sy > ih || p.h > ih - p.sy) return LLCOMP_MI_BAD_ARGS;
        if (p.flags & LLCOMP_MI_PASTE_VALUE) {
            if (es < 4 && (p.value_bits >> (8 * es))) return LLCOMP_MI_BAD_ARGS;  // bits above the element
        } else if (p.value_bits) {
            return LLCOMP_MI_BAD_ARGS;
        }
        if (!paste16_empty(p) && ++on_sample[p.dst] > kPasteMaxPiecesPerSample) return LLCOMP_MI_BAD_ARGS;
    }
    return LLCOMP_MI_OK;
}

int paste16_check_memory(const void* src, uint64_t src_bytes, const void* mask, uint64_t mask_bytes, const void* dst, uint64_t dst_bytes,
                         uint32_t esize, uint32_t n_pieces) {
    if (int rc = paste_check_memory(src, src_bytes, mask, mask_bytes, dst, dst_bytes, esize, n_pieces)) return rc;
    return n_pieces && (reinterpret_cast<uintptr_t>(mask) & 1u) ? LLCOMP_MI_BAD_ARGS : LLCOMP_MI_OK;
}

void paste16_plan(uint32_t n_dst, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, PastePlan& p) {
    p = PastePlan{};
    std::vector<uint32_t> at(size_t(n_dst) + 1, 0u);  // a counting sort: stable
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!paste16_idle(pieces[i])) ++at[pieces[i].dst + 1];
    for (uint32_t d = 0; d < n_dst; ++d) {
        if (at[d + 1]) p.samples.push_back(ComposeSample{d, at[d], at[d + 1]});
        at[d + 1] += at[d];
    }
    p.order.resize(at[n_dst]);
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!paste16_idle(pieces[i])) p.order[at[pieces[i].dst]++] = i;
}

void paste16_table_put(const llcomp_mi_paste_piece16* pieces, const PastePlan& p, uint32_t c, uint32_t layout, uint8_t* at) {
    const uint32_t cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    const PasteTable16 t(p.samples.size(), p.order.size());
    if (!p.samples.empty()) std::memcpy(at + t.samples_at, p.samples.data(), p.samples.size() * sizeof(ComposeSample));
    for (size_t j = 0; j < p.order.size(); ++j) {
        const PasteRec16 r = paste16_rec(pieces[p.order[j]], cs);
        std::memcpy(at + t.recs_at + j * sizeof(PasteRec16), &r, sizeof(PasteRec16));
    }
}

namespace {
// host memory as it is, for the rule's per-pixel function
struct PlainMem16 {
    template <uint32_t N>
    uint32_t load_el(uint64_t a) const {
        uint32_t v = 0;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);  // (little-endian hosts, like the containers)
        return v;
    }
};
}  // namespace

int paste16_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                      uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, void* out) {
    if (int rc = paste16_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces)) return rc;
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const uint32_t es = batch_esize(dtype);
    const uint64_t dst_bytes = uint64_t(n_dst) * c * ow * oh * es;
    if (!dst_in) return LLCOMP_MI_BAD_ARGS;
    if (int rc = paste16_check_memory(src, uint64_t(n_src) * c * iw * ih * es, mask, 2 * uint64_t(n_src) * iw * ih, out, dst_bytes, es, n_pieces)) return rc;
    uint8_t* o = static_cast<uint8_t*>(out);
    if (out != dst_in) std::memmove(o, dst_in, size_t(dst_bytes));
    // the rule, element by element: the last piece that selects its pixel, through the kernel's own address functions
    const PasteGeom pg = paste16_geom(reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(mask), n_src, iw,
                                      ih, ow, oh, c, es, chw);
    const ComposeGeom& g = pg.g;
    PlainMem16 mem;
    for (uint32_t d = 0; d < n_dst; ++d)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t y = 0; y < oh; ++y) {
                uint8_t* row = reinterpret_cast<uint8_t*>(uintptr_t(compose_dst_row(g, es, d, pl, y)));
                for (uint32_t x = 0; x < ow; ++x) {
                    uint32_t last = n_pieces;
                    for (uint32_t i = n_pieces; i-- > 0 && last == n_pieces;)
                        if (pieces[i].dst == d && paste16_selects(pg, pieces[i], x, y, mem)) last = i;
                    if (last == n_pieces) continue;
                    const llcomp_mi_paste_piece16& p = pieces[last];
                    for (uint32_t k = 0; k < g.cs; ++k) {
                        uint8_t* e = row + (uint64_t(x) * g.cs + k) * es;
                        if (p.flags & LLCOMP_MI_PASTE_VALUE) {
                            std::memcpy(e, &p.value_bits, es);
                        } else {
                            const uint64_t s = compose_src_row(g, es, p.src, pl, p.sy + (y - p.dy)) + (uint64_t(p.sx + (x - p.dx)) * g.cs + k) * es;
                            std::memcpy(e, reinterpret_cast<const uint8_t*>(uintptr_t(s)), es);
                        }
                    }
                }
            }
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

int llcomp_mi_paste16_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first,
                           uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    if (!n_samples || !n_workgroups) return LLCOMP_MI_BAD_ARGS;
    if (int rc = llcomp_mi::paste16_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces)) return rc;
    llcomp_mi::PastePlan p;
    llcomp_mi::paste16_plan(n_dst, pieces, n_pieces, p);
    for (size_t j = 0; j < p.samples.size(); ++j) {
        if (samples) samples[j] = p.samples[j].dst;
        if (first) first[j] = p.samples[j].first;
    }
    if (first) first[p.samples.size()] = uint32_t(p.order.size());
    if (order && !p.order.empty()) std::memcpy(order, p.order.data(), p.order.size() * 4);
    *n_samples = uint32_t(p.samples.size());
    *n_workgroups = llcomp_mi::paste_workgroups(p, ow, oh, c, dtype, layout);
    return LLCOMP_MI_OK;
}

int llcomp_mi_paste16_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                                uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces,
                                uint32_t n_pieces, void* out) {
    return llcomp_mi::paste16_reference(src, mask, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, out);
}

}  // extern "C"
