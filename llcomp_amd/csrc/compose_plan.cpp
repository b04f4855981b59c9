// compose_plan.cpp -- the host half of the batch composition (compose_plan.hpp) and llcomp_mi_compose_reference.  Plain C++, no GPU.
#include "compose_plan.hpp"

#include <cstring>

#include "compose_rule.hpp"

namespace llcomp_mi {

static_assert(sizeof(llcomp_mi_compose_piece) == 40 && sizeof(ComposeRec) == 32 && sizeof(ComposeSample) == 12, "the table's records");

int compose_check_call(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                       const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, const float* fill_value, uint32_t flags,
                       std::vector<uint32_t>& fill_bits) {
    if (int rc = batch_check_shape(n_dst, c, ow, oh, dtype, layout)) return rc;
    if (n_src)  // (no src batch is fine: FILL pieces only)
        if (int rc = batch_check_shape(n_src, c, iw, ih, dtype, layout)) return rc;
    if (n_pieces > kComposeMaxPieces || (n_pieces && !pieces) || (flags & ~LLCOMP_MI_COMPOSE_KEEP)) return LLCOMP_MI_BAD_ARGS;
    const uint32_t es = batch_esize(dtype), cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    if (uint64_t(ow) * cs >= (1ull << 31) || (n_src && uint64_t(iw) * cs >= (1ull << 31))) return LLCOMP_MI_BAD_ARGS;
    const ComposeGeom g = compose_geom(0, 0, 0, 0, 0, ow, oh, c, es, cs == 1, false);
    if (g.planes > 65535u || uint64_t(g.tiles_x) * g.tiles_y > 0x7FFFFFFFu) return LLCOMP_MI_BAD_ARGS;  // (the kernel's grid)
    std::vector<uint32_t> on_sample(n_dst, 0u);
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const llcomp_mi_compose_piece& p = pieces[i];
        if (p.dst >= n_dst || p.reserved || (p.flags & ~LLCOMP_MI_COMPOSE_FILL)) return LLCOMP_MI_BAD_ARGS;
        if (p.dx > ow || p.w > ow - p.dx || p.dy > oh || p.h > oh - p.dy) return LLCOMP_MI_BAD_ARGS;
        if (p.flags & LLCOMP_MI_COMPOSE_FILL) {
            if (p.src || p.sx || p.sy) return LLCOMP_MI_BAD_ARGS;
        } else {
            if (p.src >= n_src || p.sx > iw || p.w > iw - p.sx || p.sy > ih || p.h > ih - p.sy) return LLCOMP_MI_BAD_ARGS;
        }
        if (!compose_empty(p) && ++on_sample[p.dst] > kComposeMaxPiecesPerSample) return LLCOMP_MI_BAD_ARGS;
    }
    return batch_value_bits(dtype, c, fill_value, fill_bits);
}

int compose_check_memory(const void* src, uint64_t src_bytes, const void* dst, uint64_t dst_bytes, uint32_t esize) {
    const uint64_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (!dst || (d & (esize - 1))) return LLCOMP_MI_BAD_ARGS;
    if (!src_bytes) return LLCOMP_MI_OK;
    if (!src || (s & (esize - 1))) return LLCOMP_MI_BAD_ARGS;
    if (s < d + dst_bytes && d < s + src_bytes) return LLCOMP_MI_BAD_ARGS;
    return LLCOMP_MI_OK;
}

void compose_plan(uint32_t n_dst, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, uint32_t flags, ComposePlan& p) {
    p = ComposePlan{};
    std::vector<uint32_t> at(size_t(n_dst) + 1, 0u);  // a counting sort: stable
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!compose_empty(pieces[i])) ++at[pieces[i].dst + 1];
    for (uint32_t d = 0; d < n_dst; ++d) {
        if (at[d + 1] || !(flags & LLCOMP_MI_COMPOSE_KEEP)) p.samples.push_back(ComposeSample{d, at[d], at[d + 1]});
        at[d + 1] += at[d];
    }
    p.order.resize(at[n_dst]);
    for (uint32_t i = 0; i < n_pieces; ++i)
        if (!compose_empty(pieces[i])) p.order[at[pieces[i].dst]++] = i;
    if ((flags & LLCOMP_MI_COMPOSE_KEEP) && p.order.empty()) p.samples.clear();
}

uint64_t compose_workgroups(const ComposePlan& p, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout) {
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const ComposeGeom g = compose_geom(0, 0, 0, 0, 0, ow, oh, c, batch_esize(dtype), chw, false);
    return uint64_t(p.samples.size()) * g.planes * g.tiles_x * g.tiles_y;
}

void compose_table_put(const llcomp_mi_compose_piece* pieces, const ComposePlan& p, const std::vector<uint32_t>& fill_bits, uint32_t layout, uint8_t* at) {
    const uint32_t c = uint32_t(fill_bits.size()), cs = layout == LLCOMP_MI_LAYOUT_CHW ? 1u : c;
    const ComposeTable t(p.samples.size(), p.order.size(), c);
    if (!p.samples.empty()) std::memcpy(at + t.samples_at, p.samples.data(), p.samples.size() * sizeof(ComposeSample));
    for (size_t j = 0; j < p.order.size(); ++j) {
        const ComposeRec r = compose_rec(pieces[p.order[j]], cs);
        std::memcpy(at + t.recs_at + j * sizeof(ComposeRec), &r, sizeof(ComposeRec));
    }
    std::memcpy(at + t.fill_at, fill_bits.data(), size_t(c) * 4);
}

int compose_reference(const void* src, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow, uint32_t oh,
                      uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, const float* fill_value,
                      uint32_t flags, void* out) {
    std::vector<uint32_t> fill;
    if (int rc = compose_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, fill_value, flags, fill)) return rc;
    const bool keep = flags & LLCOMP_MI_COMPOSE_KEEP, chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const uint32_t es = batch_esize(dtype);
    const uint64_t dst_bytes = uint64_t(n_dst) * c * ow * oh * es;
    if (keep && !dst_in) return LLCOMP_MI_BAD_ARGS;
    if (int rc = compose_check_memory(src, uint64_t(n_src) * c * iw * ih * es, out, dst_bytes, es)) return rc;
    uint8_t* o = static_cast<uint8_t*>(out);
    if (keep && out != dst_in) std::memmove(o, dst_in, size_t(dst_bytes));
    // the rule, element by element: the last piece that covers it, through the kernel's own address functions
    const ComposeGeom g = compose_geom(reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(src), n_src, iw, ih, ow, oh, c, es, chw, keep);
    for (uint32_t d = 0; d < n_dst; ++d)
        for (uint32_t pl = 0; pl < g.planes; ++pl)
            for (uint32_t y = 0; y < oh; ++y) {
                uint8_t* row = reinterpret_cast<uint8_t*>(uintptr_t(compose_dst_row(g, es, d, pl, y)));
                for (uint32_t x = 0; x < ow; ++x) {
                    const llcomp_mi_compose_piece* last = nullptr;
                    for (uint32_t i = n_pieces; i-- > 0 && !last;)
                        if (pieces[i].dst == d && compose_covers(pieces[i], x, y)) last = &pieces[i];
                    if (!last && keep) continue;
                    for (uint32_t k = 0; k < g.cs; ++k) {
                        uint8_t* e = row + (uint64_t(x) * g.cs + k) * es;
                        if (!last || (last->flags & LLCOMP_MI_COMPOSE_FILL)) {
                            std::memcpy(e, &fill[chw ? pl : k], es);  // (little-endian hosts, like the containers)
                        } else {
                            const uint64_t s = compose_src_row(g, es, last->src, pl, last->sy + (y - last->dy)) +
                                               (uint64_t(last->sx + (x - last->dx)) * g.cs + k) * es;
                            std::memcpy(e, reinterpret_cast<const uint8_t*>(uintptr_t(s)), es);
                        }
                    }
                }
            }
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_compose_tile(void) { return llcomp_mi::kComposeTile; }
uint32_t llcomp_mi_compose_tile_rows(uint32_t pixel_bytes) { return llcomp_mi::compose_tile_rows(pixel_bytes); }
uint32_t llcomp_mi_compose_max_pieces_per_sample(void) { return llcomp_mi::kComposeMaxPiecesPerSample; }

int llcomp_mi_compose_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, uint32_t flags, uint32_t* samples,
                           uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups) {
    if (!n_samples || !n_workgroups) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> fill;
    if (int rc = llcomp_mi::compose_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, nullptr, flags, fill)) return rc;
    llcomp_mi::ComposePlan p;
    llcomp_mi::compose_plan(n_dst, pieces, n_pieces, flags, p);
    for (size_t j = 0; j < p.samples.size(); ++j) {
        if (samples) samples[j] = p.samples[j].dst;
        if (first) first[j] = p.samples[j].first;
    }
    if (first) first[p.samples.size()] = uint32_t(p.order.size());
    if (order && !p.order.empty()) std::memcpy(order, p.order.data(), p.order.size() * 4);
    *n_samples = uint32_t(p.samples.size());
    *n_workgroups = llcomp_mi::compose_workgroups(p, ow, oh, c, dtype, layout);
    return LLCOMP_MI_OK;
}

int llcomp_mi_compose_reference(const void* src, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                                uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_compose_piece* pieces,
                                uint32_t n_pieces, const float* fill_value, uint32_t flags, void* out) {
    return llcomp_mi::compose_reference(src, n_src, iw, ih, dst_in, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, fill_value, flags, out);
}

}  // extern "C"
