// windows_plan.cpp -- the host planner of the windowed decodes (windows_plan.hpp).  Plain C++, no GPU.
#include "windows_plan.hpp"

#include <algorithm>
#include <cstring>

namespace llcomp_mi {

int regions_setup(const Geometry& g, const Tuning& tune, const uint32_t* xy, uint32_t rw, uint32_t rh, RegionsFrame* tab, RegionsClass* classes,
                  uint32_t& n_classes) {
    if (!xy) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> rects(4 * size_t(g.frames));
    for (uint32_t f = 0; f < g.frames; ++f) {
        rects[4 * f + 0] = xy[2 * f];
        rects[4 * f + 1] = xy[2 * f + 1];
        rects[4 * f + 2] = rw;
        rects[4 * f + 3] = rh;
    }
    return regions_setup_sized(g, tune, rects.data(), rw, rh, tab, classes, n_classes);
}

int regions_setup_sized(const Geometry& g, const Tuning& tune, const uint32_t* rects, uint32_t wmax, uint32_t hmax, RegionsFrame* tab,
                        RegionsClass* classes, uint32_t& n_classes, const uint32_t* used, uint32_t n_used) {
    if (!rects || (used && (!n_used || n_used > g.frames))) return LLCOMP_MI_BAD_ARGS;
    const uint32_t m = used ? n_used : g.frames;
    RegionBox win[kRegionsClasses];
    uint32_t count[kRegionsClasses] = {}, cls = 0;
    for (uint32_t i = 0; i < m; ++i) {
        RegionBox b;
        const uint32_t f = used ? used[i] : i;
        if (f >= g.frames) return LLCOMP_MI_BAD_ARGS;
        const uint32_t* r = rects + 4 * size_t(f);
        if (!regions_window_sized(g.w, g.h, g.tile_w, g.tile_h, r[0], r[1], r[2], r[3], wmax, hmax, b, cls)) return LLCOMP_MI_BAD_ARGS;
        win[cls] = b;  // (the window's size, all the sub-geometry depends on, is the class's)
        ++count[cls];
    }
    uint32_t first[kRegionsClasses], next = 0;
    const Geometry* sub_of[kRegionsClasses] = {};
    n_classes = 0;
    for (uint32_t c = 0; c < kRegionsClasses; ++c) {
        first[c] = next;
        next += count[c];
        if (!count[c]) continue;
        RegionsClass& rc = classes[n_classes++];
        sub_of[c] = &rc.sub;
        rc.first = first[c];
        if (!regions_geometry(g, win[c], count[c], tune, rc.sub) || !regions_fits(g, rc.sub)) return LLCOMP_MI_HIP_ERROR;
    }
    for (uint32_t i = 0; i < m; ++i) {
        RegionBox b;
        const uint32_t f = used ? used[i] : i;
        const uint32_t* r = rects + 4 * size_t(f);
        (void)regions_window_sized(g.w, g.h, g.tile_w, g.tile_h, r[0], r[1], r[2], r[3], wmax, hmax, b, cls);
        const uint32_t cx = r[0] - b.tx0 * g.tile_w, cy = r[1] - b.ty0 * g.tile_h;
        // (sub.w >= wmax: a window of Wx tile columns is at least wmax pixels wide, also where it ends at a partial column)
        const uint32_t bx = std::min(cx, sub_of[cls]->w >= wmax ? sub_of[cls]->w - wmax : 0u);
        const uint32_t by = std::min(cy, sub_of[cls]->h >= hmax ? sub_of[cls]->h - hmax : 0u);
        RegionsFrame& e = tab[first[cls]++];
        e = RegionsFrame{f, b.tx0, b.ty0, bx, by, used ? i : f, cls, 0};
    }
    // (what the crop kernels rely on; the window contains the box by construction)
    for (uint32_t i = 0; i < n_classes; ++i) {
        const RegionsClass& rc = classes[i];
        for (uint32_t j = 0; j < rc.sub.frames; ++j) {
            const RegionsFrame& e = tab[rc.first + j];
            if (uint64_t(e.cx0) + wmax > rc.sub.w || uint64_t(e.cy0) + hmax > rc.sub.h || e.out >= m || e.frame >= g.frames) return LLCOMP_MI_HIP_ERROR;
        }
    }
    return LLCOMP_MI_OK;
}

uint64_t stage_bound(const Geometry& g) { return StageLayout(g.frames, g.n_slices, uint64_t(g.n_slices) * (g.slice_cap - 16)).bytes; }
uint64_t resized_tables_bound(const Geometry& g) {
    return 16 + uint64_t(g.frames) * (sizeof(ResizeFrame) + 4 * 10 * (uint64_t(g.w) + g.h)) + 16 + 256 * 4 * uint64_t(g.c);
}
uint64_t view_term(const Geometry& g) { return sizeof(ResizeFrame) + 4 * 10 * (uint64_t(g.w) + g.h) + 16 + 256 * 4 * uint64_t(g.c); }
uint64_t views_tables_bound(const Geometry& g, uint64_t total_views) {
    return resized_tables_bound(g) + (total_views > g.frames ? (total_views - g.frames) * view_term(g) : 0);
}

uint64_t padded_term(const Geometry& g) { return 4 * 13 * (uint64_t(g.w) + g.h); }
uint64_t padded_tables_bound(const Geometry& g, uint64_t total_views) {
    return views_tables_bound(g, total_views) + std::max<uint64_t>(total_views, g.frames) * padded_term(g) + 4 * uint64_t(g.c);
}

void ResampleBlock::put(uint8_t* at) const {
    std::memcpy(at, rs.data(), rs.size() * sizeof(ResizeFrame));
    std::memcpy(at + w_at(), w.data(), 4 * w.size());
    if (!tables.empty()) std::memcpy(at + tables_at(), tables.data(), tables.size());
}
uint64_t ResampleBlock::add_table(const llcomp_mi_output_format* fmt, uint32_t c, const OutFormat& o) {
    if (o.plain) return 0;
    const size_t at = (tables.size() + 15) & ~size_t(15);
    tables.resize(at + o.table_bytes(c));
    output_table(fmt, c, o, tables.data() + at);
    return at;
}

int resized_setup(const Geometry& g, const Tuning& tune, const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                  const llcomp_mi_output_format* fmt, void* d_out, ResizedPlan& p) {
    ResampleGroup vg;
    if (int rc = check_output_format(fmt, g.c, vg.out)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & (vg.out.esize - 1)) return LLCOMP_MI_BAD_ARGS;
    if (!rects || !ow || !oh || g.frames > 65535) return LLCOMP_MI_BAD_ARGS;
    for (uint32_t f = 0; f < g.frames; ++f) {
        const uint32_t rw = rects[4 * f + 2], rh = rects[4 * f + 3], filter = flags ? LLCOMP_MI_FLAG_FILTER_OF(flags[f]) : 0u;
        // (an empty rectangle is regions_setup_sized's to refuse; an unknown filter and a downscale above the filter's limit are refused here)
        if (filter >= kResizeFilters || (rw && !resize_axis_ok(filter, rw, ow)) || (rh && !resize_axis_ok(filter, rh, oh))) return LLCOMP_MI_BAD_ARGS;
        p.wmax = std::max(p.wmax, rw);
        p.hmax = std::max(p.hmax, rh);
    }
    p.tab.resize(g.frames);
    if (int rc = regions_setup_sized(g, tune, rects, p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes)) return rc;
    ResampleBlock& blk = p.tail.block;
    blk.rs.assign(g.frames, ResizeFrame{});
    std::vector<uint32_t> seen;  // (axes already computed in this call)
    for (const RegionsFrame& e : p.tab) {
        const uint32_t* r = rects + 4 * size_t(e.frame);
        ResizeFrame& z = blk.rs[e.frame];
        z.ox = r[0] - e.wx0 * g.tile_w - e.cx0;
        z.oy = r[1] - e.wy0 * g.tile_h - e.cy0;
        z.flags = flags ? flags[e.frame] & (1u | LLCOMP_MI_FLAG_FILTER_MASK) : 0u;
        z.box = e.out;  // (the frame's own box)
        if (!resize_frame_weights(LLCOMP_MI_FLAG_FILTER_OF(z.flags), r[2], r[3], ow, oh, z, blk.w, seen)) return LLCOMP_MI_BAD_ARGS;
        if (uint64_t(z.ox) + z.rw > p.wmax || uint64_t(z.oy) + z.rh > p.hmax) return LLCOMP_MI_HIP_ERROR;  // (the box holds it by construction)
    }
    vg.n = vg.chunk = g.frames;
    vg.ow = ow;
    vg.oh = oh;
    vg.mh = p.hmax;
    vg.d_out = d_out;
    vg.table_at = blk.add_table(fmt, g.c, vg.out);
    p.tail.groups.assign(1, vg);
    p.tail.box_bytes = uint64_t(g.frames) * p.wmax * p.hmax * g.c;
    p.tail.mid_bytes = uint64_t(g.frames) * p.hmax * ow * g.c;
    return LLCOMP_MI_OK;
}

int views_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_view_group* groups, uint32_t n_groups, ViewsPlan& p) {
    if (int rc = views_union(g.w, g.h, g.frames, groups, n_groups, p.u)) return rc;
    std::vector<ResampleGroup>& out = p.tail.groups;
    out.resize(n_groups);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = *view_group_at(groups, gi);
        if (int rc = check_output_format(gr.fmt, g.c, out[gi].out)) return rc;
        if (!gr.d_out || (reinterpret_cast<uintptr_t>(gr.d_out) & (out[gi].out.esize - 1))) return LLCOMP_MI_BAD_ARGS;
    }
    const uint32_t n_used = uint32_t(p.u.used.size());
    p.wmax = p.u.wmax;
    p.hmax = p.u.hmax;
    p.tab.resize(n_used);
    if (int rc = regions_setup_sized(g, tune, p.u.rects.data(), p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes, p.u.used.data(), n_used))
        return rc;
    std::vector<uint32_t> entry_of(g.frames, 0);  // a used frame's entry of the regions table
    for (uint32_t i = 0; i < n_used; ++i) entry_of[p.tab[i].frame] = i;
    const uint64_t samples = uint64_t(g.frames) * g.w * g.h * g.c;
    ResampleBlock& blk = p.tail.block;
    std::vector<uint32_t> seen;  // (axes already computed in this call)
    blk.rs.reserve(size_t(p.u.total_views));
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = *view_group_at(groups, gi);
        ResampleGroup& vg = out[gi];
        vg.n = gr.n_views;
        vg.ow = gr.ow;
        vg.oh = gr.oh;
        vg.d_out = gr.d_out;
        vg.first = uint32_t(blk.rs.size());
        for (uint32_t i = 0; i < gr.n_views; ++i) {
            const llcomp_mi_view& v = gr.views[i];
            const RegionsFrame& e = p.tab[entry_of[v.frame]];
            ResizeFrame z{};
            z.ox = v.x - e.wx0 * g.tile_w - e.cx0;  // (the box starts at or before the union's origin, which no view starts before)
            z.oy = v.y - e.wy0 * g.tile_h - e.cy0;
            z.flags = v.flags & (1u | LLCOMP_MI_FLAG_FILTER_MASK);
            z.box = e.out;
            if (!resize_frame_weights(LLCOMP_MI_FLAG_FILTER_OF(z.flags), v.rw, v.rh, gr.ow, gr.oh, z, blk.w, seen)) return LLCOMP_MI_BAD_ARGS;
            // (the box holds the union, and the union the view, by construction)
            if (e.frame != v.frame || uint64_t(z.ox) + z.rw > p.wmax || uint64_t(z.oy) + z.rh > p.hmax || z.box >= n_used) return LLCOMP_MI_HIP_ERROR;
            vg.mh = std::max(vg.mh, v.rh);
            blk.rs.push_back(z);
        }
        const uint64_t per_view = uint64_t(vg.mh) * vg.ow * g.c;
        vg.chunk = uint32_t(std::min<uint64_t>(vg.n, std::max<uint64_t>(samples / per_view, 1)));
        p.tail.mid_bytes = std::max(p.tail.mid_bytes, vg.chunk * per_view);
        vg.table_at = blk.add_table(gr.fmt, g.c, vg.out);
    }
    p.tail.box_bytes = uint64_t(n_used) * p.wmax * p.hmax * g.c;
    return LLCOMP_MI_OK;
}

int check_pad(const llcomp_mi_pad* pad) {
    return pad && pad->struct_size >= sizeof(llcomp_mi_pad) && pad->mode <= LLCOMP_MI_PAD_SYMMETRIC ? LLCOMP_MI_OK : LLCOMP_MI_BAD_ARGS;
}
// whether the call needs the bias arrays: CONSTANT with a fill other than 0
static bool pad_has_fill(const llcomp_mi_pad& pad, uint32_t c) {
    if (pad.mode != LLCOMP_MI_PAD_CONSTANT || !pad.fill) return false;
    for (uint32_t ch = 0; ch < c; ++ch)
        if (pad.fill[ch]) return true;
    return false;
}
// the call's fill values behind the weights, and their offset into every entry
static void put_fill(const llcomp_mi_pad& pad, uint32_t c, ResampleBlock& blk) {
    const uint32_t at = uint32_t(blk.w.size());
    for (uint32_t ch = 0; ch < c; ++ch) blk.w.push_back(int32_t(pad.fill[ch]));
    for (ResizeFrame& z : blk.rs) z.pad[1] = at;
}

int padded_setup(const Geometry& g, const Tuning& tune, const int32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                 const llcomp_mi_pad* pad, const llcomp_mi_output_format* fmt, void* d_out, ResizedPlan& p, std::vector<uint32_t>& src) {
    ResampleGroup vg;
    if (int rc = check_output_format(fmt, g.c, vg.out)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & (vg.out.esize - 1)) return LLCOMP_MI_BAD_ARGS;
    if (!rects || !ow || !oh || g.frames > 65535) return LLCOMP_MI_BAD_ARGS;
    if (int rc = check_pad(pad)) return rc;
    src.assign(4 * size_t(g.frames), 0);
    for (uint32_t f = 0; f < g.frames; ++f) {
        const int32_t* r = rects + 4 * size_t(f);
        const uint32_t filter = flags ? LLCOMP_MI_FLAG_FILTER_OF(flags[f]) : 0u;
        uint32_t* s = src.data() + 4 * size_t(f);
        if (r[2] < 1 || r[3] < 1 || !pad_axis(pad->mode, g.w, r[0], uint32_t(r[2]), s[0], s[2]) ||
            !pad_axis(pad->mode, g.h, r[1], uint32_t(r[3]), s[1], s[3]))
            return LLCOMP_MI_BAD_ARGS;
        if (!resize_axis_ok(filter, uint32_t(r[2]), ow) || !resize_axis_ok(filter, uint32_t(r[3]), oh)) return LLCOMP_MI_BAD_ARGS;
        p.wmax = std::max(p.wmax, s[2]);
        p.hmax = std::max(p.hmax, s[3]);
    }
    p.tab.resize(g.frames);
    if (int rc = regions_setup_sized(g, tune, src.data(), p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes)) return rc;
    const bool with_bias = pad_has_fill(*pad, g.c);
    ResampleBlock& blk = p.tail.block;
    blk.rs.assign(g.frames, ResizeFrame{});
    if (with_bias) blk.biased.assign(g.frames, 0);
    PaddedSeen seen;  // (axes already computed in this call)
    for (const RegionsFrame& e : p.tab) {
        const uint32_t* s = src.data() + 4 * size_t(e.frame);
        ResizeFrame& z = blk.rs[e.frame];
        z.ox = s[0] - e.wx0 * g.tile_w - e.cx0;
        z.oy = s[1] - e.wy0 * g.tile_h - e.cy0;
        z.flags = flags ? flags[e.frame] & (1u | LLCOMP_MI_FLAG_FILTER_MASK) : 0u;
        z.box = e.out;  // (the frame's own box)
        uint32_t got[4];
        bool biased = false;
        if (!padded_frame_weights(LLCOMP_MI_FLAG_FILTER_OF(z.flags), pad->mode, g.w, g.h, rects + 4 * size_t(e.frame), ow, oh, with_bias, z, got,
                                  &biased, blk.w, seen))
            return LLCOMP_MI_BAD_ARGS;
        if (with_bias) blk.biased[e.frame] = biased;
        // (the weights are those of the source rectangle the windows were planned for, and the box holds it by construction)
        if (std::memcmp(got, s, sizeof got) != 0 || uint64_t(z.ox) + z.rw > p.wmax || uint64_t(z.oy) + z.rh > p.hmax) return LLCOMP_MI_HIP_ERROR;
    }
    if (with_bias) put_fill(*pad, g.c, blk);
    vg.n = vg.chunk = g.frames;
    vg.ow = ow;
    vg.oh = oh;
    vg.mh = p.hmax;
    vg.d_out = d_out;
    vg.table_at = blk.add_table(fmt, g.c, vg.out);
    p.tail.groups.assign(1, vg);
    p.tail.box_bytes = uint64_t(g.frames) * p.wmax * p.hmax * g.c;
    p.tail.mid_bytes = uint64_t(g.frames) * p.hmax * ow * g.c;
    return LLCOMP_MI_OK;
}

int padded_views_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                       ViewsPlan& p) {
    if (!groups || !n_groups || groups->struct_size != sizeof(llcomp_mi_view_group)) return LLCOMP_MI_BAD_ARGS;
    if (int rc = check_pad(pad)) return rc;
    // the groups again with every view's source rectangle in place of its rectangle: what views_union and the windows see
    std::vector<llcomp_mi_view_group> sgroups(n_groups);
    std::vector<std::vector<llcomp_mi_view>> sviews(n_groups);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = *view_group_at(groups, gi);
        if (gr.struct_size != sizeof(llcomp_mi_view_group) || !gr.n_views || gr.n_views > 65535 || !gr.views || !gr.ow || !gr.oh)
            return LLCOMP_MI_BAD_ARGS;
        sviews[gi].assign(gr.views, gr.views + gr.n_views);
        for (llcomp_mi_view& v : sviews[gi]) {
            const uint32_t filter = LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu);
            const uint32_t rw = v.rw, rh = v.rh;
            if (!rw || !rh || rw > 0x7FFFFFFFu || rh > 0x7FFFFFFFu || !resize_axis_ok(filter, rw, gr.ow) || !resize_axis_ok(filter, rh, gr.oh))
                return LLCOMP_MI_BAD_ARGS;
            if (!pad_axis(pad->mode, g.w, int32_t(v.x), rw, v.x, v.rw) || !pad_axis(pad->mode, g.h, int32_t(v.y), rh, v.y, v.rh))
                return LLCOMP_MI_BAD_ARGS;
        }
        sgroups[gi] = gr;
        sgroups[gi].views = sviews[gi].data();
    }
    if (int rc = views_union(g.w, g.h, g.frames, sgroups.data(), n_groups, p.u)) return rc;
    std::vector<ResampleGroup>& out = p.tail.groups;
    out.resize(n_groups);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = sgroups[gi];
        if (int rc = check_output_format(gr.fmt, g.c, out[gi].out)) return rc;
        if (!gr.d_out || (reinterpret_cast<uintptr_t>(gr.d_out) & (out[gi].out.esize - 1))) return LLCOMP_MI_BAD_ARGS;
    }
    const uint32_t n_used = uint32_t(p.u.used.size());
    p.wmax = p.u.wmax;
    p.hmax = p.u.hmax;
    p.tab.resize(n_used);
    if (int rc = regions_setup_sized(g, tune, p.u.rects.data(), p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes, p.u.used.data(), n_used))
        return rc;
    std::vector<uint32_t> entry_of(g.frames, 0);  // a used frame's entry of the regions table
    for (uint32_t i = 0; i < n_used; ++i) entry_of[p.tab[i].frame] = i;
    const uint64_t samples = uint64_t(g.frames) * g.w * g.h * g.c;
    const bool with_bias = pad_has_fill(*pad, g.c);
    ResampleBlock& blk = p.tail.block;
    PaddedSeen seen;  // (axes already computed in this call)
    blk.rs.reserve(size_t(p.u.total_views));
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = *view_group_at(groups, gi);
        ResampleGroup& vg = out[gi];
        vg.n = gr.n_views;
        vg.ow = gr.ow;
        vg.oh = gr.oh;
        vg.d_out = gr.d_out;
        vg.first = uint32_t(blk.rs.size());
        for (uint32_t i = 0; i < gr.n_views; ++i) {
            const llcomp_mi_view& v = gr.views[i];
            const llcomp_mi_view& sv = sviews[gi][i];
            const RegionsFrame& e = p.tab[entry_of[v.frame]];
            ResizeFrame z{};
            z.ox = sv.x - e.wx0 * g.tile_w - e.cx0;  // (the box starts at or before the union's origin, which no source rectangle starts before)
            z.oy = sv.y - e.wy0 * g.tile_h - e.cy0;
            z.flags = v.flags & (1u | LLCOMP_MI_FLAG_FILTER_MASK);
            z.box = e.out;
            const int32_t rect[4] = {int32_t(v.x), int32_t(v.y), int32_t(v.rw), int32_t(v.rh)};
            uint32_t got[4];
            bool biased = false;
            if (!padded_frame_weights(LLCOMP_MI_FLAG_FILTER_OF(z.flags), pad->mode, g.w, g.h, rect, gr.ow, gr.oh, with_bias, z, got, &biased, blk.w, seen))
                return LLCOMP_MI_BAD_ARGS;
            if (e.frame != v.frame || got[0] != sv.x || got[1] != sv.y || got[2] != sv.rw || got[3] != sv.rh || uint64_t(z.ox) + z.rw > p.wmax ||
                uint64_t(z.oy) + z.rh > p.hmax || z.box >= n_used)
                return LLCOMP_MI_HIP_ERROR;
            vg.mh = std::max(vg.mh, z.rh);
            blk.rs.push_back(z);
            if (with_bias) blk.biased.push_back(biased);
        }
        const uint64_t per_view = uint64_t(vg.mh) * vg.ow * g.c;
        vg.chunk = uint32_t(std::min<uint64_t>(vg.n, std::max<uint64_t>(samples / per_view, 1)));
        p.tail.mid_bytes = std::max(p.tail.mid_bytes, vg.chunk * per_view);
        vg.table_at = blk.add_table(gr.fmt, g.c, vg.out);
    }
    if (with_bias) put_fill(*pad, g.c, blk);
    p.tail.box_bytes = uint64_t(n_used) * p.wmax * p.hmax * g.c;
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

int llcomp_mi_pad_axis(uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t* s0, uint32_t* s_len) {
    uint32_t a = 0, l = 0;
    if (!s0 || !s_len || !llcomp_mi::pad_axis(mode, n, x, r, a, l)) return LLCOMP_MI_BAD_ARGS;
    *s0 = a;
    *s_len = l;
    return LLCOMP_MI_OK;
}

uint32_t llcomp_mi_padded_filter_weights(uint32_t filter, uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t out_len, uint32_t* s0,
                                         uint32_t* lo, int32_t* q, int32_t* bias) {
    llcomp_mi::PaddedAxis a;
    if (!llcomp_mi::padded_axis(filter, mode, n, x, r, out_len, a)) return 0;
    if (s0) *s0 = a.s0;
    if (lo) std::memcpy(lo, a.lo.data(), 4 * size_t(out_len));
    if (q) std::memcpy(q, a.q.data(), 4 * a.q.size());
    if (bias) std::memcpy(bias, a.bias.data(), 4 * size_t(out_len));
    return a.k;
}

int llcomp_mi_padded_regions_plan(uint32_t w, uint32_t h, const int32_t* rects, uint32_t n, const llcomp_mi_pad* pad, uint32_t* src) {
    if (!rects || !n || !src || llcomp_mi::check_pad(pad)) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> s(4 * size_t(n));
    for (uint32_t f = 0; f < n; ++f) {
        const int32_t* r = rects + 4 * size_t(f);
        uint32_t* o = s.data() + 4 * size_t(f);
        if (r[2] < 1 || r[3] < 1 || !llcomp_mi::pad_axis(pad->mode, w, r[0], uint32_t(r[2]), o[0], o[2]) ||
            !llcomp_mi::pad_axis(pad->mode, h, r[1], uint32_t(r[3]), o[1], o[3]))
            return LLCOMP_MI_BAD_ARGS;
    }
    std::memcpy(src, s.data(), 4 * s.size());
    return LLCOMP_MI_OK;
}

}  // extern "C"
