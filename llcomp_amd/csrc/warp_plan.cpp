// warp_plan.cpp -- the host planner of the warped views (warp_plan.hpp) and llcomp_mi_warp_reference.  Plain C++, no GPU.
#include "warp_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "warp_rule.hpp"

namespace llcomp_mi {

namespace {

bool warp_filter_ok(uint32_t filter) {
    return filter == LLCOMP_MI_FILTER_NEAREST || filter == LLCOMP_MI_FILTER_BILINEAR || filter == LLCOMP_MI_FILTER_BICUBIC;
}

// the first index in [0, n) for which a predicate that is false, ..., false, true, ..., true holds; n if none
template <class Pred>
uint32_t first_true(uint32_t n, const Pred& pred) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pred(mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}
// [a, b): the indices x of [0, n) with lo <= val(x) < hi, for val monotone in x -- not decreasing when up, not increasing otherwise
template <class T, class Val>
void range_where(uint32_t n, bool up, T lo, T hi, const Val& val, uint32_t& a, uint32_t& b) {
    if (up) {
        a = first_true(n, [&](uint32_t x) { return val(x) >= lo; });
        b = first_true(n, [&](uint32_t x) { return val(x) >= hi; });
    } else {
        a = first_true(n, [&](uint32_t x) { return val(x) < hi; });
        b = first_true(n, [&](uint32_t x) { return val(x) < lo; });
    }
}

// the bounding box of the taps seen so far, in frame coordinates, both ends inclusive
struct TapBox {
    int64_t x0 = INT64_MAX, y0 = INT64_MAX, x1 = -1, y1 = -1;
    void add(int64_t cx0, int64_t cx1, int64_t cy0, int64_t cy1) {
        x0 = std::min(x0, cx0);
        x1 = std::max(x1, cx1);
        y0 = std::min(y0, cy0);
        y1 = std::max(y1, cy1);
    }
    bool empty() const { return x1 < 0; }
};

void smooth_taps(const double* m, uint32_t filter, int32_t w, int32_t h, uint32_t x, uint32_t y, TapBox& box) {
    double xin, yin;
    warp_xy(m, x, y, xin, yin);
    const WarpTap t = warp_tap(xin, yin);
    if (filter == LLCOMP_MI_FILTER_BICUBIC)
        box.add(warp_cl(t.X - 1, w), warp_cl(t.X + 2, w), warp_cl(t.Y - 1, h), warp_cl(t.Y + 2, h));
    else
        box.add(warp_cl(t.X, w), warp_cl(t.X + 1, w), warp_cl(t.Y, h), warp_cl(t.Y + 1, h));
}

void smooth_rect(uint32_t w, uint32_t h, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, TapBox& box) {
    auto inside = [&](uint32_t x, uint32_t y) {
        double xin, yin;
        warp_xy(m, x, y, xin, yin);
        return warp_inside(xin, yin, w, h);
    };
    // all four corner pixels inside: every pixel is (each coordinate lies between its values at the corners), and the corners hold the extremes
    const bool all = inside(0, 0) && inside(ow - 1, 0) && inside(0, oh - 1) && inside(ow - 1, oh - 1);
    for (uint32_t y = 0; y < oh; y = (all && y + 1 < oh) ? oh - 1 : y + 1) {
        uint32_t a = 0, b = ow;
        if (!(inside(0, y) && inside(ow - 1, y))) {
            uint32_t ax, bx, ay, by;
            range_where<double>(ow, m[0] >= 0.0, 0.0, double(w), [&](uint32_t x) { double xi, yi; warp_xy(m, x, y, xi, yi); return xi; }, ax, bx);
            range_where<double>(ow, m[3] >= 0.0, 0.0, double(h), [&](uint32_t x) { double xi, yi; warp_xy(m, x, y, xi, yi); return yi; }, ay, by);
            a = std::max(ax, ay);
            b = std::min(bx, by);
        }
        if (a >= b) continue;
        smooth_taps(m, filter, int32_t(w), int32_t(h), a, y, box);
        smooth_taps(m, filter, int32_t(w), int32_t(h), b - 1, y, box);
    }
}

void fixed_rect(uint32_t w, uint32_t h, const double* m, uint32_t ow, uint32_t oh, TapBox& box) {
    int32_t A[6];
    warp_fixed_matrix(m, A);
    // without wrapping the 32-bit sums are linear in x and y: their extremes sit at the corner pixels
    auto wide = [&](int k, uint32_t x, uint32_t y) { return int64_t(A[k + 2]) + int64_t(x) * A[k] + int64_t(y) * A[k + 1]; };
    bool wraps = false;
    for (int k = 0; k < 6; k += 3)
        for (uint32_t corner = 0; corner < 4; ++corner) {
            const int64_t v = wide(k, corner & 1 ? ow - 1 : 0, corner & 2 ? oh - 1 : 0);
            wraps = wraps || v < INT32_MIN || v > INT32_MAX;
        }
    auto one = [&](uint32_t x, uint32_t y) {
        int32_t xi, yi;
        warp_fixed_xy(A, x, y, xi, yi);
        if (xi >= 0 && xi < int32_t(w) && yi >= 0 && yi < int32_t(h)) box.add(xi, xi, yi, yi);
    };
    if (wraps) {  // (only at the very edge of the limits: every pixel by itself)
        for (uint32_t y = 0; y < oh; ++y)
            for (uint32_t x = 0; x < ow; ++x) one(x, y);
        return;
    }
    for (uint32_t y = 0; y < oh; ++y) {
        uint32_t ax, bx, ay, by;
        range_where<int64_t>(ow, A[0] >= 0, 0, int64_t(w) << 16, [&](uint32_t x) { return wide(0, x, y); }, ax, bx);
        range_where<int64_t>(ow, A[3] >= 0, 0, int64_t(h) << 16, [&](uint32_t x) { return wide(3, x, y); }, ay, by);
        const uint32_t a = std::max(ax, ay), b = std::min(bx, by);
        if (a >= b) continue;
        one(a, y);
        one(b - 1, y);
    }
}

void scale_rect(uint32_t w, uint32_t h, const double* m, uint32_t ow, uint32_t oh, TapBox& box) {
    std::vector<int32_t> xi(ow), yi(oh);
    warp_scale_table(m[0], m[2], ow, w, xi.data());
    warp_scale_table(m[4], m[5], oh, h, yi.data());
    int64_t x0 = INT64_MAX, x1 = -1, y0 = INT64_MAX, y1 = -1;
    for (int32_t v : xi)
        if (v >= 0) x0 = std::min<int64_t>(x0, v), x1 = std::max<int64_t>(x1, v);
    for (int32_t v : yi)
        if (v >= 0) y0 = std::min<int64_t>(y0, v), y1 = std::max<int64_t>(y1, v);
    if (x1 >= 0 && y1 >= 0) box.add(x0, x1, y0, y1);
}

}  // namespace

uint64_t warp_view_term(const Geometry& g) { return sizeof(WarpEntry) + 4 * (uint64_t(g.w) + g.h) + g.c + 16 + 256 * 4 * uint64_t(g.c); }
uint64_t warp_tables_bound(const Geometry& g, uint64_t total_views) { return 48 + std::max<uint64_t>(total_views, 1) * warp_view_term(g); }

void WarpTail::put(uint8_t* at) const {
    std::memcpy(at, ws.data(), ws.size() * sizeof(WarpEntry));
    if (!tabs.empty()) std::memcpy(at + tabs_at(), tabs.data(), 4 * tabs.size());
    if (!fills.empty()) std::memcpy(at + fills_at(), fills.data(), fills.size());
    if (!tables.empty()) {
        std::memset(at + fills_at() + fills.size(), 0, size_t(tables_at() - fills_at() - fills.size()));
        std::memcpy(at + tables_at(), tables.data(), tables.size());
    }
}

int warp_check(const double* m, uint32_t filter, uint32_t ow, uint32_t oh) {
    if (!m || !ow || !oh || !warp_filter_ok(filter)) return LLCOMP_MI_BAD_ARGS;
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(m[i])) return LLCOMP_MI_BAD_ARGS;
    if (filter == LLCOMP_MI_FILTER_NEAREST) {
        for (uint32_t corner = 0; corner < 4; ++corner) {  // PIL's check_fixed
            const double p = corner & 1 ? double(ow) : 0.0, q = corner & 2 ? double(oh) : 0.0;
            const double a = p * m[0], b = q * m[1], d = p * m[3], e = q * m[4];
            const double x = (a + b) + m[2], y = (d + e) + m[5];
            if (!(std::fabs(x) < 32768.0 && std::fabs(y) < 32768.0)) return LLCOMP_MI_BAD_ARGS;
        }
        return LLCOMP_MI_OK;
    }
    for (uint32_t corner = 0; corner < 4; ++corner) {
        double xin, yin;
        warp_xy(m, corner & 1 ? ow - 1 : 0, corner & 2 ? oh - 1 : 0, xin, yin);
        if (!(std::fabs(xin) < 1073741824.0 && std::fabs(yin) < 1073741824.0)) return LLCOMP_MI_BAD_ARGS;
    }
    return LLCOMP_MI_OK;
}

int warp_source_rect(uint32_t w, uint32_t h, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4], bool& empty) {
    if (!w || !h || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || !rect) return LLCOMP_MI_BAD_ARGS;
    if (int rc = warp_check(m, filter, ow, oh)) return rc;
    TapBox box;
    if (filter != LLCOMP_MI_FILTER_NEAREST)
        smooth_rect(w, h, m, filter, ow, oh, box);
    else if (warp_is_scale(m))
        scale_rect(w, h, m, ow, oh, box);
    else
        fixed_rect(w, h, m, ow, oh, box);
    empty = box.empty();
    rect[0] = empty ? 0 : uint32_t(box.x0);
    rect[1] = empty ? 0 : uint32_t(box.y0);
    rect[2] = empty ? 0 : uint32_t(box.x1 - box.x0 + 1);
    rect[3] = empty ? 0 : uint32_t(box.y1 - box.y0 + 1);
    return LLCOMP_MI_OK;
}

int warp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, const uint8_t* fill, uint32_t ow,
                   uint32_t oh, uint8_t* out) {
    if (!src || !out || !w || !h || !c || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return LLCOMP_MI_BAD_ARGS;
    if (int rc = warp_check(m, filter, ow, oh)) return rc;
    const bool scale = filter == LLCOMP_MI_FILTER_NEAREST && warp_is_scale(m);
    std::vector<int32_t> xt, yt;
    int32_t A[6] = {};
    if (scale) {
        xt.resize(ow);
        yt.resize(oh);
        warp_scale_table(m[0], m[2], ow, w, xt.data());
        warp_scale_table(m[4], m[5], oh, h, yt.data());
    } else if (filter == LLCOMP_MI_FILTER_NEAREST) {
        warp_fixed_matrix(m, A);
    }
    for (uint32_t y = 0; y < oh; ++y)
        for (uint32_t x = 0; x < ow; ++x) {
            uint8_t* o = out + (size_t(y) * ow + x) * c;
            if (filter == LLCOMP_MI_FILTER_NEAREST) {
                int32_t xi, yi;
                if (scale)
                    xi = xt[x], yi = yt[y];
                else
                    warp_fixed_xy(A, x, y, xi, yi);
                const bool in = xi >= 0 && xi < int32_t(w) && yi >= 0 && yi < int32_t(h);
                for (uint32_t ch = 0; ch < c; ++ch) o[ch] = in ? src[(size_t(yi) * w + uint32_t(xi)) * c + ch] : (fill ? fill[ch] : 0);
                continue;
            }
            double xin, yin;
            warp_xy(m, x, y, xin, yin);
            if (!warp_inside(xin, yin, w, h)) {
                for (uint32_t ch = 0; ch < c; ++ch) o[ch] = fill ? fill[ch] : 0;
                continue;
            }
            const WarpTap t = warp_tap(xin, yin);
            for (uint32_t ch = 0; ch < c; ++ch) {
                auto P = [&](int32_t row, int32_t col) { return double(src[(size_t(row) * w + uint32_t(col)) * c + ch]); };
                o[ch] = uint8_t(filter == LLCOMP_MI_FILTER_BICUBIC ? warp_bicubic(P, t, int32_t(w), int32_t(h)) : warp_bilinear(P, t, int32_t(w), int32_t(h)));
            }
        }
    return LLCOMP_MI_OK;
}

static const llcomp_mi_warp_group* warp_group_at(const llcomp_mi_warp_group* groups, uint32_t i) {
    return reinterpret_cast<const llcomp_mi_warp_group*>(reinterpret_cast<const uint8_t*>(groups) + size_t(i) * groups->struct_size);
}

int warp_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_warp_group* groups, uint32_t n_groups, ViewsUnion& u,
               std::vector<uint32_t>& rects, uint64_t& total_views) {
    u = ViewsUnion{};
    rects.clear();
    total_views = 0;
    if (!groups || !n_groups || !frames || !w || !h || groups->struct_size != sizeof(llcomp_mi_warp_group)) return LLCOMP_MI_BAD_ARGS;
    // every view that reads pixels as a rectangle view of its own group, at its own size: what views_union takes the unions of
    std::vector<llcomp_mi_view> sviews;
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_warp_group& gr = *warp_group_at(groups, gi);
        if (gr.struct_size != sizeof(llcomp_mi_warp_group) || !gr.n_views || gr.n_views > 65535 || !gr.views || !gr.ow || !gr.oh)
            return LLCOMP_MI_BAD_ARGS;
        for (uint32_t i = 0; i < gr.n_views; ++i) {
            const llcomp_mi_warp_view& v = gr.views[i];
            uint32_t r[4];
            bool empty = true;
            if (v.frame >= frames) return LLCOMP_MI_BAD_ARGS;
            if (int rc = warp_source_rect(w, h, v.m, LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu), gr.ow, gr.oh, r, empty)) return rc;
            rects.insert(rects.end(), {r[0], r[1], r[2], r[3], empty ? 1u : 0u});
            if (!empty) sviews.push_back(llcomp_mi_view{v.frame, r[0], r[1], r[2], r[3], LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_NEAREST)});
        }
        total_views += gr.n_views;
    }
    u.rects.assign(4 * size_t(frames), 0);
    if (sviews.empty()) return LLCOMP_MI_OK;
    std::vector<llcomp_mi_view_group> sgroups(sviews.size());
    for (size_t i = 0; i < sviews.size(); ++i)
        sgroups[i] = llcomp_mi_view_group{uint32_t(sizeof(llcomp_mi_view_group)), 1, &sviews[i], sviews[i].rw, sviews[i].rh, nullptr, nullptr};
    return views_union(w, h, frames, sgroups.data(), uint32_t(sgroups.size()), u);
}

int warp_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_warp_group* groups, uint32_t n_groups, WarpPlan& p) {
    std::vector<uint32_t> rects;
    if (int rc = warp_union(g.w, g.h, g.frames, groups, n_groups, p.u, rects, p.total_views)) return rc;
    std::vector<WarpOut>& out = p.tail.groups;
    out.resize(n_groups);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_warp_group& gr = *warp_group_at(groups, gi);
        if (int rc = check_output_format(gr.fmt, g.c, out[gi].out)) return rc;
        if (!gr.d_out || (reinterpret_cast<uintptr_t>(gr.d_out) & (out[gi].out.esize - 1))) return LLCOMP_MI_BAD_ARGS;
    }
    const uint32_t n_used = uint32_t(p.u.used.size());
    p.wmax = p.u.wmax;
    p.hmax = p.u.hmax;
    p.tab.resize(n_used);
    if (n_used)
        if (int rc = regions_setup_sized(g, tune, p.u.rects.data(), p.wmax, p.hmax, p.tab.data(), p.classes, p.n_classes, p.u.used.data(), n_used))
            return rc;
    std::vector<uint32_t> entry_of(g.frames, 0);  // a used frame's entry of the regions table
    for (uint32_t i = 0; i < n_used; ++i) entry_of[p.tab[i].frame] = i;
    WarpTail& t = p.tail;
    t.ws.reserve(size_t(p.total_views));
    const uint32_t* r = rects.data();
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_warp_group& gr = *warp_group_at(groups, gi);
        WarpOut& vg = out[gi];
        vg.n = gr.n_views;
        vg.ow = gr.ow;
        vg.oh = gr.oh;
        vg.d_out = gr.d_out;
        vg.first = uint32_t(t.ws.size());
        for (uint32_t i = 0; i < gr.n_views; ++i, r += 5) {
            const llcomp_mi_warp_view& v = gr.views[i];
            const uint32_t filter = LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu);
            WarpEntry z;
            std::memset(&z, 0, sizeof z);
            uint32_t form = kWarpEmpty;
            if (!r[4]) {
                const RegionsFrame& e = p.tab[entry_of[v.frame]];
                const uint64_t bx = uint64_t(e.wx0) * g.tile_w + e.cx0, by = uint64_t(e.wy0) * g.tile_h + e.cy0;
                // (the box holds the union, and the union the view's source rectangle, by construction)
                if (e.frame != v.frame || r[0] < bx || r[1] < by || uint64_t(r[0]) + r[2] > bx + p.wmax || uint64_t(r[1]) + r[3] > by + p.hmax ||
                    e.out >= n_used)
                    return LLCOMP_MI_HIP_ERROR;
                z.bx = int32_t(bx);
                z.by = int32_t(by);
                z.box = e.out;
                if (filter != LLCOMP_MI_FILTER_NEAREST) {
                    form = kWarpSmooth;
                    std::memcpy(z.m, v.m, sizeof z.m);
                } else if (warp_is_scale(v.m)) {
                    form = kWarpTable;
                    z.t[0] = uint32_t(t.tabs.size());
                    z.t[1] = z.t[0] + gr.ow;
                    t.tabs.resize(t.tabs.size() + gr.ow + gr.oh);
                    warp_scale_table(v.m[0], v.m[2], gr.ow, g.w, t.tabs.data() + z.t[0]);
                    warp_scale_table(v.m[4], v.m[5], gr.oh, g.h, t.tabs.data() + z.t[1]);
                } else {
                    form = kWarpFixed;
                    warp_fixed_matrix(v.m, z.a);
                }
            }
            z.flags = (v.flags & (1u | LLCOMP_MI_FLAG_FILTER_MASK)) | (form << kWarpFormShift);
            t.ws.push_back(z);
        }
        vg.fill_at = uint32_t(t.fills.size());
        for (uint32_t ch = 0; ch < g.c; ++ch) t.fills.push_back(gr.fill ? gr.fill[ch] : 0);
        if (!vg.out.plain) {
            const size_t at = (t.tables.size() + 15) & ~size_t(15);
            t.tables.resize(at + vg.out.table_bytes(g.c));
            output_table(gr.fmt, g.c, vg.out, t.tables.data() + at);
            vg.table_at = at;
        }
    }
    t.box_bytes = uint64_t(n_used) * p.wmax * p.hmax * g.c;
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

int llcomp_mi_warp_source_rect(uint32_t w, uint32_t h, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4], uint32_t* empty) {
    uint32_t r[4];
    bool e = true;
    if (!rect || !empty) return LLCOMP_MI_BAD_ARGS;
    if (int rc = llcomp_mi::warp_source_rect(w, h, m, filter, ow, oh, r, e)) return rc;
    std::memcpy(rect, r, sizeof r);
    *empty = e ? 1u : 0u;
    return LLCOMP_MI_OK;
}

int llcomp_mi_warp_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                              const llcomp_mi_warp_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows, uint32_t* n_used,
                              uint32_t* n_classes) {
    if (!n_used || !n_classes || c < 1 || c > llcomp_mi::kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    llcomp_mi::ViewsUnion u;
    std::vector<uint32_t> rects;
    uint64_t total = 0;
    if (int rc = llcomp_mi::warp_union(w, h, frames, groups, n_groups, u, rects, total)) return rc;
    if (u.used.empty()) {  // every view is all fill: nothing is decoded
        if (unions) std::memset(unions, 0, 16 * size_t(frames));
        if (windows) std::memset(windows, 0, 16 * size_t(frames));
        *n_used = *n_classes = 0;
        return LLCOMP_MI_OK;
    }
    // the unions as one rectangle view per used frame: the windows and classes are llcomp_mi_views_plan's for them
    std::vector<llcomp_mi_view> views;
    for (uint32_t f : u.used) {
        const uint32_t* r = u.rects.data() + 4 * size_t(f);
        views.push_back(llcomp_mi_view{f, r[0], r[1], r[2], r[3], LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_NEAREST)});
    }
    std::vector<llcomp_mi_view_group> sg(views.size());
    for (size_t i = 0; i < views.size(); ++i)
        sg[i] = llcomp_mi_view_group{uint32_t(sizeof(llcomp_mi_view_group)), 1, &views[i], views[i].rw, views[i].rh, nullptr, nullptr};
    return llcomp_mi_views_plan(w, h, c, tile_w, tile_h, planar, frames, sg.data(), uint32_t(sg.size()), unions, windows, n_used, n_classes);
}

int llcomp_mi_warp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, const uint8_t* fill,
                             uint32_t ow, uint32_t oh, uint8_t* out) {
    return llcomp_mi::warp_reference(src, w, h, c, m, filter, fill, ow, oh, out);
}

}  // extern "C"
