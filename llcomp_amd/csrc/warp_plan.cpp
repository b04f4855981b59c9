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

// ---- perspective views ----

// first_true started at a guess: it gallops from `near` (probes 1, 2, 4, ... indices away) to an index on the other side of the answer and
// bisects between the two, so it costs O(log(1 + the distance from the guess)) evaluations.  As first_true, it ends between an index
// SEEN false (or the start) and one SEEN true (or n).
template <class Pred>
uint32_t first_true_near(uint32_t n, uint32_t near, const Pred& pred) {
    uint32_t lo = 0, hi = n;  // lo - 1 was seen false (or lo == 0), hi was seen true (or hi == n)
    if (!n) return 0;
    const uint32_t at = std::min(near, n - 1);
    if (pred(at)) {
        hi = at;
        for (uint64_t step = 1; hi > 0; step *= 2) {
            const uint32_t probe = hi > step ? uint32_t(hi - step) : 0;
            if (!pred(probe)) {
                lo = probe + 1;
                break;
            }
            hi = probe;
        }
    } else {
        lo = at + 1;
        for (uint64_t step = 1; lo < n; step *= 2) {
            const uint32_t probe = uint32_t(std::min<uint64_t>(lo - 1 + step, n - 1));
            if (pred(probe)) {
                hi = probe;
                break;
            }
            lo = probe + 1;
        }
    }
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pred(mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}
// range_where with the answers of the row before as guesses (ab: in and out)
template <class Val>
void range_near(uint32_t n, bool up, double lo, double hi, const Val& val, uint32_t ab[2]) {
    if (up) {
        ab[0] = first_true_near(n, ab[0], [&](uint32_t x) { return val(x) >= lo; });
        ab[1] = first_true_near(n, ab[1], [&](uint32_t x) { return val(x) >= hi; });
    } else {
        ab[0] = first_true_near(n, ab[0], [&](uint32_t x) { return val(x) < hi; });
        ab[1] = first_true_near(n, ab[1], [&](uint32_t x) { return val(x) < lo; });
    }
}

// the taps of one pixel under the perspective rule, `wide` more pixels on every side, clamped into the image
void persp_taps(const double* a, uint32_t filter, int32_t w, int32_t h, uint32_t x, uint32_t y, int32_t wide, TapBox& box) {
    double xin, yin;
    persp_xy(a, x, y, xin, yin);
    // (a pixel that is inside only up to the planner's margin may lie a hair outside the image: what is converted is clamped first)
    const double cx = std::min(std::max(xin, -2.0), double(w) + 2.0), cy = std::min(std::max(yin, -2.0), double(h) + 2.0);
    int64_t x0, x1, y0, y1;
    if (filter == LLCOMP_MI_FILTER_NEAREST) {
        x0 = x1 = int64_t(std::floor(cx));
        y0 = y1 = int64_t(std::floor(cy));
    } else {
        const double fx = std::floor(cx - 0.5), fy = std::floor(cy - 0.5);  // (warp_tap's origin, in 64 bits: w + 2 need not fit 32)
        const int64_t back = filter == LLCOMP_MI_FILTER_BICUBIC ? 1 : 0;
        x0 = int64_t(fx) - back, x1 = int64_t(fx) + 1 + back, y0 = int64_t(fy) - back, y1 = int64_t(fy) + 1 + back;
    }
    auto cl = [](int64_t t, int64_t n) { return std::min(std::max<int64_t>(t, 0), n - 1); };
    box.add(cl(x0 - wide, w), cl(x1 + wide, w), cl(y0 - wide, h), cl(y1 + wide, h));
}

// The source rectangle of a perspective view: a bound.  With N1, N2, D the rule's two numerators and its denominator as computed,
// n1, n2, d the same sums in real arithmetic and q = n / d:
//   * each of N1, N2, D differs from its real sum by at most 3 u (|c0| ow + |c1| oh + |c2|), u = 2^-53.  The FAST PATH requires
//     M = (that sum for n1) + (for n2) + (w + h + 2) (that sum for d) <= 2^30 Dmin, Dmin the least computed denominator of the four
//     corner pixels (the rounded D is monotone in x and in y, so no pixel's is smaller).  Then d > 0 everywhere, and wherever |q| <= w + h + 2
//     the computed coordinate Q is within delta = 2^-20 of q; elsewhere the relative error is that small and Q is outside as q is.
//   * with d > 0, q1 and q2 are EXACTLY monotone along an output row.  So the pixels of a row with -2 delta <= q < n + 2 delta on both
//     axes are one interval, which holds every pixel the rule calls inside.  It is bisected on the computed Q with the thresholds
//     -4 delta and n + 4 delta: a bisection ends between an index seen below the threshold and one seen at or above it, and what is
//     seen below -4 delta has q < -3 delta, so by monotony of q every index on that side is outside.  A row whose two ends differ by
//     less than 16 delta is not bisected: all of it is taken.  Each of the four searches of a row starts at the answer of the row
//     before (first_true_near): where one edge of the image crosses the rows is a straight line in the output, its index moves one
//     way from row to row and by at most ow in all, and a search costs O(log(1 + its move)) <= O(1 + its move) evaluations -- O(ow + oh)
//     per view.
//   * from both ends of that interval the pixels the rule calls outside are walked off one by one -- normally none or one, a whole
//     row only where a row's image runs along the image's edge within 2^-17 of it -- so [a, b) starts and ends with an inside pixel
//     and the rectangle is empty exactly when no pixel is inside.
//   * q1 and q2 of every pixel of [a, b) lie between their values at a and b - 1, so Q lies within delta of the span of Q(a) and
//     Q(b - 1), and every tap origin floor(Q - 0.5), or index trunc(Q), within ONE of theirs: the taps of a and b - 1, one pixel
//     wider on every side and clamped to the image, contain the taps of every inside pixel of the row.  A superset, and on no side
//     more than a pixel beyond the taps of an inside pixel.
// A map beyond the fast path's condition (a denominator all but cancelled) walks every pixel.
void persp_rect(uint32_t w, uint32_t h, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, TapBox& box) {
    const int32_t iw = int32_t(w), ih = int32_t(h);
    auto inside = [&](uint32_t x, uint32_t y) {
        double xin, yin;
        persp_xy(a, x, y, xin, yin);
        return warp_inside(xin, yin, w, h);
    };
    double dmin = persp_den(a, 0, 0);
    for (uint32_t corner = 1; corner < 4; ++corner) dmin = std::min(dmin, persp_den(a, corner & 1 ? ow - 1 : 0, corner & 2 ? oh - 1 : 0));
    auto mag = [&](int k, double c2) { return std::fabs(a[k]) * double(ow) + std::fabs(a[k + 1]) * double(oh) + c2; };
    const double M = mag(0, std::fabs(a[2])) + mag(3, std::fabs(a[5])) + (double(w) + double(h) + 2.0) * mag(6, 1.0);
    if (!(M <= dmin * 1073741824.0)) {
        for (uint32_t y = 0; y < oh; ++y)
            for (uint32_t x = 0; x < ow; ++x)
                if (inside(x, y)) persp_taps(a, filter, iw, ih, x, y, 0, box);
        return;
    }
    // all four corner pixels inside: the coordinates of every pixel lie between the corners' (monotone along rows and columns)
    if (inside(0, 0) && inside(ow - 1, 0) && inside(0, oh - 1) && inside(ow - 1, oh - 1)) {
        for (uint32_t corner = 0; corner < 4; ++corner) persp_taps(a, filter, iw, ih, corner & 1 ? ow - 1 : 0, corner & 2 ? oh - 1 : 0, 1, box);
        return;
    }
    constexpr double delta = 1.0 / 1048576.0;
    uint32_t near[2][2] = {{0, ow}, {0, ow}};  // per axis: where the row before entered and left the image
    for (uint32_t y = 0; y < oh; ++y) {
        uint32_t lo = 0, hi = ow;
        for (int axis = 0; axis < 2; ++axis) {
            auto val = [&](uint32_t x) {
                double xin, yin;
                persp_xy(a, x, y, xin, yin);
                return axis ? yin : xin;
            };
            const double t0 = -4.0 * delta, t1 = double(axis ? h : w) + 4.0 * delta, e0 = val(0), e1 = val(ow - 1);
            if (std::fabs(e1 - e0) < 16.0 * delta) {
                if (std::max(e0, e1) < t0 - delta || std::min(e0, e1) >= t1 + delta) lo = hi;  // (the whole row is outside)
                continue;
            }
            range_near(ow, e1 > e0, t0, t1, val, near[axis]);
            lo = std::max(lo, near[axis][0]);
            hi = std::min(hi, near[axis][1]);
        }
        while (lo < hi && !inside(lo, y)) ++lo;
        while (lo < hi && !inside(hi - 1, y)) --hi;
        if (lo >= hi) continue;
        persp_taps(a, filter, iw, ih, lo, y, 1, box);
        persp_taps(a, filter, iw, ih, hi - 1, y, 1, box);
    }
}

}  // namespace

uint64_t persp_tables_bound(const Geometry& g, uint64_t total_views) {
    return warp_tables_bound(g, total_views) + std::max<uint64_t>(total_views, 1) * (sizeof(PerspEntry) - sizeof(WarpEntry));
}

int persp_check(const double* a, uint32_t filter, uint32_t ow, uint32_t oh) {
    if (!a || !ow || !oh || !warp_filter_ok(filter)) return LLCOMP_MI_BAD_ARGS;
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(a[i])) return LLCOMP_MI_BAD_ARGS;
    for (uint32_t corner = 0; corner < 4; ++corner) {
        const uint32_t x = corner & 1 ? ow - 1 : 0, y = corner & 2 ? oh - 1 : 0;
        double xin, yin;
        if (!(persp_den(a, x, y) > 0.0)) return LLCOMP_MI_BAD_ARGS;
        persp_xy(a, x, y, xin, yin);
        if (!(std::fabs(xin) < 1073741824.0 && std::fabs(yin) < 1073741824.0)) return LLCOMP_MI_BAD_ARGS;
    }
    return LLCOMP_MI_OK;
}

int persp_source_rect(uint32_t w, uint32_t h, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4], bool& empty) {
    if (!w || !h || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || !rect) return LLCOMP_MI_BAD_ARGS;
    if (int rc = persp_check(a, filter, ow, oh)) return rc;
    TapBox box;
    persp_rect(w, h, a, filter, ow, oh, box);
    empty = box.empty();
    rect[0] = empty ? 0 : uint32_t(box.x0);
    rect[1] = empty ? 0 : uint32_t(box.y0);
    rect[2] = empty ? 0 : uint32_t(box.x1 - box.x0 + 1);
    rect[3] = empty ? 0 : uint32_t(box.y1 - box.y0 + 1);
    return LLCOMP_MI_OK;
}

int persp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* a, uint32_t filter, const uint8_t* fill, uint32_t ow,
                    uint32_t oh, uint8_t* out) {
    if (!src || !out || !w || !h || !c || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return LLCOMP_MI_BAD_ARGS;
    if (int rc = persp_check(a, filter, ow, oh)) return rc;
    for (uint32_t y = 0; y < oh; ++y)
        for (uint32_t x = 0; x < ow; ++x) {
            uint8_t* o = out + (size_t(y) * ow + x) * c;
            double xin, yin;
            persp_xy(a, x, y, xin, yin);
            if (filter == LLCOMP_MI_FILTER_NEAREST) {
                const int32_t xi = persp_index(xin, w), yi = persp_index(yin, h);
                const bool in = xi >= 0 && yi >= 0;
                for (uint32_t ch = 0; ch < c; ++ch) o[ch] = in ? src[(size_t(yi) * w + uint32_t(xi)) * c + ch] : (fill ? fill[ch] : 0);
                continue;
            }
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

uint64_t warp_view_term(const Geometry& g) { return sizeof(WarpEntry) + 4 * (uint64_t(g.w) + g.h) + g.c + 16 + 256 * 4 * uint64_t(g.c); }
uint64_t warp_tables_bound(const Geometry& g, uint64_t total_views) { return 48 + std::max<uint64_t>(total_views, 1) * warp_view_term(g); }

void WarpTail::put(uint8_t* at) const {
    if (!ws.empty()) std::memcpy(at, ws.data(), ws.size() * sizeof(WarpEntry));
    if (!ps.empty()) std::memcpy(at + ws.size() * sizeof(WarpEntry), ps.data(), ps.size() * sizeof(PerspEntry));
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

namespace {

// The two kinds of group -- llcomp_mi_warp_group and llcomp_mi_perspective_group, the same fields around their own view type -- go
// through ONE union and ONE setup; what differs is a view's source rectangle and the entry it stages.
template <class Group>
const Group* warp_group_at(const Group* groups, uint32_t i) {
    return reinterpret_cast<const Group*>(reinterpret_cast<const uint8_t*>(groups) + size_t(i) * groups->struct_size);
}
int view_rect(uint32_t w, uint32_t h, const llcomp_mi_warp_view& v, uint32_t ow, uint32_t oh, uint32_t r[4], bool& empty) {
    return warp_source_rect(w, h, v.m, LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu), ow, oh, r, empty);
}
int view_rect(uint32_t w, uint32_t h, const llcomp_mi_perspective_view& v, uint32_t ow, uint32_t oh, uint32_t r[4], bool& empty) {
    return persp_source_rect(w, h, v.a, LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu), ow, oh, r, empty);
}
// the entry of one view: box == nullptr for a view that reads no pixel, else {bx, by, box}
void push_entry(WarpTail& t, const Geometry& g, const llcomp_mi_warp_view& v, uint32_t ow, uint32_t oh, const uint32_t* box) {
    const uint32_t filter = LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu);
    WarpEntry z;
    std::memset(&z, 0, sizeof z);
    uint32_t form = kWarpEmpty;
    if (box) {
        z.bx = int32_t(box[0]);
        z.by = int32_t(box[1]);
        z.box = box[2];
        if (filter != LLCOMP_MI_FILTER_NEAREST) {
            form = kWarpSmooth;
            std::memcpy(z.m, v.m, sizeof z.m);
        } else if (warp_is_scale(v.m)) {
            form = kWarpTable;
            z.t[0] = uint32_t(t.tabs.size());
            z.t[1] = z.t[0] + ow;
            t.tabs.resize(t.tabs.size() + ow + oh);
            warp_scale_table(v.m[0], v.m[2], ow, g.w, t.tabs.data() + z.t[0]);
            warp_scale_table(v.m[4], v.m[5], oh, g.h, t.tabs.data() + z.t[1]);
        } else {
            form = kWarpFixed;
            warp_fixed_matrix(v.m, z.a);
        }
    }
    z.flags = (v.flags & (1u | LLCOMP_MI_FLAG_FILTER_MASK)) | (form << kWarpFormShift);
    t.ws.push_back(z);
}
void push_entry(WarpTail& t, const Geometry&, const llcomp_mi_perspective_view& v, uint32_t, uint32_t, const uint32_t* box) {
    PerspEntry z;
    std::memset(&z, 0, sizeof z);
    std::memcpy(z.a, v.a, sizeof z.a);
    if (box) {
        z.bx = int32_t(box[0]);
        z.by = int32_t(box[1]);
        z.box = box[2];
    }
    z.flags = (v.flags & (1u | LLCOMP_MI_FLAG_FILTER_MASK)) | (box ? 0u : kPerspEmpty);
    t.ps.push_back(z);
}

template <class Group>
int union_of(uint32_t w, uint32_t h, uint32_t frames, const Group* groups, uint32_t n_groups, ViewsUnion& u, std::vector<uint32_t>& rects,
             uint64_t& total_views) {
    u = ViewsUnion{};
    rects.clear();
    total_views = 0;
    if (!groups || !n_groups || !frames || !w || !h || groups->struct_size != sizeof(Group)) return LLCOMP_MI_BAD_ARGS;
    // every view that reads pixels as a rectangle view of its own group, at its own size: what views_union takes the unions of
    std::vector<llcomp_mi_view> sviews;
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const Group& gr = *warp_group_at(groups, gi);
        if (gr.struct_size != sizeof(Group) || !gr.n_views || gr.n_views > 65535 || !gr.views || !gr.ow || !gr.oh)
            return LLCOMP_MI_BAD_ARGS;
        for (uint32_t i = 0; i < gr.n_views; ++i) {
            const auto& v = gr.views[i];
            uint32_t r[4];
            bool empty = true;
            if (v.frame >= frames) return LLCOMP_MI_BAD_ARGS;
            if (int rc = view_rect(w, h, v, gr.ow, gr.oh, r, empty)) return rc;
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

template <class Group>
int setup_of(const Geometry& g, const Tuning& tune, const Group* groups, uint32_t n_groups, WarpPlan& p) {
    std::vector<uint32_t> rects;
    if (int rc = union_of(g.w, g.h, g.frames, groups, n_groups, p.u, rects, p.total_views)) return rc;
    std::vector<WarpOut>& out = p.tail.groups;
    out.resize(n_groups);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const Group& gr = *warp_group_at(groups, gi);
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
    const uint32_t* r = rects.data();
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const Group& gr = *warp_group_at(groups, gi);
        WarpOut& vg = out[gi];
        vg.n = gr.n_views;
        vg.ow = gr.ow;
        vg.oh = gr.oh;
        vg.d_out = gr.d_out;
        vg.first = uint32_t(t.ws.size() + t.ps.size());
        for (uint32_t i = 0; i < gr.n_views; ++i, r += 5) {
            const auto& v = gr.views[i];
            if (r[4]) {
                push_entry(t, g, v, gr.ow, gr.oh, nullptr);
                continue;
            }
            const RegionsFrame& e = p.tab[entry_of[v.frame]];
            const uint64_t bx = uint64_t(e.wx0) * g.tile_w + e.cx0, by = uint64_t(e.wy0) * g.tile_h + e.cy0;
            // (the box holds the union, and the union the view's source rectangle, by construction)
            if (e.frame != v.frame || r[0] < bx || r[1] < by || uint64_t(r[0]) + r[2] > bx + p.wmax || uint64_t(r[1]) + r[3] > by + p.hmax ||
                e.out >= n_used)
                return LLCOMP_MI_HIP_ERROR;
            const uint32_t box[3] = {uint32_t(bx), uint32_t(by), e.out};
            push_entry(t, g, v, gr.ow, gr.oh, box);
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

// the unions as one rectangle view per used frame: the windows and classes are llcomp_mi_views_plan's for them
int plan_of_union(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames, const ViewsUnion& u,
                  uint32_t* unions, uint32_t* windows, uint32_t* n_used, uint32_t* n_classes) {
    if (u.used.empty()) {  // every view is all fill: nothing is decoded
        if (unions) std::memset(unions, 0, 16 * size_t(frames));
        if (windows) std::memset(windows, 0, 16 * size_t(frames));
        *n_used = *n_classes = 0;
        return LLCOMP_MI_OK;
    }
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

}  // namespace

int warp_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_warp_group* groups, uint32_t n_groups, ViewsUnion& u,
               std::vector<uint32_t>& rects, uint64_t& total_views) {
    return union_of(w, h, frames, groups, n_groups, u, rects, total_views);
}
int warp_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_warp_group* groups, uint32_t n_groups, WarpPlan& p) {
    return setup_of(g, tune, groups, n_groups, p);
}
int persp_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_perspective_group* groups, uint32_t n_groups, ViewsUnion& u,
                std::vector<uint32_t>& rects, uint64_t& total_views) {
    return union_of(w, h, frames, groups, n_groups, u, rects, total_views);
}
int persp_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_perspective_group* groups, uint32_t n_groups, WarpPlan& p) {
    return setup_of(g, tune, groups, n_groups, p);
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
    return llcomp_mi::plan_of_union(w, h, c, tile_w, tile_h, planar, frames, u, unions, windows, n_used, n_classes);
}

int llcomp_mi_warp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, const uint8_t* fill,
                             uint32_t ow, uint32_t oh, uint8_t* out) {
    return llcomp_mi::warp_reference(src, w, h, c, m, filter, fill, ow, oh, out);
}

int llcomp_mi_perspective_source_rect(uint32_t w, uint32_t h, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4],
                                      uint32_t* empty) {
    uint32_t r[4];
    bool e = true;
    if (!rect || !empty) return LLCOMP_MI_BAD_ARGS;
    if (int rc = llcomp_mi::persp_source_rect(w, h, a, filter, ow, oh, r, e)) return rc;
    std::memcpy(rect, r, sizeof r);
    *empty = e ? 1u : 0u;
    return LLCOMP_MI_OK;
}

int llcomp_mi_perspective_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                                     const llcomp_mi_perspective_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows,
                                     uint32_t* n_used, uint32_t* n_classes) {
    if (!n_used || !n_classes || c < 1 || c > llcomp_mi::kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    llcomp_mi::ViewsUnion u;
    std::vector<uint32_t> rects;
    uint64_t total = 0;
    if (int rc = llcomp_mi::persp_union(w, h, frames, groups, n_groups, u, rects, total)) return rc;
    return llcomp_mi::plan_of_union(w, h, c, tile_w, tile_h, planar, frames, u, unions, windows, n_used, n_classes);
}

int llcomp_mi_perspective_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* a, uint32_t filter, const uint8_t* fill,
                                    uint32_t ow, uint32_t oh, uint8_t* out) {
    return llcomp_mi::persp_reference(src, w, h, c, a, filter, fill, ow, oh, out);
}

}  // extern "C"
