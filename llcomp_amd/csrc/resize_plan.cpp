// resize_plan.cpp -- the host half of the resampling (resize_plan.hpp): the filters' weights in Q22, the checked output format and its
// table.  Plain C++: the planner (windows_plan.cpp) links it without a HIP compiler.  The rule is include/llcomp_mi.h's
// llcomp_mi_resize_filter_weights; the GPU runs exactly the weights resize_weights computes.
#include "resize_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace llcomp_mi {

// The filters' kernel functions, as PIL's Resample.c states them (operation for operation: the weights are compared bit for bit).
static double f_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
static double f_triangle(double x) { return std::max(0.0, 1.0 - std::fabs(x)); }
static double f_hamming(double x) {
    x = std::fabs(x);
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return std::sin(x) / x * (0.54 + 0.46 * std::cos(x));
}
static double f_bicubic(double x) {
    constexpr double a = -0.5;
    x = std::fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double f_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
static double f_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? f_sinc(x) * f_sinc(x / 3) : 0.0; }

struct FilterRule {
    double (*f)(double);
    double radius;  // S: the kernel function's support at scale 1 (geometry.hpp: resize_axis_ok keeps S * max(scale, 1) <= kResizeMaxDown)
};
static const FilterRule* filter_rule(uint32_t filter) {
    static const FilterRule kRules[kResizeFilters] = {{f_triangle, 1.0}, {nullptr, 0.0}, {f_box, 0.5}, {f_hamming, 1.0}, {f_bicubic, 2.0}, {f_lanczos, 3.0}};
    return filter < kResizeFilters ? &kRules[filter] : nullptr;
}

// One pass over the outputs: every output's lo and its Q22 run (at most `span` taps) into lo_all / q_all, and K.
static uint32_t weights_pass(uint32_t filter, uint32_t in_len, uint32_t out_len, std::vector<uint32_t>& lo_all, std::vector<int32_t>& q_all,
                             uint32_t& span) {
    lo_all.resize(out_len);
    if (filter == LLCOMP_MI_FILTER_NEAREST) {  // (the centre-aligned rule in exact integers: one tap of 1.0)
        span = 1;
        q_all.assign(out_len, 1 << 22);
        for (uint32_t i = 0; i < out_len; ++i) lo_all[i] = uint32_t((2 * uint64_t(i) + 1) * in_len / (2 * uint64_t(out_len)));
        return 1;
    }
    const FilterRule& r = *filter_rule(filter);
    const double scale = double(in_len) / double(out_len), support = r.radius * std::max(scale, 1.0), ss = 1.0 / std::max(scale, 1.0);
    span = uint32_t(std::ceil(2.0 * support)) + 2;  // (support <= kResizeMaxDown: resize_axis_ok)
    q_all.assign(size_t(out_len) * span, 0);
    double w[2 * kResizeMaxDown + 4];
    uint32_t k = 1;
    for (uint32_t i = 0; i < out_len; ++i) {
        const double center = (i + 0.5) * scale;
        const int64_t a = std::max<int64_t>(int64_t(center - support + 0.5), 0);
        const int64_t b = std::min<int64_t>(int64_t(center + support + 0.5), in_len);
        const uint32_t n = uint32_t(std::min<int64_t>(std::max<int64_t>(b - a, 0), span));
        double sum = 0.0;
        for (uint32_t j = 0; j < n; ++j) {
            w[j] = r.f((double(a + int64_t(j)) - center + 0.5) * ss);
            sum += w[j];
        }
        int32_t* q = q_all.data() + size_t(i) * span;
        uint32_t last = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const double v = sum != 0.0 ? w[j] / sum : w[j];
            q[j] = v < 0.0 ? int32_t(-0.5 + v * double(1 << 22)) : int32_t(0.5 + v * double(1 << 22));  // (both truncate toward zero)
            if (q[j]) last = j + 1;
        }
        lo_all[i] = uint32_t(a);
        k = std::max(k, last);
    }
    return k;
}

uint32_t resize_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q) {
    if (!resize_axis_ok(filter, in_len, out_len)) return 0;
    std::vector<uint32_t> lo_all;
    std::vector<int32_t> q_all;
    uint32_t span = 0;
    const uint32_t k = weights_pass(filter, in_len, out_len, lo_all, q_all, span);
    for (uint32_t i = 0; i < out_len; ++i) {
        if (lo) lo[i] = lo_all[i];
        if (q)
            for (uint32_t j = 0; j < k; ++j) q[size_t(i) * k + j] = q_all[size_t(i) * span + j];
    }
    return k;
}

// One axis for the kernels: lo moved left over zero weights until lo + k <= in_len, weights tap-major.  An axis already in `w` (the
// same filter and in_len -> out_len earlier in the call: `seen` holds {filter, in_len, out_len, k, at} of each) is shared, not computed
// again.
static uint32_t axis_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, std::vector<int32_t>& w, uint32_t& at, std::vector<uint32_t>& seen) {
    if (!resize_axis_ok(filter, in_len, out_len)) return 0;
    for (size_t i = 0; i + 5 <= seen.size(); i += 5)
        if (seen[i] == filter && seen[i + 1] == in_len && seen[i + 2] == out_len) {
            at = seen[i + 4];
            return seen[i + 3];
        }
    thread_local std::vector<uint32_t> lo;  // (scratch, reused from call to call)
    thread_local std::vector<int32_t> q;
    uint32_t span = 0;
    const uint32_t k = weights_pass(filter, in_len, out_len, lo, q, span);
    at = uint32_t(w.size());
    w.resize(w.size() + size_t(out_len) * (k + 1), 0);
    int32_t* l = w.data() + at;
    int32_t* t = l + out_len;
    for (uint32_t i = 0; i < out_len; ++i) {
        const uint32_t a = std::min(lo[i], in_len - k), s = lo[i] - a;  // (k <= in_len: every run lies inside [0, in_len))
        l[i] = int32_t(a);
        for (uint32_t j = 0; j + s < k; ++j) t[size_t(j + s) * out_len + i] = q[size_t(i) * span + j];
    }
    seen.insert(seen.end(), {filter, in_len, out_len, k, at});
    return k;
}

bool resize_frame_weights(uint32_t filter, uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, ResizeFrame& e, std::vector<int32_t>& w,
                          std::vector<uint32_t>& seen) {
    e.rw = rw;
    e.rh = rh;
    e.kx = axis_weights(filter, rw, ow, w, e.hx, seen);
    e.ky = axis_weights(filter, rh, oh, w, e.vy, seen);
    return e.kx && e.ky;
}

// ---- rectangles that leave the image ------------------------------------------------------------------------------------------------

// The index map of a padded index t (outside [0, n)) for the modes that have one; numpy's np.pad modes of the same names.
static int64_t pad_index(uint32_t mode, int64_t n, int64_t t) {
    switch (mode) {
        case LLCOMP_MI_PAD_EDGE: return t < 0 ? 0 : n - 1;
        case LLCOMP_MI_PAD_REFLECT: return t < 0 ? -t : 2 * (n - 1) - t;
        default: return t < 0 ? -t - 1 : 2 * n - 1 - t;  // SYMMETRIC
    }
}

bool pad_axis(uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t& s0, uint32_t& s_len) {
    if (mode > LLCOMP_MI_PAD_SYMMETRIC || !n || !r) return false;
    const int64_t N = n, X = x, end = X + int64_t(r);
    if (X >= N || end <= 0) return false;  // no image pixel
    const int64_t p = std::max<int64_t>(-X, 0), e = std::max<int64_t>(end - N, 0);
    if (std::max(p, e) > (mode == LLCOMP_MI_PAD_REFLECT ? N - 1 : N)) return false;
    int64_t a = std::max<int64_t>(X, 0), b = std::min(end, N);  // the part inside; the padded indices map next to it or into it
    if (mode == LLCOMP_MI_PAD_REFLECT) {
        if (p) b = std::max(b, p + 1);      // t = -1 .. -p -> 1 .. p
        if (e) a = std::min(a, N - 1 - e);  // t = n .. n + e - 1 -> n - 2 .. n - 1 - e
    } else if (mode == LLCOMP_MI_PAD_SYMMETRIC) {
        if (p) b = std::max(b, p);      // -> 0 .. p - 1
        if (e) a = std::min(a, N - e);  // -> n - 1 .. n - e
    }
    s0 = uint32_t(a);
    s_len = uint32_t(b - a);
    return true;
}

bool padded_axis(uint32_t filter, uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t out_len, PaddedAxis& ax) {
    ax = PaddedAxis{};
    if (!pad_axis(mode, n, x, r, ax.s0, ax.s_len) || !resize_axis_ok(filter, r, out_len)) return false;
    thread_local std::vector<uint32_t> lo;  // (scratch, reused from call to call)
    thread_local std::vector<int32_t> q, run;
    thread_local std::vector<uint32_t> first, len;
    uint32_t span = 0;
    weights_pass(filter, r, out_len, lo, q, span);
    const int64_t N = n, X = x;
    const bool inside = X >= 0 && X + int64_t(r) <= N;  // (then nothing folds, and no leading zero is trimmed: the unpadded tables)
    // every output's folded run, in place over its taps: m is 1-Lipschitz, so the sources of `span` consecutive taps span at most `span`
    run.assign(size_t(out_len) * span, 0);
    first.assign(out_len, 0);
    len.assign(out_len, 0);
    ax.bias.assign(out_len, 0);
    for (uint32_t i = 0; i < out_len; ++i) {
        const int32_t* qi = q.data() + size_t(i) * span;
        int64_t smin = INT64_MAX, smax = -1;
        int64_t src[2 * kResizeMaxDown + 4];
        for (uint32_t j = 0; j < span; ++j) {
            src[j] = -1;
            if (!qi[j]) continue;
            const int64_t t = X + int64_t(lo[i]) + j;
            if (t >= 0 && t < N)
                src[j] = t;
            else if (mode == LLCOMP_MI_PAD_CONSTANT)
                ax.bias[i] += qi[j];
            else
                src[j] = pad_index(mode, N, t);
            if (src[j] >= 0) {
                smin = std::min(smin, src[j]);
                smax = std::max(smax, src[j]);
            }
        }
        if (ax.bias[i]) ax.any_bias = true;
        if (smax < 0) continue;  // (every tap outside, or no weight at all: a run of no taps at 0)
        if (inside) smin = X + int64_t(lo[i]);
        int32_t* ri = run.data() + size_t(i) * span;
        for (uint32_t j = 0; j < span; ++j)
            if (src[j] >= 0) ri[src[j] - smin] += qi[j];
        uint32_t a = 0, b = uint32_t(smax - smin + 1);
        while (b > 0 && !ri[b - 1]) --b;
        if (!inside)
            while (a < b && !ri[a]) ++a;
        first[i] = uint32_t(smin - int64_t(ax.s0)) + a;
        len[i] = b - a;
        if (a) std::memmove(ri, ri + a, size_t(b - a) * sizeof(int32_t));
        if (b == a) first[i] = 0;
    }
    ax.k = 1;
    for (uint32_t i = 0; i < out_len; ++i) ax.k = std::max(ax.k, len[i]);
    ax.lo.assign(out_len, 0);
    ax.q.assign(size_t(out_len) * ax.k, 0);
    for (uint32_t i = 0; i < out_len; ++i) {
        const uint32_t a = std::min(first[i], ax.s_len - ax.k), s = first[i] - a;  // (k <= s_len: every run lies inside the interval)
        ax.lo[i] = int32_t(a);
        for (uint32_t j = 0; j < len[i]; ++j) ax.q[size_t(i) * ax.k + s + j] = run[size_t(i) * span + j];
    }
    return true;
}

// One padded axis for the kernels (axis_weights for it): lo[out], then the folded weights tap-major.
static const PaddedSeen::Axis* padded_axis_weights(uint32_t filter, uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t out_len,
                                                   std::vector<int32_t>& w, PaddedSeen& seen) {
    for (const PaddedSeen::Axis& a : seen.axes)
        if (a.filter == filter && a.mode == mode && a.n == n && a.x == x && a.r == r && a.out == out_len) return &a;
    PaddedSeen::Axis rec{filter, mode, n, r, out_len, x, 0, 0, 0, 0, 0, false};
    if (x >= 0 && uint64_t(x) + r <= n) {  // inside the image: the unpadded axis, shared with every other rectangle of this size
        rec.k = axis_weights(filter, r, out_len, w, rec.at, seen.plain);
        if (!rec.k) return nullptr;
        rec.s0 = uint32_t(x);
        rec.s_len = r;
        rec.bias_at = uint32_t(seen.bias.size());
        seen.bias.resize(seen.bias.size() + out_len, 0);
    } else {
        thread_local PaddedAxis ax;
        if (!padded_axis(filter, mode, n, x, r, out_len, ax)) return nullptr;
        rec.k = ax.k;
        rec.s0 = ax.s0;
        rec.s_len = ax.s_len;
        rec.any_bias = ax.any_bias;
        rec.at = uint32_t(w.size());
        w.resize(w.size() + size_t(out_len) * (ax.k + 1), 0);
        int32_t* l = w.data() + rec.at;
        int32_t* t = l + out_len;
        for (uint32_t i = 0; i < out_len; ++i) {
            l[i] = ax.lo[i];
            for (uint32_t j = 0; j < ax.k; ++j) t[size_t(j) * out_len + i] = ax.q[size_t(i) * ax.k + j];
        }
        rec.bias_at = uint32_t(seen.bias.size());
        seen.bias.insert(seen.bias.end(), ax.bias.begin(), ax.bias.end());
    }
    seen.axes.push_back(rec);
    return &seen.axes.back();
}

bool padded_frame_weights(uint32_t filter, uint32_t mode, uint32_t w, uint32_t h, const int32_t* rect, uint32_t ow, uint32_t oh, bool with_bias,
                          ResizeFrame& e, uint32_t src[4], bool* biased, std::vector<int32_t>& wts, PaddedSeen& seen) {
    if (rect[2] <= 0 || rect[3] <= 0) return false;
    const PaddedSeen::Axis* ax = padded_axis_weights(filter, mode, w, rect[0], uint32_t(rect[2]), ow, wts, seen);
    if (!ax) return false;
    const PaddedSeen::Axis hx = *ax;  // (a copy: the next call may move the records)
    ax = padded_axis_weights(filter, mode, h, rect[1], uint32_t(rect[3]), oh, wts, seen);
    if (!ax) return false;
    const PaddedSeen::Axis vy = *ax;
    src[0] = hx.s0;
    src[1] = vy.s0;
    e.rw = src[2] = hx.s_len;
    e.rh = src[3] = vy.s_len;
    e.kx = hx.k;
    e.ky = vy.k;
    e.hx = hx.at;
    e.vy = vy.at;
    if (biased) *biased = hx.any_bias || vy.any_bias;
    if (!with_bias) return true;
    for (const PaddedSeen::Pair& p : seen.pairs)
        if (p.hx == hx.at && p.vy == vy.at) {
            e.pad[0] = p.at;
            return true;
        }
    e.pad[0] = uint32_t(wts.size());
    wts.insert(wts.end(), seen.bias.begin() + hx.bias_at, seen.bias.begin() + hx.bias_at + ow);
    wts.insert(wts.end(), seen.bias.begin() + vy.bias_at, seen.bias.begin() + vy.bias_at + oh);
    seen.pairs.push_back(PaddedSeen::Pair{hx.at, vy.at, e.pad[0]});
    return true;
}

int check_output_format(const llcomp_mi_output_format* fmt, uint32_t c, OutFormat& o) {
    o = OutFormat{};
    if (!fmt) return LLCOMP_MI_OK;
    if (fmt->struct_size < sizeof(llcomp_mi_output_format) || fmt->dtype > LLCOMP_MI_DTYPE_BF16 || fmt->layout > LLCOMP_MI_LAYOUT_CHW ||
        fmt->scale > 1 || !c || c > 255)
        return LLCOMP_MI_BAD_ARGS;
    if (fmt->dtype == LLCOMP_MI_DTYPE_U8 && (fmt->scale || fmt->mean || fmt->std)) return LLCOMP_MI_BAD_ARGS;
    for (uint32_t ch = 0; ch < c; ++ch) {
        if (fmt->mean && !std::isfinite(fmt->mean[ch])) return LLCOMP_MI_BAD_ARGS;
        if (fmt->std && (!std::isfinite(fmt->std[ch]) || fmt->std[ch] == 0.0f)) return LLCOMP_MI_BAD_ARGS;
    }
    static constexpr uint32_t kSize[4] = {1, 4, 2, 2};
    o.dtype = fmt->dtype;
    o.layout = fmt->layout;
    o.esize = kSize[fmt->dtype];
    o.plain = fmt->dtype == LLCOMP_MI_DTYPE_U8 && fmt->layout == LLCOMP_MI_LAYOUT_HWC;
    return LLCOMP_MI_OK;
}

// binary32 -> binary16, round to nearest even, overflow to +-inf (F. Giesen's float_to_half_fast3_rtne, public domain): the subnormal
// range through a float addition that rounds at the right bit, the normal range through integer rounding of the mantissa.
static uint16_t f32_to_f16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = u & 0x80000000u;
    u ^= sign;
    uint32_t o;
    if (u >= (127u + 16) << 23) {  // at or past 2^16: inf (or NaN)
        o = u > 0x7F800000u ? 0x7E00u : 0x7C00u;
    } else if (u < 113u << 23) {  // below 2^-14: a subnormal half or zero
        const uint32_t magic_u = ((127u - 15) + (23 - 10) + 1) << 23;
        float magic, g;
        std::memcpy(&magic, &magic_u, 4);
        std::memcpy(&g, &u, 4);
        g += magic;
        std::memcpy(&o, &g, 4);
        o -= magic_u;
    } else {
        const uint32_t odd = (u >> 13) & 1u;
        u += (uint32_t(15 - 127) << 23) + 0xFFFu + odd;
        o = u >> 13;
    }
    return uint16_t(o | (sign >> 16));
}

void output_table(const llcomp_mi_output_format* fmt, uint32_t c, const OutFormat& o, uint8_t* table) {
    for (uint32_t ch = 0; ch < c; ++ch)
        for (uint32_t v = 0; v < 256; ++v) {
            // (the rule: binary32, no fused operations -- none can fuse here, there is no multiply -- in this order)
            float t = float(v);
            if (fmt && fmt->scale) t = t / 255.0f;
            if (fmt && fmt->mean) t = t - fmt->mean[ch];
            if (fmt && fmt->std) t = t / fmt->std[ch];
            uint32_t u;
            std::memcpy(&u, &t, 4);
            const size_t at = size_t(ch) * 256 + v;
            switch (o.dtype) {
                case LLCOMP_MI_DTYPE_F32: std::memcpy(table + 4 * at, &u, 4); break;
                case LLCOMP_MI_DTYPE_F16: {
                    const uint16_t h = f32_to_f16(t);
                    std::memcpy(table + 2 * at, &h, 2);
                    break;
                }
                case LLCOMP_MI_DTYPE_BF16: {
                    const uint16_t b = uint16_t((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);  // (no NaN reaches here: every input is finite)
                    std::memcpy(table + 2 * at, &b, 2);
                    break;
                }
                default: table[at] = uint8_t(v); break;
            }
        }
}

}  // namespace llcomp_mi
