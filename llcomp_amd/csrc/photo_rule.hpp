// photo_rule.hpp -- the rule of the photometric chains (include/llcomp_mi.h: "Photometric chains"), stated ONCE: these functions are
// compiled into the kernels (photo_kernels.hip) and into llcomp_mi_photo_reference and the planner's checks (photo_plan.cpp).  The rule is
// PIL's ImageEnhance / ImageOps: blend in IEEE binary32, the mean and autocontrast in binary64, every operation rounded by itself, so
// nothing here may be contracted into a fused multiply-add: hipcc does that on the device by default, and the pragma below switches it
// off for every file that includes this header (new files only: the existing sources never include it and are built as they were).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "geometry.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
// (g++ builds of the host checks target baseline x86-64, which has no fused multiply-add to contract into)

namespace llcomp_mi {

// PIL's L of an RGB pixel
LLMI_HD inline uint32_t photo_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// PIL's ImagingBlend of one sample: d the degenerate image's, v the view's
LLMI_HD inline uint32_t photo_blend(uint32_t d, uint32_t v, float a) {
    const float diff = float(int32_t(v) - int32_t(d));
    const float s = a * diff;
    const float t = float(int32_t(d)) + s;
    if (a >= 0.0f && a <= 1.0f) return uint32_t(int32_t(t)) & 0xFFu;  // (t lies between d and v)
    return t <= 0.0f ? 0u : (t >= 255.0f ? 255u : uint32_t(int32_t(t)));
}

// Every op is of one kind: it says which kernels take a view in a step (photo_kernels.hip) and which branch the host's reference
// (photo_plan.cpp).  kPixel: computed from the pixel by itself (photo_pixel), and what is no op code at all, for which nothing is
// computed.  kTable: one table per channel, the rest of the pointwise family 0..8.  kBlur: GAUSSIAN_BLUR.  kSharp: ADJUST_SHARPNESS.
enum class PhotoKind : uint32_t { kPixel, kTable, kBlur, kSharp };
LLMI_HD inline PhotoKind photo_kind(uint32_t op) {
    if (op < LLCOMP_MI_PHOTO_OP_COUNT) return op == LLCOMP_MI_PHOTO_COLOR || op == LLCOMP_MI_PHOTO_GRAYSCALE ? PhotoKind::kPixel : PhotoKind::kTable;
    return op == LLCOMP_MI_PHOTO_GAUSSIAN_BLUR ? PhotoKind::kBlur : op == LLCOMP_MI_PHOTO_ADJUST_SHARPNESS ? PhotoKind::kSharp : PhotoKind::kPixel;
}
// the ops of kTable that need the view's statistics first (CONTRAST the sum of L, the other two a histogram per channel)
LLMI_HD inline bool photo_needs_stats(uint32_t op) {
    return op == LLCOMP_MI_PHOTO_CONTRAST || op == LLCOMP_MI_PHOTO_AUTOCONTRAST || op == LLCOMP_MI_PHOTO_EQUALIZE;
}

// the limits of one op: finite factors within 0..256, an integer threshold within 0..256, integer bits within 1..8, a finite radius
// within 0..LLCOMP_MI_PHOTO_MAX_RADIUS, a finite hue factor within -0.5..0.5
LLMI_HD inline bool photo_op_ok(uint32_t op, float param) {
    switch (op) {
        case LLCOMP_MI_PHOTO_BRIGHTNESS:
        case LLCOMP_MI_PHOTO_CONTRAST:
        case LLCOMP_MI_PHOTO_ADJUST_SHARPNESS:
        case LLCOMP_MI_PHOTO_COLOR: return param >= 0.0f && param <= 256.0f;  // (false for a NaN)
        case LLCOMP_MI_PHOTO_SOLARIZE: return param >= 0.0f && param <= 256.0f && float(int32_t(param)) == param;
        case LLCOMP_MI_PHOTO_POSTERIZE: return param >= 1.0f && param <= 8.0f && float(int32_t(param)) == param;
        case LLCOMP_MI_PHOTO_GRAYSCALE:
        case LLCOMP_MI_PHOTO_INVERT:
        case LLCOMP_MI_PHOTO_AUTOCONTRAST:
        case LLCOMP_MI_PHOTO_EQUALIZE: return true;
        case LLCOMP_MI_PHOTO_GAUSSIAN_BLUR: return param >= 0.0f && param <= float(LLCOMP_MI_PHOTO_MAX_RADIUS);
        case LLCOMP_MI_PHOTO_ADJUST_HUE: return param >= -0.5f && param <= 0.5f;
        default: return false;
    }
}

// CONTRAST's degenerate value: the view's mean L, rounded as PIL rounds it
LLMI_HD inline uint32_t photo_mean(uint64_t sum_l, uint64_t n) {
    const double q = double(sum_l) / double(n);
    return uint32_t(int32_t(q + 0.5));
}

// The table of a table-kind op for one channel: lut[256] from the parameter and the view's statistics -- hist[256] the channel's
// histogram (read by AUTOCONTRAST and EQUALIZE only), sum_l the view's sum of L (CONTRAST only), n its pixels.
template <class Hist>
LLMI_HD inline void photo_table(uint32_t op, float param, const Hist& hist, uint64_t sum_l, uint64_t n, uint8_t* lut) {
    for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(i);
    switch (op) {
        case LLCOMP_MI_PHOTO_BRIGHTNESS:
            for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(photo_blend(0, i, param));
            break;
        case LLCOMP_MI_PHOTO_CONTRAST: {
            const uint32_t m = photo_mean(sum_l, n);
            for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(photo_blend(m, i, param));
            break;
        }
        case LLCOMP_MI_PHOTO_INVERT:
            for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(255u - i);
            break;
        case LLCOMP_MI_PHOTO_SOLARIZE: {
            const uint32_t t = uint32_t(int32_t(param));
            for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(i < t ? i : 255u - i);
            break;
        }
        case LLCOMP_MI_PHOTO_POSTERIZE: {
            const uint32_t mask = ~((1u << (8u - uint32_t(int32_t(param)))) - 1u);
            for (uint32_t i = 0; i < 256; ++i) lut[i] = uint8_t(i & mask);
            break;
        }
        case LLCOMP_MI_PHOTO_AUTOCONTRAST: {
            uint32_t lo = 256, hi = 0;
            for (uint32_t i = 0; i < 256; ++i)
                if (hist[i]) {
                    if (lo == 256) lo = i;
                    hi = i;
                }
            if (lo == 256 || hi <= lo) break;
            const double s = 255.0 / double(hi - lo);
            const double o = -double(lo) * s;
            for (uint32_t i = 0; i < 256; ++i) {
                const double p = double(i) * s;
                const int32_t ix = int32_t(p + o);
                lut[i] = uint8_t(ix < 0 ? 0 : (ix > 255 ? 255 : ix));
            }
            break;
        }
        case LLCOMP_MI_PHOTO_EQUALIZE: {
            uint32_t present = 0, last = 0;
            for (uint32_t i = 0; i < 256; ++i)
                if (hist[i]) {
                    ++present;
                    last = i;
                }
            if (present < 2) break;
            const uint64_t step = (n - hist[last]) / 255;
            if (!step) break;
            uint64_t acc = step / 2;
            for (uint32_t i = 0; i < 256; ++i) {
                const uint64_t q = acc / step;
                lut[i] = uint8_t(q > 255 ? 255 : q);
                acc += hist[i];
            }
            break;
        }
        default: break;
    }
}

// GAUSSIAN_BLUR: the box of ImageFilter.GaussianBlur(radius) with three passes -- r its whole radius, ww the weight of the 2r + 1
// samples inside, fw that of the two samples at r + 1, in units of 2^-24.  Binary32 throughout but the square root.
LLMI_HD inline void photo_blur_weights(float radius, uint32_t& r, uint32_t& ww, uint32_t& fw) {
    const float s2 = radius * radius / 3.0f;
    const float big_l = float(sqrt(double(12.0f * s2 + 1.0f)));
    const float l = floorf((big_l - 1.0f) / 2.0f);
    const float num = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
    const float den = 6.0f * (s2 - (l + 1.0f) * (l + 1.0f));
    const float fr = l + num / den;
    r = uint32_t(int32_t(fr));
    ww = uint32_t(float(1u << 24) / (fr * 2.0f + 1.0f));
    fw = ((1u << 24) - (2u * r + 1u) * ww) / 2u;
}
// ... and one output sample of a line pass: acc the sum of the 2r + 1 samples around it, far that of the two at r + 1 (the line's
// ends replicated), in wrapping 32-bit arithmetic
LLMI_HD inline uint32_t photo_blur_tap(uint32_t acc, uint32_t far, uint32_t ww, uint32_t fw) {
    return (acc * ww + far * fw + (1u << 23)) >> 24;
}
// How far the three passes reach to each side of a sample
LLMI_HD inline uint32_t photo_blur_reach(uint32_t r) { return 3u * (r + 1u); }

// ADJUST_SHARPNESS: PIL's ImageFilter.SMOOTH of one interior sample -- sum9 the sum of the nine samples of its 3 x 3 window, the sample
// itself among them.  PIL adds nine binary32 products of (1 1 1 / 1 5 1 / 1 1 1) / 13 onto 0.5 and truncates; the integer form is the
// same byte in whatever order the nine are summed (include/llcomp_mi.h).  A sample of the outermost rows and columns is its own smooth
// value; the op's result is photo_blend(smooth, sample, factor).
LLMI_HD inline uint32_t photo_smooth(uint32_t sum9, uint32_t centre) { return (sum9 + 4u * centre + 6u) / 13u; }
LLMI_HD inline bool photo_smooth_interior(uint64_t x, uint64_t y, uint64_t w, uint64_t h) { return x >= 1 && x + 1 < w && y >= 1 && y + 1 < h; }

// ADJUST_HUE: the byte added to H ...
LLMI_HD inline uint32_t photo_hue_shift(float factor) { return uint32_t(int32_t(double(factor) * 255.0)) & 0xFFu; }
LLMI_HD inline uint32_t photo_clip8(int32_t v) { return v < 0 ? 0u : (v > 255 ? 255u : uint32_t(v)); }
// ... PIL's convert("HSV") of one pixel ...
LLMI_HD inline void photo_rgb2hsv(uint32_t r, uint32_t g, uint32_t b, uint32_t& hh, uint32_t& ss, uint32_t& vv) {
    const uint32_t mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    vv = mx;
    hh = ss = 0;
    if (mx == mn) return;
    const float cr = float(int32_t(mx - mn));
    const float s = cr / float(int32_t(mx));
    const float rc = float(int32_t(mx - r)) / cr, gc = float(int32_t(mx - g)) / cr, bc = float(int32_t(mx - b)) / cr;
    float h;
    if (r == mx)
        h = float(double(bc) - double(gc));
    else if (g == mx)
        h = float((2.0 + double(rc)) - double(bc));
    else
        h = float((4.0 + double(gc)) - double(rc));
    const double q = double(h) / 6.0 + 1.0;
    h = float(fmod(q, 1.0));
    hh = photo_clip8(int32_t(double(h) * 255.0));
    ss = photo_clip8(int32_t(double(s) * 255.0));
}
// ... and its convert("RGB") of an HSV pixel
LLMI_HD inline void photo_hsv2rgb(uint32_t hh, uint32_t ss, uint32_t vv, uint32_t& r, uint32_t& g, uint32_t& b) {
    r = g = b = vv;
    if (!ss) return;
    const double h = double(float(int32_t(hh))) * 6.0 / 255.0;
    const double fl = floor(h);
    const int32_t i = int32_t(fl);
    const float f = float(h - double(float(i)));
    const float fs = float(double(float(int32_t(ss))) / 255.0);
    const double v = double(int32_t(vv));
    const double ps = 1.0 - double(fs);
    const double qm = double(fs) * double(f);
    const double tm = double(fs) * (1.0 - double(f));
    const uint32_t p = photo_clip8(int32_t(round(v * ps)));
    const uint32_t q = photo_clip8(int32_t(round(v * (1.0 - qm))));
    const uint32_t t = photo_clip8(int32_t(round(v * (1.0 - tm))));
    switch (i % 6) {
        case 0: r = vv, g = t, b = p; break;
        case 1: r = q, g = vv, b = p; break;
        case 2: r = p, g = vv, b = t; break;
        case 3: r = p, g = q, b = vv; break;
        case 4: r = t, g = p, b = vv; break;
        default: r = vv, g = p, b = q; break;
    }
}
// ... on one RGB pixel in place
LLMI_HD inline void photo_hue(uint32_t& r, uint32_t& g, uint32_t& b, uint32_t shift) {
    uint32_t hh, ss, vv;
    photo_rgb2hsv(r, g, b, hh, ss, vv);
    photo_hsv2rgb((hh + shift) & 0xFFu, ss, vv, r, g, b);
}

// The ops of kPixel on one RGB pixel in place: COLOR blends with the pixel's own L, GRAYSCALE is it, ADJUST_HUE adds `shift` to H --
// photo_hue_shift(param), the caller's, so that it stays out of the loop over the pixels.  Any other op leaves the pixel as it is.
LLMI_HD inline void photo_pixel(uint32_t op, float param, uint32_t shift, uint32_t& r, uint32_t& g, uint32_t& b) {
    if (op == LLCOMP_MI_PHOTO_COLOR) {
        const uint32_t l = photo_luma(r, g, b);
        r = photo_blend(l, r, param), g = photo_blend(l, g, param), b = photo_blend(l, b, param);
    } else if (op == LLCOMP_MI_PHOTO_GRAYSCALE) {
        r = g = b = photo_luma(r, g, b);
    } else if (op == LLCOMP_MI_PHOTO_ADJUST_HUE) {
        photo_hue(r, g, b, shift);
    }
}

}  // namespace llcomp_mi
