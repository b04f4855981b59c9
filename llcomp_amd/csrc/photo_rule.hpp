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

// the ops that need the view's statistics first (CONTRAST the sum of L, the other two a histogram per channel) ...
LLMI_HD inline bool photo_needs_stats(uint32_t op) {
    return op == LLCOMP_MI_PHOTO_CONTRAST || op == LLCOMP_MI_PHOTO_AUTOCONTRAST || op == LLCOMP_MI_PHOTO_EQUALIZE;
}
// ... and the ops that are one table per channel (every op but the two that mix channels)
LLMI_HD inline bool photo_is_table(uint32_t op) {
    return op < LLCOMP_MI_PHOTO_OP_COUNT && op != LLCOMP_MI_PHOTO_COLOR && op != LLCOMP_MI_PHOTO_GRAYSCALE;
}

// the limits of one op: finite factors within 0..256, an integer threshold within 0..256, integer bits within 1..8
LLMI_HD inline bool photo_op_ok(uint32_t op, float param) {
    switch (op) {
        case LLCOMP_MI_PHOTO_BRIGHTNESS:
        case LLCOMP_MI_PHOTO_CONTRAST:
        case LLCOMP_MI_PHOTO_COLOR: return param >= 0.0f && param <= 256.0f;  // (false for a NaN)
        case LLCOMP_MI_PHOTO_SOLARIZE: return param >= 0.0f && param <= 256.0f && float(int32_t(param)) == param;
        case LLCOMP_MI_PHOTO_POSTERIZE: return param >= 1.0f && param <= 8.0f && float(int32_t(param)) == param;
        case LLCOMP_MI_PHOTO_GRAYSCALE:
        case LLCOMP_MI_PHOTO_INVERT:
        case LLCOMP_MI_PHOTO_AUTOCONTRAST:
        case LLCOMP_MI_PHOTO_EQUALIZE: return true;
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

// The two ops that mix channels, on one RGB pixel in place
LLMI_HD inline void photo_color(uint32_t& r, uint32_t& g, uint32_t& b, float a) {
    const uint32_t l = photo_luma(r, g, b);
    r = photo_blend(l, r, a);
    g = photo_blend(l, g, a);
    b = photo_blend(l, b, a);
}
LLMI_HD inline void photo_grayscale(uint32_t& r, uint32_t& g, uint32_t& b) { r = g = b = photo_luma(r, g, b); }

}  // namespace llcomp_mi
