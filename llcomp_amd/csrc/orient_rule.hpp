// orient_rule.hpp -- the rule of the batch orientation (include/llcomp_mi.h: "Batch orientation"), stated ONCE: these functions are
// compiled into the kernel (orient_kernels.hip) and into llcomp_mi_orient_reference and the checks (orient_plan.cpp).  A code is 0 or
// PIL's Image.Transpose value plus 1; out(x, y) = in(orient_src(code, ow, oh, x, y)); elements move, nothing is computed on them.
// The element's size and the shape of a batch: batch_ops.hpp.
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "batch_ops.hpp"

namespace llcomp_mi {

constexpr uint32_t kOrientCodes = 8;

struct OrientXY {
    uint32_t x, y;
};
struct OrientRect {  // x0 <= x < x1, y0 <= y < y1
    uint32_t x0, y0, x1, y1;
};

// The codes that exchange the axes: they keep the shape of a square sample only
LLMI_HD inline bool orient_transposes(uint32_t code) {
    return code == LLCOMP_MI_ORIENT_ROTATE_90 || code == LLCOMP_MI_ORIENT_ROTATE_270 || code == LLCOMP_MI_ORIENT_TRANSPOSE ||
           code == LLCOMP_MI_ORIENT_TRANSVERSE;
}

// THE RULE: the pixel of the input that the output's pixel (x, y) takes, in a sample of ow x oh pixels (ow == oh where the code transposes)
LLMI_HD inline OrientXY orient_src(uint32_t code, uint32_t ow, uint32_t oh, uint32_t x, uint32_t y) {
    switch (code) {
        case LLCOMP_MI_ORIENT_FLIP_LEFT_RIGHT: return {ow - 1 - x, y};
        case LLCOMP_MI_ORIENT_FLIP_TOP_BOTTOM: return {x, oh - 1 - y};
        case LLCOMP_MI_ORIENT_ROTATE_90: return {ow - 1 - y, x};
        case LLCOMP_MI_ORIENT_ROTATE_180: return {ow - 1 - x, oh - 1 - y};
        case LLCOMP_MI_ORIENT_ROTATE_270: return {y, oh - 1 - x};
        case LLCOMP_MI_ORIENT_TRANSPOSE: return {y, x};
        case LLCOMP_MI_ORIENT_TRANSVERSE: return {ow - 1 - y, oh - 1 - x};
        default: return {x, y};
    }
}

// The length of the longest orbit of a pixel under the code's map: the quarter turns have 4, the other six are involutions
LLMI_HD inline uint32_t orient_order(uint32_t code) {
    return code == LLCOMP_MI_ORIENT_NONE ? 1u : (code == LLCOMP_MI_ORIENT_ROTATE_90 || code == LLCOMP_MI_ORIENT_ROTATE_270) ? 4u : 2u;
}
// The code whose map is the code's map applied k times, k below orient_order(code): the quarter turns pass through the half turn
LLMI_HD inline uint32_t orient_power(uint32_t code, uint32_t k) {
    if (k == 0) return LLCOMP_MI_ORIENT_NONE;
    if (k == 1 || orient_order(code) == 2) return code;
    if (k == 2) return LLCOMP_MI_ORIENT_ROTATE_180;
    return code == LLCOMP_MI_ORIENT_ROTATE_90 ? LLCOMP_MI_ORIENT_ROTATE_270 : LLCOMP_MI_ORIENT_ROTATE_90;
}

// The fundamental domain of a code: one pixel of every orbit that has more than one, none of an orbit of one (a pixel that is its own
// image: the middle column of a mirror of odd width, the diagonal of a transposition, the centre of an odd square).  The domain's
// pixels and their images under the powers of the map are all the pixels that move, each once.  It lies in the rectangle
// [0, dw) x [0, dh) of orient_domain_box and is the part of it where orient_in_domain holds.
//   mirror: the left half; vertical flip: the top half; half turn: the top half and, for an odd height, the left half of the middle row;
//   quarter turns: the quarter [0, ceil(n / 2)) x [0, floor(n / 2)); transposition: above the diagonal; transverse: above the antidiagonal
LLMI_HD inline OrientXY orient_domain_box(uint32_t code, uint32_t ow, uint32_t oh) {
    switch (code) {
        case LLCOMP_MI_ORIENT_FLIP_LEFT_RIGHT: return {ow / 2, oh};
        case LLCOMP_MI_ORIENT_FLIP_TOP_BOTTOM: return {ow, oh / 2};
        case LLCOMP_MI_ORIENT_ROTATE_180: return {ow, oh - oh / 2};
        case LLCOMP_MI_ORIENT_ROTATE_90:
        case LLCOMP_MI_ORIENT_ROTATE_270: return {ow - ow / 2, oh / 2};
        case LLCOMP_MI_ORIENT_TRANSPOSE:
        case LLCOMP_MI_ORIENT_TRANSVERSE: return {ow, oh};
        default: return {0, 0};
    }
}
LLMI_HD inline bool orient_in_domain(uint32_t code, uint32_t ow, uint32_t oh, uint32_t x, uint32_t y) {
    switch (code) {
        case LLCOMP_MI_ORIENT_ROTATE_180: return y < oh / 2 || x < ow / 2;  // (inside the box: y == oh / 2 is the middle row of an odd height)
        case LLCOMP_MI_ORIENT_TRANSPOSE: return y < x;
        case LLCOMP_MI_ORIENT_TRANSVERSE: return uint64_t(x) + y + 1 < ow;
        default: return true;
    }
}
// What a rectangle inside the box holds of the domain: 0 nothing, 1 some of its pixels, 2 all of them.  The domains are convex inside
// their boxes but for the half turn's, whose notch is at the box's last row: the four corners decide.
LLMI_HD inline uint32_t orient_rect_in_domain(uint32_t code, uint32_t ow, uint32_t oh, const OrientRect& r) {
    const uint32_t in = uint32_t(orient_in_domain(code, ow, oh, r.x0, r.y0)) + uint32_t(orient_in_domain(code, ow, oh, r.x1 - 1, r.y0)) +
                        uint32_t(orient_in_domain(code, ow, oh, r.x0, r.y1 - 1)) + uint32_t(orient_in_domain(code, ow, oh, r.x1 - 1, r.y1 - 1));
    return in == 4 ? 2u : in ? 1u : 0u;
}
// The image of a rectangle under out -> in of a code: again a rectangle, from two opposite corners
LLMI_HD inline OrientRect orient_rect_src(uint32_t code, uint32_t ow, uint32_t oh, const OrientRect& r) {
    const OrientXY a = orient_src(code, ow, oh, r.x0, r.y0), b = orient_src(code, ow, oh, r.x1 - 1, r.y1 - 1);
    return {a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, (a.x < b.x ? b.x : a.x) + 1, (a.y < b.y ? b.y : a.y) + 1};
}

}  // namespace llcomp_mi
