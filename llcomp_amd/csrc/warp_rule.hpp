// warp_rule.hpp -- the per-pixel rule of the warped views (include/llcomp_mi.h: "Views under an affine map"), stated ONCE: these functions
// are compiled into the gather kernel (warp_kernels.hip) and into llcomp_mi_warp_reference and the planner (warp_plan.cpp).  The rule is
// PIL's Image.transform(AFFINE) in IEEE binary64 with every operation rounded by itself, so nothing here may be contracted into a fused
// multiply-add: hipcc does that on the device by default, and the pragma below switches it off for every file that includes this header
// (new files only: the existing sources never include it and are built as they were).  The perspective views' coordinate rule
// (PIL's PERSPECTIVE: two true divisions per pixel) is at the end; from the coordinate on it shares everything above.
#pragma once
#include <cmath>
#include <cstdint>

#include "geometry.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
// (g++ builds of the host checks target baseline x86-64, which has no fused multiply-add to contract into)

namespace llcomp_mi {

enum : uint32_t { kWarpSmooth = 0, kWarpFixed = 1, kWarpTable = 2, kWarpEmpty = 3 };  // how a view's source coordinates are found

LLMI_HD inline int32_t warp_cl(int32_t t, int32_t n) { return t < 0 ? 0 : (t > n - 1 ? n - 1 : t); }

// BILINEAR and BICUBIC: the source coordinate of output pixel (x, y)
LLMI_HD inline void warp_xy(const double* m, uint32_t x, uint32_t y, double& xin, double& yin) {
    const double xs = double(x) + 0.5, ys = double(y) + 0.5;
    const double a = m[0] * xs, b = m[1] * ys, d = m[3] * xs, e = m[4] * ys;
    const double ab = a + b, de = d + e;
    xin = ab + m[2];
    yin = de + m[5];
}
LLMI_HD inline bool warp_inside(double xin, double yin, uint32_t w, uint32_t h) {
    return xin >= 0.0 && xin < double(w) && yin >= 0.0 && yin < double(h);
}
// ... and, for a pixel inside, the tap origin (X, Y) and the fractions
struct WarpTap {
    int32_t X, Y;
    double dx, dy;
};
LLMI_HD inline WarpTap warp_tap(double xin, double yin) {
    const double xh = xin - 0.5, yh = yin - 0.5;
    const double fx = floor(xh), fy = floor(yh);
    return WarpTap{int32_t(fx), int32_t(fy), xh - fx, yh - fy};
}

// One channel of one pixel.  P(row, col) is the frame's u8 sample of that channel as a double, rows and columns in frame coordinates.
template <class Px>
LLMI_HD inline uint32_t warp_bilinear(const Px& P, const WarpTap& t, int32_t w, int32_t h) {
    const int32_t c0 = warp_cl(t.X, w), c1 = warp_cl(t.X + 1, w), r0 = warp_cl(t.Y, h);
    const double a0 = P(r0, c0), a1 = P(r0, c1);
    const double s0 = (a1 - a0) * t.dx;
    const double v1 = a0 + s0;
    double v2 = v1;
    if (t.Y + 1 >= 0 && t.Y + 1 < h) {
        const double b0 = P(t.Y + 1, c0), b1 = P(t.Y + 1, c1);
        const double s1 = (b1 - b0) * t.dx;
        v2 = b0 + s1;
    }
    const double s = (v2 - v1) * t.dy;
    const double v = v1 + s;
    return uint32_t(int32_t(v));
}
LLMI_HD inline double warp_cub(double p0, double p1, double p2, double p3, double d) {
    const double q2 = -p0 + p2;
    const double q3 = ((2.0 * (p0 - p1)) + p2) - p3;
    const double q4 = (((-p0) + p1) - p2) + p3;
    const double i3 = d * q4;
    const double i2 = d * (q3 + i3);
    const double i1 = d * (q2 + i2);
    return p1 + i1;
}
template <class Px>
LLMI_HD inline uint32_t warp_bicubic(const Px& P, const WarpTap& t, int32_t w, int32_t h) {
    const int32_t c0 = warp_cl(t.X - 1, w), c1 = warp_cl(t.X, w), c2 = warp_cl(t.X + 1, w), c3 = warp_cl(t.X + 2, w);
    const int32_t r0 = warp_cl(t.Y - 1, h);
    double r[4];
    r[0] = warp_cub(P(r0, c0), P(r0, c1), P(r0, c2), P(r0, c3), t.dx);
    for (int32_t k = 1; k < 4; ++k) {
        const int32_t row = t.Y - 1 + k;
        r[k] = row >= 0 && row < h ? warp_cub(P(row, c0), P(row, c1), P(row, c2), P(row, c3), t.dx) : r[k - 1];
    }
    const double v = warp_cub(r[0], r[1], r[2], r[3], t.dy);
    return v <= 0.0 ? 0u : (v >= 255.0 ? 255u : uint32_t(int32_t(v)));
}

// NEAREST, any matrix but a pure scale: PIL's 16.16 form.  FIX(t) = floor(t * 65536 + 0.5) as int32 (wrapping where it does not fit).
LLMI_HD inline int32_t warp_fix(double t) {
    const double p = t * 65536.0;
    const double f = floor(p + 0.5);
    return int32_t(uint32_t(uint64_t(int64_t(f))));
}
LLMI_HD inline void warp_fixed_matrix(const double* m, int32_t* A) {
    const double h0 = m[0] * 0.5, h1 = m[1] * 0.5, h3 = m[3] * 0.5, h4 = m[4] * 0.5;
    const double t2 = (m[2] + h0) + h1, t5 = (m[5] + h3) + h4;
    A[0] = warp_fix(m[0]);
    A[1] = warp_fix(m[1]);
    A[2] = warp_fix(t2);
    A[3] = warp_fix(m[3]);
    A[4] = warp_fix(m[4]);
    A[5] = warp_fix(t5);
}
LLMI_HD inline void warp_fixed_xy(const int32_t* A, uint32_t x, uint32_t y, int32_t& xi, int32_t& yi) {
    const uint32_t ux = uint32_t(A[2]) + x * uint32_t(A[0]) + y * uint32_t(A[1]);
    const uint32_t uy = uint32_t(A[5]) + x * uint32_t(A[3]) + y * uint32_t(A[4]);
    xi = int32_t(ux) >> 16;
    yi = int32_t(uy) >> 16;
}
// NEAREST, a pure scale (m1 == 0 and m3 == 0): the source index of every output index of one axis, accumulated as PIL does; -1 = outside
inline void warp_scale_table(double m_scale, double m_off, uint32_t n_out, uint32_t n_in, int32_t* tab) {
    const double half = m_scale * 0.5;
    double o = m_off + half;
    for (uint32_t k = 0; k < n_out; ++k) {
        // (the limits keep |o| far below 2^31; the comparison also sends what does not fit to "outside")
        tab[k] = o < 0.0 || o >= double(n_in) ? -1 : int32_t(o);
        o = o + m_scale;
    }
}
LLMI_HD inline bool warp_is_scale(const double* m) { return m[1] == 0.0 && m[3] == 0.0; }

// Perspective views (include/llcomp_mi.h: "Views under a projective map"): PIL's Image.transform(PERSPECTIVE).  The denominator and
// the source coordinate of output pixel (x, y) under a[0..7]; the two quotients are true binary64 divisions (whose expansion on the GPU
// uses fused multiply-adds of its own and is correctly rounded), the sums and products above them are rounded one by one.
LLMI_HD inline double persp_den(const double* a, uint32_t x, uint32_t y) {
    const double xs = double(x) + 0.5, ys = double(y) + 0.5;
    const double g = a[6] * xs, k = a[7] * ys;
    const double gk = g + k;
    return gk + 1.0;
}
LLMI_HD inline void persp_xy(const double* a, uint32_t x, uint32_t y, double& xin, double& yin) {
    const double xs = double(x) + 0.5, ys = double(y) + 0.5;
    const double p = a[0] * xs, q = a[1] * ys, d = a[3] * xs, e = a[4] * ys, g = a[6] * xs, k = a[7] * ys;
    const double pq = p + q, de = d + e, gk = g + k;
    const double nx = pq + a[2], ny = de + a[5], den = gk + 1.0;
    xin = nx / den;
    yin = ny / den;
}
// NEAREST: PIL's COORD(v) = v < 0 ? -1 : (int) v of one coordinate, for an axis of n pixels; what lies at or beyond n is outside either
// way and is -1 here too, so nothing that does not fit an int32 is ever converted
LLMI_HD inline int32_t persp_index(double t, uint32_t n) { return t >= 0.0 && t < double(n) ? int32_t(t) : -1; }

}  // namespace llcomp_mi
