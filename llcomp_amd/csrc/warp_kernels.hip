// warp_kernels.hip -- the gather kernel of the warped views (llcomp_mi_codec_decode_warped_views): every view's output pixels, each from
// the few pixels of its frame's box that PIL's Image.transform(AFFINE) reads for it, under NEAREST, BILINEAR or BICUBIC.  Not separable:
// one thread per output pixel, all channels, no intermediate buffer.  The arithmetic is warp_rule.hpp's -- the functions
// llcomp_mi_warp_reference runs on the host -- in binary64 with NO fused multiply-add: the header's pragma holds for this whole file.
// And k_persp, the same gather for the perspective views (llcomp_mi_codec_decode_perspective_views, PIL's PERSPECTIVE): a kernel of its
// own, so that k_warp's instantiations keep their registers (DESIGN.md "Perspective views" has both sets of figures).
#include "warp_rule.hpp"

#include "out_store.hpp"
#include "warp.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace llcomp_mi {

namespace {

// Workgroups of 16 x 16 output pixels (blockIdx.x: the tile, row-major; blockIdx.y: the view), so that the taps of a rotated tile stay
// close together in the box.  C: the channel count where it is 1..4 (the loops over channels unroll), 0 for any other (c_rt).  LUT: the
// group has an output format, whose table [c][256] of E-byte elements is looked up where it lies; CHW: its layout.  Without one the u8
// value goes to [view][y][x][ch].
// A frame pixel (col, row) is read at (col - bx, row - by) of the entry's box, clamped into the box: the plan guarantees that the clamp
// never moves a read, and a read can never leave d_box.
template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_warp(const uint8_t* __restrict__ box, const WarpEntry* __restrict__ ws, const int32_t* __restrict__ tabs,
                                              const uint8_t* __restrict__ fill, const void* __restrict__ table, void* __restrict__ out, uint32_t bw,
                                              uint32_t bh, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, uint32_t c_rt) {
    using T = typename OutElem<E>::T;
    const uint32_t c = C ? uint32_t(C) : c_rt;
    const uint32_t tiles_x = ow / 16 + (ow % 16 != 0), v = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * 16 + threadIdx.x, y = ty * 16 + threadIdx.y;
    if (x >= ow || y >= oh) return;
    const WarpEntry& e = ws[v];
    const uint32_t flags = e.flags, form = (flags >> kWarpFormShift) & 3u, filter = (flags >> 4) & 7u;
    const uint32_t xo = (flags & 1u) ? ow - 1 - x : x;
    const size_t plane = size_t(oh) * ow, px = size_t(y) * ow + xo;
    T* const o = static_cast<T*>(out);
    const T* const lut = static_cast<const T*>(table);
    auto put = [&](uint32_t ch, uint32_t val) { out_store<T, CHW, LUT>(o, lut, v, c, plane, px, ch, val); };
    const uint8_t* const b = box + size_t(e.box) * bh * bw * c;
    const int32_t bx = e.bx, by = e.by;
    auto at = [&](int32_t row, int32_t col) {
        const uint32_t r = uint32_t(warp_cl(row - by, int32_t(bh))), k = uint32_t(warp_cl(col - bx, int32_t(bw)));
        return b + (size_t(r) * bw + k) * c;
    };
    if (form == kWarpSmooth) {
        double xin, yin;
        warp_xy(e.m, x, y, xin, yin);
        if (warp_inside(xin, yin, w, h)) {
            const WarpTap t = warp_tap(xin, yin);
            if (filter == LLCOMP_MI_FILTER_BICUBIC) {
                for (uint32_t ch = 0; ch < c; ++ch) {
                    auto P = [&](int32_t row, int32_t col) { return double(at(row, col)[ch]); };
                    put(ch, warp_bicubic(P, t, int32_t(w), int32_t(h)));
                }
            } else {
                for (uint32_t ch = 0; ch < c; ++ch) {
                    auto P = [&](int32_t row, int32_t col) { return double(at(row, col)[ch]); };
                    put(ch, warp_bilinear(P, t, int32_t(w), int32_t(h)));
                }
            }
            return;
        }
    } else if (form != kWarpEmpty) {
        int32_t xi, yi;
        if (form == kWarpTable) {
            xi = tabs[e.t[0] + x];
            yi = tabs[e.t[1] + y];
        } else {
            warp_fixed_xy(e.a, x, y, xi, yi);
        }
        if (xi >= 0 && xi < int32_t(w) && yi >= 0 && yi < int32_t(h)) {
            const uint8_t* p = at(yi, xi);
            for (uint32_t ch = 0; ch < c; ++ch) put(ch, p[ch]);
            return;
        }
    }
    for (uint32_t ch = 0; ch < c; ++ch) put(ch, fill[ch]);
}

// The perspective gather: the launch shape, the box reads and the stores of k_warp, the coordinates by persp_xy -- two binary64
// divisions per pixel, each expanded by the compiler into a correctly rounded sequence (its own fused multiply-adds are what makes the
// quotient exact; the rule's sums and products above it stay unfused under the pragma).
template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_persp(const uint8_t* __restrict__ box, const PerspEntry* __restrict__ ps, const uint8_t* __restrict__ fill,
                                               const void* __restrict__ table, void* __restrict__ out, uint32_t bw, uint32_t bh, uint32_t w,
                                               uint32_t h, uint32_t ow, uint32_t oh, uint32_t c_rt) {
    using T = typename OutElem<E>::T;
    const uint32_t c = C ? uint32_t(C) : c_rt;
    const uint32_t tiles_x = ow / 16 + (ow % 16 != 0), v = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * 16 + threadIdx.x, y = ty * 16 + threadIdx.y;
    if (x >= ow || y >= oh) return;
    const PerspEntry& e = ps[v];
    const uint32_t flags = e.flags, filter = (flags >> 4) & 7u;
    const uint32_t xo = (flags & 1u) ? ow - 1 - x : x;
    const size_t plane = size_t(oh) * ow, px = size_t(y) * ow + xo;
    T* const o = static_cast<T*>(out);
    const T* const lut = static_cast<const T*>(table);
    auto put = [&](uint32_t ch, uint32_t val) { out_store<T, CHW, LUT>(o, lut, v, c, plane, px, ch, val); };
    const uint8_t* const b = box + size_t(e.box) * bh * bw * c;
    const int32_t bx = e.bx, by = e.by;
    auto at = [&](int32_t row, int32_t col) {
        const uint32_t r = uint32_t(warp_cl(row - by, int32_t(bh))), k = uint32_t(warp_cl(col - bx, int32_t(bw)));
        return b + (size_t(r) * bw + k) * c;
    };
    if (!(flags & kPerspEmpty)) {
        double xin, yin;
        persp_xy(e.a, x, y, xin, yin);
        if (warp_inside(xin, yin, w, h)) {  // (NEAREST: exactly the pixels whose two indices are not -1)
            if (filter == LLCOMP_MI_FILTER_NEAREST) {
                const uint8_t* p = at(persp_index(yin, h), persp_index(xin, w));
                for (uint32_t ch = 0; ch < c; ++ch) put(ch, p[ch]);
                return;
            }
            const WarpTap t = warp_tap(xin, yin);
            if (filter == LLCOMP_MI_FILTER_BICUBIC) {
                for (uint32_t ch = 0; ch < c; ++ch) {
                    auto P = [&](int32_t row, int32_t col) { return double(at(row, col)[ch]); };
                    put(ch, warp_bicubic(P, t, int32_t(w), int32_t(h)));
                }
            } else {
                for (uint32_t ch = 0; ch < c; ++ch) {
                    auto P = [&](int32_t row, int32_t col) { return double(at(row, col)[ch]); };
                    put(ch, warp_bilinear(P, t, int32_t(w), int32_t(h)));
                }
            }
            return;
        }
    }
    for (uint32_t ch = 0; ch < c; ++ch) put(ch, fill[ch]);
}

template <int E, bool CHW, bool LUT>
void launch_persp_c(dim3 grid, hipStream_t s, const uint8_t* d_box, const PerspEntry* d_ps, const uint8_t* d_fill, const void* d_table, void* d_out,
                    uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh) {
    const dim3 blk(16, 16);
    switch (c) {
        case 1: k_persp<1, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ps, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 2: k_persp<2, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ps, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 3: k_persp<3, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ps, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 4: k_persp<4, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ps, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        default: k_persp<0, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ps, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
    }
}

template <int E, bool CHW, bool LUT>
void launch_c(dim3 grid, hipStream_t s, const uint8_t* d_box, const WarpEntry* d_ws, const int32_t* d_tabs, const uint8_t* d_fill, const void* d_table,
              void* d_out, uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh) {
    const dim3 blk(16, 16);
    switch (c) {
        case 1: k_warp<1, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ws, d_tabs, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 2: k_warp<2, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ws, d_tabs, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 3: k_warp<3, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ws, d_tabs, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        case 4: k_warp<4, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ws, d_tabs, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
        default: k_warp<0, E, CHW, LUT><<<grid, blk, 0, s>>>(d_box, d_ws, d_tabs, d_fill, d_table, d_out, bw, bh, w, h, ow, oh, c); break;
    }
}

}  // namespace

hipError_t launch_warp(const uint8_t* d_box, const WarpEntry* d_ws, const int32_t* d_tabs, const uint8_t* d_fill, const void* d_table,
                       const OutFormat& o, void* d_out, uint32_t views, uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow,
                       uint32_t oh, hipStream_t stream) {
    if (!views || views > 65535 || !c || c > 255 || !w || !h || !ow || !oh || !d_ws || !d_fill || !d_out) return hipErrorInvalidValue;
    if (w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || bw > 0x7FFFFFFFu || bh > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (!o.plain && (!d_table || (reinterpret_cast<uintptr_t>(d_table) & (o.esize - 1)))) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d_out) & (o.esize - 1)) return hipErrorInvalidValue;
    const uint64_t gx = (uint64_t(ow) + 15) / 16, gy = (uint64_t(oh) + 15) / 16;
    if (gx * gy > 0x7FFFFFFFull) return hipErrorInvalidValue;  // (an output of 2^39 pixels: no buffer holds it)
    const dim3 grid(uint32_t(gx * gy), views);
    dispatch_out(o, [&](auto E, auto CHW, auto LUT) {
        launch_c<E(), CHW(), LUT()>(grid, stream, d_box, d_ws, d_tabs, d_fill, d_table, d_out, c, bw, bh, w, h, ow, oh);
    });
    return hipGetLastError();
}

hipError_t launch_persp(const uint8_t* d_box, const PerspEntry* d_ps, const uint8_t* d_fill, const void* d_table, const OutFormat& o, void* d_out,
                        uint32_t views, uint32_t c, uint32_t bw, uint32_t bh, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, hipStream_t stream) {
    if (!views || views > 65535 || !c || c > 255 || !w || !h || !ow || !oh || !d_ps || !d_fill || !d_out) return hipErrorInvalidValue;
    if (w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || bw > 0x7FFFFFFFu || bh > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d_ps) & 7) return hipErrorInvalidValue;
    if (!o.plain && (!d_table || (reinterpret_cast<uintptr_t>(d_table) & (o.esize - 1)))) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d_out) & (o.esize - 1)) return hipErrorInvalidValue;
    const uint64_t gx = (uint64_t(ow) + 15) / 16, gy = (uint64_t(oh) + 15) / 16;
    if (gx * gy > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid(uint32_t(gx * gy), views);
    dispatch_out(o, [&](auto E, auto CHW, auto LUT) {
        launch_persp_c<E(), CHW(), LUT()>(grid, stream, d_box, d_ps, d_fill, d_table, d_out, c, bw, bh, w, h, ow, oh);
    });
    return hipGetLastError();
}

}  // namespace llcomp_mi
