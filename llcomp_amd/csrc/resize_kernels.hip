// resize_kernels.hip -- the resampling of a resized regions decode (llcomp_mi_codec_decode_resized_regions): every frame's rectangle,
// cut from its box by the regions decode, to one output shape with the triangle filter with antialiasing (PIL's bilinear, torch's
// interpolate(mode="bilinear", align_corners=False, antialias=True)) in Q22 integers, horizontal pass first, rounded to u8 in between.
// The rule is include/llcomp_mi.h's llcomp_mi_resize_weights; the GPU runs exactly the weights resize_weights computes.
#include "resize.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/llcomp_mi.h"

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

namespace {

// Clamped at both ends: bicubic and Lanczos have negative lobes, so a sum can leave [0, 255] on either side.  One v_med3_i32, written
// out: from min(max(x >> 22, 0), 255) hipcc (ROCm 7.0) selects gfx950's v_ashr_pk_u8_i32 for two channels at a time and ORs the other
// channels into the register as if its upper half were zero, and on the MI355X the c = 4 paths then stored wrong bytes in channels
// 2 and 3 (channels 0 and 1, the packed pair, were right).  The asm keeps the value opaque, so every channel takes this one instruction.
__device__ __forceinline__ uint32_t q22_round(int32_t acc) {
    const int32_t v = (acc + (1 << 21)) >> 22;
    int32_t r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(255));
    return uint32_t(r);
}

// Horizontal pass: one lane per (entry, rectangle row, output x), all channels; lanes of a row read neighbouring weights (tap-major).
// Entry f (blockIdx.y) reads its rectangle from box e.box -- its own frame's for a resized regions decode, the box of the view's frame
// for a views decode, where several entries share a box -- and writes rows [0, rh) of mid[f], whose pitch mh is the launch's largest
// rectangle height, not the box's.
template <int C>
__global__ __launch_bounds__(256) void k_resize_h(const uint8_t* __restrict__ box, uint8_t* __restrict__ mid, const ResizeFrame* __restrict__ tab,
                                                  const int32_t* __restrict__ wts, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow,
                                                  uint32_t c_rt) {
    const uint32_t c = C ? uint32_t(C) : c_rt;
    const uint32_t f = blockIdx.y;
    const ResizeFrame& e = tab[f];
    const uint32_t rh = e.rh, kx = e.kx;
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= uint64_t(rh) * ow) return;
    const uint32_t r = uint32_t(i / ow), x = uint32_t(i - uint64_t(r) * ow);
    const int32_t* lo = wts + e.hx;
    const int32_t* q = lo + ow + x;
    const uint8_t* src = box + ((size_t(e.box) * bh + e.oy + r) * bw + e.ox + uint32_t(lo[x])) * c;
    uint8_t* dst = mid + ((size_t(f) * mh + r) * ow + x) * c;
    if constexpr (C == 4) {
        int32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t j = 0; j < kx; ++j) {
            const int32_t wj = q[size_t(j) * ow];
            const uint32_t p = *reinterpret_cast<const uint32_t*>(src + 4 * j);
            a0 += wj * int32_t(p & 0xFF);
            a1 += wj * int32_t((p >> 8) & 0xFF);
            a2 += wj * int32_t((p >> 16) & 0xFF);
            a3 += wj * int32_t(p >> 24);
        }
        *reinterpret_cast<uint32_t*>(dst) = q22_round(a0) | (q22_round(a1) << 8) | (q22_round(a2) << 16) | (q22_round(a3) << 24);
    } else if constexpr (C == 3) {
        int32_t a0 = 0, a1 = 0, a2 = 0;
        for (uint32_t j = 0; j < kx; ++j) {
            const int32_t wj = q[size_t(j) * ow];
            a0 += wj * int32_t(src[3 * j]);
            a1 += wj * int32_t(src[3 * j + 1]);
            a2 += wj * int32_t(src[3 * j + 2]);
        }
        dst[0] = uint8_t(q22_round(a0));
        dst[1] = uint8_t(q22_round(a1));
        dst[2] = uint8_t(q22_round(a2));
    } else {
        for (uint32_t ch = 0; ch < c; ++ch) {
            int32_t a = 0;
            for (uint32_t j = 0; j < kx; ++j) a += q[size_t(j) * ow] * int32_t(src[size_t(j) * c + ch]);
            dst[ch] = uint8_t(q22_round(a));
        }
    }
}

// Vertical pass: one lane per output pixel, coalesced along x; a row's weights are the same for all its lanes.  The mirror is applied
// on the store.  Entry f reads mid[f] (pitch mh rows) and writes out[f].
template <int C>
__global__ __launch_bounds__(256) void k_resize_v(const uint8_t* __restrict__ mid, uint8_t* __restrict__ out, const ResizeFrame* __restrict__ tab,
                                                  const int32_t* __restrict__ wts, uint32_t mh, uint32_t ow, uint32_t oh, uint32_t c_rt) {
    const uint32_t c = C ? uint32_t(C) : c_rt;
    const uint32_t f = blockIdx.y;
    const ResizeFrame& e = tab[f];
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= uint64_t(oh) * ow) return;
    const uint32_t y = uint32_t(i / ow), x = uint32_t(i - uint64_t(y) * ow), ky = e.ky;
    const int32_t* lo = wts + e.vy;
    const int32_t* q = lo + oh + y;
    const size_t stride = size_t(ow) * c;
    const uint8_t* src = mid + ((size_t(f) * mh + uint32_t(lo[y])) * ow + x) * c;
    const uint32_t xo = (e.flags & 1u) ? ow - 1 - x : x;
    uint8_t* dst = out + ((size_t(f) * oh + y) * ow + xo) * c;
    if constexpr (C == 4) {
        int32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint32_t p = *reinterpret_cast<const uint32_t*>(src + j * stride);
            a0 += wj * int32_t(p & 0xFF);
            a1 += wj * int32_t((p >> 8) & 0xFF);
            a2 += wj * int32_t((p >> 16) & 0xFF);
            a3 += wj * int32_t(p >> 24);
        }
        *reinterpret_cast<uint32_t*>(dst) = q22_round(a0) | (q22_round(a1) << 8) | (q22_round(a2) << 16) | (q22_round(a3) << 24);
    } else if constexpr (C == 3) {
        int32_t a0 = 0, a1 = 0, a2 = 0;
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint8_t* p = src + j * stride;
            a0 += wj * int32_t(p[0]);
            a1 += wj * int32_t(p[1]);
            a2 += wj * int32_t(p[2]);
        }
        dst[0] = uint8_t(q22_round(a0));
        dst[1] = uint8_t(q22_round(a1));
        dst[2] = uint8_t(q22_round(a2));
    } else {
        for (uint32_t ch = 0; ch < c; ++ch) {
            int32_t a = 0;
            for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride + ch]);
            dst[ch] = uint8_t(q22_round(a));
        }
    }
}

template <int E> struct Elem;
template <> struct Elem<1> { using T = uint8_t; };
template <> struct Elem<2> { using T = uint16_t; };
template <> struct Elem<4> { using T = uint32_t; };

// Vertical pass with an output format: k_resize_v's u8 value of every channel, looked up in the format's table (output_table, [c][256]
// elements of E bytes) and stored in the layout.  CHW: one element per channel plane, so a wave's lanes store consecutive elements of
// every plane (reversed under the mirror); HWC: the pixel's c elements, one vector store for C = 4 (the caller checks that d_out is
// aligned for it).  C = 1 / 3 / 4 copy the table to LDS (at most 4 KiB); the generic path (C = 0, any c up to 255) reads it where it lies.
template <int C, int E, bool CHW>
__global__ __launch_bounds__(256) void k_resize_v_out(const uint8_t* __restrict__ mid, void* __restrict__ out, const ResizeFrame* __restrict__ tab,
                                                      const int32_t* __restrict__ wts, const uint32_t* __restrict__ table, uint32_t mh, uint32_t ow,
                                                      uint32_t oh, uint32_t c_rt) {
    using T = typename Elem<E>::T;
    const uint32_t c = C ? uint32_t(C) : c_rt;
    __shared__ uint32_t s_lut[C ? C * 64 * E : 1];
    if constexpr (C != 0) {
        for (uint32_t j = threadIdx.x; j < uint32_t(C * 64 * E); j += 256) s_lut[j] = table[j];
        __syncthreads();
    }
    const T* __restrict__ lut = reinterpret_cast<const T*>(C ? s_lut : table);
    const uint32_t f = blockIdx.y;
    const ResizeFrame& e = tab[f];
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= uint64_t(oh) * ow) return;
    const uint32_t y = uint32_t(i / ow), x = uint32_t(i - uint64_t(y) * ow), ky = e.ky;
    const int32_t* lo = wts + e.vy;
    const int32_t* q = lo + oh + y;
    const size_t stride = size_t(ow) * c;
    const uint8_t* src = mid + ((size_t(f) * mh + uint32_t(lo[y])) * ow + x) * c;
    const uint32_t xo = (e.flags & 1u) ? ow - 1 - x : x;
    T* const o = static_cast<T*>(out);
    const size_t plane = size_t(oh) * ow, px = size_t(y) * ow + xo;  // (CHW: element [f][ch][y][xo] = (f * c + ch) * plane + px)
    auto put = [&](uint32_t ch, uint32_t v) {
        if constexpr (CHW)
            o[(size_t(f) * c + ch) * plane + px] = lut[ch * 256 + v];
        else
            o[(size_t(f) * plane + px) * c + ch] = lut[ch * 256 + v];
    };
    if constexpr (C == 4) {
        int32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint32_t p = *reinterpret_cast<const uint32_t*>(src + j * stride);
            a0 += wj * int32_t(p & 0xFF);
            a1 += wj * int32_t((p >> 8) & 0xFF);
            a2 += wj * int32_t((p >> 16) & 0xFF);
            a3 += wj * int32_t(p >> 24);
        }
        const uint32_t l0 = lut[q22_round(a0)], l1 = lut[256 + q22_round(a1)], l2 = lut[512 + q22_round(a2)], l3 = lut[768 + q22_round(a3)];
        if constexpr (CHW) {
            o[size_t(f) * 4 * plane + px] = T(l0);
            o[(size_t(f) * 4 + 1) * plane + px] = T(l1);
            o[(size_t(f) * 4 + 2) * plane + px] = T(l2);
            o[(size_t(f) * 4 + 3) * plane + px] = T(l3);
        } else {
            T* d = o + (size_t(f) * plane + px) * 4;
            if constexpr (E == 1)
                *reinterpret_cast<uint32_t*>(d) = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
            else if constexpr (E == 2)
                *reinterpret_cast<uint2*>(d) = make_uint2(l0 | (l1 << 16), l2 | (l3 << 16));
            else
                *reinterpret_cast<uint4*>(d) = make_uint4(l0, l1, l2, l3);
        }
    } else if constexpr (C == 3) {
        int32_t a0 = 0, a1 = 0, a2 = 0;
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint8_t* p = src + j * stride;
            a0 += wj * int32_t(p[0]);
            a1 += wj * int32_t(p[1]);
            a2 += wj * int32_t(p[2]);
        }
        put(0, q22_round(a0));
        put(1, q22_round(a1));
        put(2, q22_round(a2));
    } else if constexpr (C == 1) {
        int32_t a = 0;
        for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride]);
        put(0, q22_round(a));
    } else {
        for (uint32_t ch = 0; ch < c; ++ch) {
            int32_t a = 0;
            for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride + ch]);
            put(ch, q22_round(a));
        }
    }
}

template <int E, bool CHW>
void launch_v_out(dim3 gv, hipStream_t stream, const uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const uint32_t* d_table,
                  uint32_t c, uint32_t mh, uint32_t ow, uint32_t oh, bool vec4) {
    const dim3 blk(256);
    switch (c) {
        case 1: k_resize_v_out<1, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;
        case 3: k_resize_v_out<3, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;
        case 4:
            if (CHW || vec4)
                k_resize_v_out<4, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c);
            else
                k_resize_v_out<0, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c);
            break;
        default: k_resize_v_out<0, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;
    }
}

}  // namespace

// The horizontal pass of both launchers.
static hipError_t launch_h(const uint8_t* d_box, uint8_t* d_mid, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t frames, uint32_t c, uint32_t bw,
                           uint32_t bh, uint32_t mh, uint32_t ow, hipStream_t stream) {
    const uint64_t hb = (uint64_t(mh) * ow + 255) / 256;
    if (hb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gh(uint32_t(hb), frames), blk(256);
    switch (c) {
        case 1: k_resize_h<1><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;
        case 3: k_resize_h<3><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;
        case 4: k_resize_h<4><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;
        default: k_resize_h<0><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;
    }
    return hipSuccess;
}

hipError_t launch_resize(const uint8_t* d_box, uint8_t* d_mid, uint8_t* d_px, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t frames,
                         uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow, uint32_t oh, hipStream_t stream) {
    if (!frames || !c || !bw || !bh || !mh || !ow || !oh || frames > 65535) return hipErrorInvalidValue;
    const uint64_t vb = (uint64_t(oh) * ow + 255) / 256;
    if (vb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gv(uint32_t(vb), frames), blk(256);
    // (the box and the intermediate are the codec's own, 4-byte aligned; the output is the caller's: 32-bit stores only when aligned)
    const bool out4 = (reinterpret_cast<uintptr_t>(d_px) & 3u) == 0;
    if (hipError_t err = launch_h(d_box, d_mid, d_tab, d_w, frames, c, bw, bh, mh, ow, stream)) return err;
    switch (c) {
        case 1: k_resize_v<1><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;
        case 3: k_resize_v<3><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;
        case 4:
            if (out4)
                k_resize_v<4><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c);
            else
                k_resize_v<0><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c);
            break;
        default: k_resize_v<0><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;
    }
    return hipGetLastError();
}

hipError_t launch_resize_out(const uint8_t* d_box, uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const void* d_table,
                             const OutFormat& o, uint32_t frames, uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow,
                             uint32_t oh, hipStream_t stream) {
    if (o.plain) return launch_resize(d_box, d_mid, static_cast<uint8_t*>(d_out), d_tab, d_w, frames, c, bw, bh, mh, ow, oh, stream);
    if (!frames || !c || c > 255 || !bw || !bh || !mh || !ow || !oh || frames > 65535 || !d_table) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d_table) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & (o.esize - 1))) return hipErrorInvalidValue;
    const uint64_t vb = (uint64_t(oh) * ow + 255) / 256;
    if (vb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gv(uint32_t(vb), frames);
    if (hipError_t err = launch_h(d_box, d_mid, d_tab, d_w, frames, c, bw, bh, mh, ow, stream)) return err;
    // (HWC at c = 4 stores a pixel's 4 elements at once: only where d_out is aligned to 4 elements)
    const bool vec4 = (reinterpret_cast<uintptr_t>(d_out) & (4 * o.esize - 1)) == 0;
    const uint32_t* t = static_cast<const uint32_t*>(d_table);
    const bool chw = o.layout == LLCOMP_MI_LAYOUT_CHW;
    if (o.esize == 1)  // (U8 CHW: U8 HWC is plain)
        launch_v_out<1, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4);
    else if (o.esize == 2)
        chw ? launch_v_out<2, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4)
            : launch_v_out<2, false>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4);
    else
        chw ? launch_v_out<4, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4)
            : launch_v_out<4, false>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4);
    return hipGetLastError();
}

}  // namespace llcomp_mi

extern "C" uint32_t llcomp_mi_resize_weights(uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q) {
    return llcomp_mi::resize_weights(LLCOMP_MI_FILTER_BILINEAR, in_len, out_len, lo, q);
}

extern "C" uint32_t llcomp_mi_resize_filter_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q) {
    return llcomp_mi::resize_weights(filter, in_len, out_len, lo, q);
}

extern "C" int llcomp_mi_output_table(const llcomp_mi_output_format* fmt, uint32_t c, void* table) {
    llcomp_mi::OutFormat o;
    if (!fmt || !table) return LLCOMP_MI_BAD_ARGS;
    if (int rc = llcomp_mi::check_output_format(fmt, c, o)) return rc;
    llcomp_mi::output_table(fmt, c, o, static_cast<uint8_t*>(table));
    return LLCOMP_MI_OK;
}
