// resize_kernels.hip -- the resampling of a resized regions decode (llcomp_mi_codec_decode_resized_regions): every frame's rectangle,
// cut from its box by the regions decode, to one output shape with the triangle filter with antialiasing (PIL's bilinear, torch's
// interpolate(mode="bilinear", align_corners=False, antialias=True)) in Q22 integers, horizontal pass first, rounded to u8 in between.
// The rule is include/llcomp_mi.h's llcomp_mi_resize_weights; the GPU runs exactly the weights resize_weights computes.
#include "resize.hpp"

namespace llcomp_mi {

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
//
// BIAS (a padded call with a constant fill other than 0, include/llcomp_mi.h: llcomp_mi_pad): the accumulator of channel ch starts at
// bias[x] * fill[ch] -- the weight of the taps that fell outside the image times the fill -- with the entry's bias arrays at e.pad[0]
// (horizontal [ow], then vertical [oh]) and the call's c fill values at e.pad[1] of the weights.  Both are read ahead of the tap loop.
template <int C, bool BIAS>
__device__ __forceinline__ void resize_h(const uint8_t* box, uint8_t* mid, const ResizeFrame* tab,
                                         const int32_t* wts, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow, uint32_t c_rt) {
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
    int32_t b = 0;
    const int32_t* fill = nullptr;
    if constexpr (BIAS) {
        b = wts[e.pad[0] + x];
        fill = wts + e.pad[1];
    }
    auto start = [&](uint32_t ch) { return BIAS ? b * fill[ch] : int32_t(0); };
    if constexpr (C == 4) {
        int32_t a0 = start(0), a1 = start(1), a2 = start(2), a3 = start(3);
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
        int32_t a0 = start(0), a1 = start(1), a2 = start(2);
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
            int32_t a = start(ch);
            for (uint32_t j = 0; j < kx; ++j) a += q[size_t(j) * ow] * int32_t(src[size_t(j) * c + ch]);
            dst[ch] = uint8_t(q22_round(a));
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_resize_h(const uint8_t* __restrict__ box, uint8_t* __restrict__ mid, const ResizeFrame* __restrict__ tab,
                                                  const int32_t* __restrict__ wts, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow,
                                                  uint32_t c_rt) {
    resize_h<C, false>(box, mid, tab, wts, bw, bh, mh, ow, c_rt);
}
template <int C>
__global__ __launch_bounds__(256) void k_resize_h_bias(const uint8_t* __restrict__ box, uint8_t* __restrict__ mid,
                                                       const ResizeFrame* __restrict__ tab, const int32_t* __restrict__ wts, uint32_t bw,
                                                       uint32_t bh, uint32_t mh, uint32_t ow, uint32_t c_rt) {
    resize_h<C, true>(box, mid, tab, wts, bw, bh, mh, ow, c_rt);
}

// Vertical pass: one lane per output pixel, coalesced along x; a row's weights are the same for all its lanes.  The mirror is applied
// on the store.  Entry f reads mid[f] (pitch mh rows) and writes out[f].  BIAS: the accumulators start at bias[ow + y] * fill[ch].
template <int C, bool BIAS>
__device__ __forceinline__ void resize_v(const uint8_t* mid, uint8_t* out, const ResizeFrame* tab,
                                         const int32_t* wts, uint32_t mh, uint32_t ow, uint32_t oh, uint32_t c_rt) {
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
    int32_t b = 0;
    const int32_t* fill = nullptr;
    if constexpr (BIAS) {
        b = wts[e.pad[0] + ow + y];
        fill = wts + e.pad[1];
    }
    auto start = [&](uint32_t ch) { return BIAS ? b * fill[ch] : int32_t(0); };
    if constexpr (C == 4) {
        int32_t a0 = start(0), a1 = start(1), a2 = start(2), a3 = start(3);
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
        int32_t a0 = start(0), a1 = start(1), a2 = start(2);
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
            int32_t a = start(ch);
            for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride + ch]);
            dst[ch] = uint8_t(q22_round(a));
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_resize_v(const uint8_t* __restrict__ mid, uint8_t* __restrict__ out, const ResizeFrame* __restrict__ tab,
                                                  const int32_t* __restrict__ wts, uint32_t mh, uint32_t ow, uint32_t oh, uint32_t c_rt) {
    resize_v<C, false>(mid, out, tab, wts, mh, ow, oh, c_rt);
}
template <int C>
__global__ __launch_bounds__(256) void k_resize_v_bias(const uint8_t* __restrict__ mid, uint8_t* __restrict__ out, const ResizeFrame* __restrict__ tab,
                                                       const int32_t* __restrict__ wts, uint32_t mh, uint32_t ow, uint32_t oh, uint32_t c_rt) {
    resize_v<C, true>(mid, out, tab, wts, mh, ow, oh, c_rt);
}

template <int E> struct Elem;
template <> struct Elem<1> { using T = uint8_t; };
template <> struct Elem<2> { using T = uint16_t; };
template <> struct Elem<4> { using T = uint32_t; };

// Vertical pass with an output format: k_resize_v's u8 value of every channel, looked up in the format's table (output_table, [c][256]
// elements of E bytes) and stored in the layout.  CHW: one element per channel plane, so a wave's lanes store consecutive elements of
// every plane (reversed under the mirror); HWC: the pixel's c elements, one vector store for C = 4 (the caller checks that d_out is
// aligned for it).  C = 1 / 3 / 4 copy the table to LDS (at most 4 KiB); the generic path (C = 0, any c up to 255) reads it where it lies.
// BIAS as in the vertical pass; the body is resize_v_out_body.inc for both kernels.
template <int C, int E, bool CHW>
__global__ __launch_bounds__(256) void k_resize_v_out(const uint8_t* __restrict__ mid, void* __restrict__ out, const ResizeFrame* __restrict__ tab,
                                                      const int32_t* __restrict__ wts, const uint32_t* __restrict__ table, uint32_t mh, uint32_t ow,
                                                      uint32_t oh, uint32_t c_rt) {
    constexpr bool BIAS = false;
#include "resize_v_out_body.inc"
}
template <int C, int E, bool CHW>
__global__ __launch_bounds__(256) void k_resize_v_out_bias(const uint8_t* __restrict__ mid, void* __restrict__ out,
                                                           const ResizeFrame* __restrict__ tab, const int32_t* __restrict__ wts,
                                                           const uint32_t* __restrict__ table, uint32_t mh, uint32_t ow, uint32_t oh,
                                                           uint32_t c_rt) {
    constexpr bool BIAS = true;
#include "resize_v_out_body.inc"
}

// (one switch for both forms of a kernel: K is k_resize_x or k_resize_x_bias)
#define LLMI_V_OUT(K)                                                                                                \
    switch (c) {                                                                                                     \
        case 1: K<1, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;       \
        case 3: K<3, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;       \
        case 4:                                                                                                      \
            if (CHW || vec4)                                                                                         \
                K<4, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c);              \
            else                                                                                                     \
                K<0, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c);              \
            break;                                                                                                   \
        default: K<0, E, CHW><<<gv, blk, 0, stream>>>(d_mid, d_out, d_tab, d_w, d_table, mh, ow, oh, c); break;      \
    }
template <int E, bool CHW>
void launch_v_out(dim3 gv, hipStream_t stream, const uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const uint32_t* d_table,
                  uint32_t c, uint32_t mh, uint32_t ow, uint32_t oh, bool vec4, bool bias) {
    const dim3 blk(256);
    if (bias) {
        LLMI_V_OUT(k_resize_v_out_bias)
    } else {
        LLMI_V_OUT(k_resize_v_out)
    }
}
#undef LLMI_V_OUT

}  // namespace

// The horizontal pass of both launchers.
static hipError_t launch_h(const uint8_t* d_box, uint8_t* d_mid, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t frames, uint32_t c, uint32_t bw,
                           uint32_t bh, uint32_t mh, uint32_t ow, bool bias, hipStream_t stream) {
    const uint64_t hb = (uint64_t(mh) * ow + 255) / 256;
    if (hb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gh(uint32_t(hb), frames), blk(256);
#define LLMI_H(K)                                                                                    \
    switch (c) {                                                                                     \
        case 1: K<1><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;    \
        case 3: K<3><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;    \
        case 4: K<4><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;    \
        default: K<0><<<gh, blk, 0, stream>>>(d_box, d_mid, d_tab, d_w, bw, bh, mh, ow, c); break;   \
    }
    if (bias) {
        LLMI_H(k_resize_h_bias)
    } else {
        LLMI_H(k_resize_h)
    }
#undef LLMI_H
    return hipSuccess;
}

hipError_t launch_resize(const uint8_t* d_box, uint8_t* d_mid, uint8_t* d_px, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t frames,
                         uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow, uint32_t oh, hipStream_t stream, bool bias) {
    if (!frames || !c || !bw || !bh || !mh || !ow || !oh || frames > 65535) return hipErrorInvalidValue;
    const uint64_t vb = (uint64_t(oh) * ow + 255) / 256;
    if (vb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gv(uint32_t(vb), frames), blk(256);
    // (the box and the intermediate are the codec's own, 4-byte aligned; the output is the caller's: 32-bit stores only when aligned)
    const bool out4 = (reinterpret_cast<uintptr_t>(d_px) & 3u) == 0;
    if (hipError_t err = launch_h(d_box, d_mid, d_tab, d_w, frames, c, bw, bh, mh, ow, bias, stream)) return err;
#define LLMI_V(K)                                                                               \
    switch (c) {                                                                                \
        case 1: K<1><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;    \
        case 3: K<3><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;    \
        case 4:                                                                                 \
            if (out4)                                                                           \
                K<4><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c);           \
            else                                                                                \
                K<0><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c);           \
            break;                                                                              \
        default: K<0><<<gv, blk, 0, stream>>>(d_mid, d_px, d_tab, d_w, mh, ow, oh, c); break;   \
    }
    if (bias) {
        LLMI_V(k_resize_v_bias)
    } else {
        LLMI_V(k_resize_v)
    }
#undef LLMI_V
    return hipGetLastError();
}

hipError_t launch_resize_out(const uint8_t* d_box, uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const void* d_table,
                             const OutFormat& o, uint32_t frames, uint32_t c, uint32_t bw, uint32_t bh, uint32_t mh, uint32_t ow,
                             uint32_t oh, hipStream_t stream, bool bias) {
    if (o.plain) return launch_resize(d_box, d_mid, static_cast<uint8_t*>(d_out), d_tab, d_w, frames, c, bw, bh, mh, ow, oh, stream, bias);
    if (!frames || !c || c > 255 || !bw || !bh || !mh || !ow || !oh || frames > 65535 || !d_table) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d_table) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & (o.esize - 1))) return hipErrorInvalidValue;
    const uint64_t vb = (uint64_t(oh) * ow + 255) / 256;
    if (vb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 gv(uint32_t(vb), frames);
    if (hipError_t err = launch_h(d_box, d_mid, d_tab, d_w, frames, c, bw, bh, mh, ow, bias, stream)) return err;
    // (HWC at c = 4 stores a pixel's 4 elements at once: only where d_out is aligned to 4 elements)
    const bool vec4 = (reinterpret_cast<uintptr_t>(d_out) & (4 * o.esize - 1)) == 0;
    const uint32_t* t = static_cast<const uint32_t*>(d_table);
    const bool chw = o.layout == LLCOMP_MI_LAYOUT_CHW;
    if (o.esize == 1)  // (U8 CHW: U8 HWC is plain)
        launch_v_out<1, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4, bias);
    else if (o.esize == 2)
        chw ? launch_v_out<2, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4, bias)
            : launch_v_out<2, false>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4, bias);
    else
        chw ? launch_v_out<4, true>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4, bias)
            : launch_v_out<4, false>(gv, stream, d_mid, d_out, d_tab, d_w, t, c, mh, ow, oh, vec4, bias);
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
