// mix_rule.hpp -- the rule of the batch mixing (include/llcomp_mi.h: "Batch mixing"), stated ONCE: these functions are compiled into the
// kernels (mix_kernels.hip) and into llcomp_mi_mix_reference and the planner's checks (mix_plan.cpp).  The rule is torch's on the CPU:
// every product and the sum of a blend in IEEE binary32, each rounded by itself and then to the element's type, so nothing here may be
// contracted into a fused multiply-add: hipcc does that on the device by default, and the pragma below switches it off for every file
// that includes this header.  The element's size and the shape of a batch: batch_ops.hpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "batch_ops.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
// (g++ builds of the host checks target baseline x86-64, which has no fused multiply-add to contract into)

namespace llcomp_mi {

LLMI_HD inline uint32_t mix_f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
LLMI_HD inline float mix_f32_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
LLMI_HD inline bool mix_finite(float f) { return (mix_f32_bits(f) & 0x7F800000u) != 0x7F800000u; }

// An element's bits widened to binary32 (exact for every dtype) ...
template <uint32_t DT>
LLMI_HD inline float mix_widen(uint32_t b) {
    if constexpr (DT == LLCOMP_MI_DTYPE_F32) {
        return mix_f32_of(b);
    } else if constexpr (DT == LLCOMP_MI_DTYPE_BF16) {
        return mix_f32_of(b << 16);
    } else if constexpr (DT == LLCOMP_MI_DTYPE_F16) {
#if defined(__HIP_DEVICE_COMPILE__)
        return float(__builtin_bit_cast(_Float16, uint16_t(b)));  // (the conversion is exact: one instruction says what the integers below say)
#else
        const uint32_t sign = (b & 0x8000u) << 16, em = b & 0x7FFFu;
        if (em >= 0x7C00u) return mix_f32_of(sign | 0x7F800000u | ((em & 0x3FFu) << 13));
        if (em >= 0x0400u) return mix_f32_of(sign | ((em << 13) + 0x38000000u));
        const float m = float(int32_t(em)) * 5.9604644775390625e-08f;  // a subnormal: em * 2^-24
        return sign ? -m : m;
#endif
    } else {
        return float(int32_t(b));
    }
}
// ... and a binary32 value rounded to the dtype, to nearest even, overflow to +-inf; a NaN stays some NaN
template <uint32_t DT>
LLMI_HD inline uint32_t mix_narrow(float f) {
    if constexpr (DT == LLCOMP_MI_DTYPE_F32) {
        return mix_f32_bits(f);
    } else if constexpr (DT == LLCOMP_MI_DTYPE_BF16) {
        const uint32_t x = mix_f32_bits(f);
        if ((x & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
        return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
    } else if constexpr (DT == LLCOMP_MI_DTYPE_F16) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_bit_cast(uint16_t, _Float16(f));  // (round to nearest even, the default mode: v_cvt_f16_f32)
#else
        const uint32_t u = mix_f32_bits(f), sign = (u >> 16) & 0x8000u, x = u & 0x7FFFFFFFu;
        if (x > 0x7F800000u) return sign | 0x7E00u;
        if (x >= 0x477FF000u) return sign | 0x7C00u;  // 65520 and above round to inf
        if (x < 0x38800000u) return sign | (mix_f32_bits(mix_f32_of(x) + 0.5f) - 0x3F000000u);  // below 2^-14: the sum's ulp is 2^-24, binary16's subnormal step
        return sign | ((x + 0xC8000FFFu + ((x >> 13) & 1u)) >> 13);
#endif
    } else {
        return uint32_t(int32_t(f));
    }
}
// rd of the rule: mix_narrow, and the dtype's one quiet NaN for a NaN
template <uint32_t DT>
LLMI_HD inline uint32_t mix_round(float f) {
    if (f != f) return DT == LLCOMP_MI_DTYPE_F32 ? 0x7FC00000u : DT == LLCOMP_MI_DTYPE_F16 ? 0x7E00u : 0x7FC0u;
    return mix_narrow<DT>(f);
}

// A product as a binary32 value of its own.  On the device hipcc folds a multiply and the rounding to binary16 behind it into one
// v_fma_mixlo_f16 with an addend of +0, and -0 + +0 is +0: a product of -0 would lose its sign.  The empty statement keeps the two apart.
LLMI_HD inline float mix_product(float a, float b) {
    float p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    return p;
}

// BLEND of the elements own and partner
template <uint32_t DT>
LLMI_HD inline uint32_t mix_blend(uint32_t own, uint32_t partner, float w_own, float w_partner) {
    const float a = mix_product(mix_widen<DT>(own), w_own);
    const float b = mix_product(mix_widen<DT>(partner), w_partner);
    const float s = mix_widen<DT>(mix_narrow<DT>(a)) + mix_widen<DT>(mix_narrow<DT>(b));
    return mix_round<DT>(s);
}

// (x, y) lies in the rectangle r = {x, y, w, h}; an empty one holds nothing
LLMI_HD inline bool mix_rect_empty(const uint32_t* r) { return !r[2] || !r[3]; }
LLMI_HD inline bool mix_in_rect(const uint32_t* r, uint32_t x, uint32_t y) { return x >= r[0] && x - r[0] < r[2] && y >= r[1] && y - r[1] < r[3]; }
// ... and the rectangle lies in ow x oh (an empty one does wherever it is)
LLMI_HD inline bool mix_rect_ok(const uint32_t* r, uint32_t ow, uint32_t oh) {
    return mix_rect_empty(r) || (r[0] < ow && r[2] <= ow - r[0] && r[1] < oh && r[3] <= oh - r[1]);
}

// What the rule reads of one record beside the weights and the rectangles: the sample mixes (its partner is another sample) and blends
struct MixWhat {
    bool mixes, blend;
};
LLMI_HD inline MixWhat mix_what(const llcomp_mi_mix_sample& s, uint32_t i) { return MixWhat{s.partner != i, (s.flags & LLCOMP_MI_MIX_BLEND) != 0}; }

// The rule for one element of sample i.  own / partner: the two samples' elements as they stood before the call; ev: the erase value of
// the element's channel in the dtype; in_erase_own / in_erase_partner / in_box: the element's pixel lies in erase_i / erase_p / box_i.
template <uint32_t DT>
LLMI_HD inline uint32_t mix_element(MixWhat what, float w_own, float w_partner, uint32_t own, uint32_t partner, uint32_t ev, bool in_erase_own,
                                    bool in_erase_partner, bool in_box) {
    const uint32_t e_own = in_erase_own ? ev : own;
    if (!what.mixes) return e_own;
    const uint32_t e_partner = in_erase_partner ? ev : partner;
    if (in_box) return e_partner;
    if constexpr (DT != LLCOMP_MI_DTYPE_U8) {
        if (what.blend) return mix_blend<DT>(e_own, e_partner, w_own, w_partner);
    }
    return e_own;
}

// Where element e of a sample lies: channel, row and column, in either layout ...
struct MixAt {
    uint32_t ch, y, x;
};
template <bool CHW>
LLMI_HD inline MixAt mix_at(uint64_t e, uint32_t c, uint32_t ow, uint32_t oh) {
    const uint64_t plane = uint64_t(ow) * oh;
    if (!((e | plane) >> 32)) {  // (the same quotients in 32 bits, which is what the GPU divides in)
        const uint32_t e32 = uint32_t(e), pl = uint32_t(plane), px = CHW ? e32 % pl : e32 / c;
        return MixAt{CHW ? e32 / pl : e32 % c, px / ow, px % ow};
    }
    const uint64_t px = CHW ? e % plane : e / c;
    return MixAt{uint32_t(CHW ? e / plane : e % c), uint32_t(px / ow), uint32_t(px % ow)};
}
// ... and where the element behind it does
template <bool CHW>
LLMI_HD inline MixAt mix_next(MixAt a, uint32_t c, uint32_t ow, uint32_t oh) {
    if constexpr (CHW) {
        if (++a.x == ow) {
            a.x = 0;
            if (++a.y == oh) a.y = 0, ++a.ch;
        }
    } else {
        if (++a.ch == c) {
            a.ch = 0;
            if (++a.x == ow) a.x = 0, ++a.y;
        }
    }
    return a;
}

// The erase value v of a channel in the dtype; false for one the dtype cannot take (not finite; U8: no integer from 0 to 255)
LLMI_HD inline bool mix_erase_bits(uint32_t dtype, float v, uint32_t& bits) {
    if (!mix_finite(v)) return false;
    switch (dtype) {
        case LLCOMP_MI_DTYPE_U8:
            if (!(v >= 0.0f && v <= 255.0f) || float(int32_t(v)) != v) return false;
            bits = uint32_t(int32_t(v));
            return true;
        case LLCOMP_MI_DTYPE_F32: bits = mix_round<LLCOMP_MI_DTYPE_F32>(v); return true;
        case LLCOMP_MI_DTYPE_F16: bits = mix_round<LLCOMP_MI_DTYPE_F16>(v); return true;
        case LLCOMP_MI_DTYPE_BF16: bits = mix_round<LLCOMP_MI_DTYPE_BF16>(v); return true;
        default: return false;
    }
}
// ... and a call's value per channel (the mixing's erase value, the composition's fill; NULL: zeros) as bits[c] in the dtype; BAD_ARGS,
// and bits as it was, for a value the dtype cannot take
inline int batch_value_bits(uint32_t dtype, uint32_t c, const float* values, std::vector<uint32_t>& bits) {
    std::vector<uint32_t> b(c, 0u);
    for (uint32_t ch = 0; ch < c; ++ch)
        if (!mix_erase_bits(dtype, values ? values[ch] : 0.0f, b[ch])) return LLCOMP_MI_BAD_ARGS;
    bits.swap(b);
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi
