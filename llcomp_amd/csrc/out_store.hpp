// out_store.hpp -- one element of a formatted output (include/llcomp_mi.h: llcomp_mi_output_format), as the kernels behind a group's
// output write it: the gather of the warped views (warp_kernels.hip) and the last step of a photometric chain (photo_kernels.hip).
// (The vertical resample pass keeps its own text, resize_v_out_body.inc says why.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace llcomp_mi {

template <int E> struct OutElem;
template <> struct OutElem<1> { using T = uint8_t; };
template <> struct OutElem<2> { using T = uint16_t; };
template <> struct OutElem<4> { using T = uint32_t; };

// u8 value `val` of channel ch of pixel px (= y * ow + x) of view v -> o, through the format's table lut[c][256] where LUT, at
// [v][ch][px] (CHW) or [v][px][ch] (HWC); plane = oh * ow
template <class T, bool CHW, bool LUT>
__device__ __forceinline__ void out_store(T* o, const T* lut, size_t v, uint32_t c, size_t plane, size_t px, uint32_t ch, uint32_t val) {
    const T el = LUT ? lut[ch * 256 + val] : T(val);
    if constexpr (CHW)
        o[(v * c + ch) * plane + px] = el;
    else
        o[(v * plane + px) * c + ch] = el;
}

}  // namespace llcomp_mi
