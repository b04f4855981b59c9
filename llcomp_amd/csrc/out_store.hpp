// out_store.hpp -- one element of a formatted output (include/llcomp_mi.h: llcomp_mi_output_format), as the kernels behind a group's
// output write it: the gather of the warped views (warp_kernels.hip) and the last step of a photometric chain (photo_kernels.hip).
// (The vertical resample pass keeps its own text, resize_v_out_body.inc says why; and resize_kernels.hip's launch_resize_out keeps its
// own switch over the format: its plain case is another launcher and its kernels have no LUT parameter, so dispatch_out would
// instantiate kernels that do not exist.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "resize_plan.hpp"

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

// The one switch over a checked format: f(E, CHW, LUT) -- the element size, the layout and whether there is a table, as integral
// constants (E() is the value) -- in exactly the combinations the kernels are instantiated for: plain U8 HWC has no table, U8 CHW and
// the 2- and 4-byte elements in either layout go through theirs.
template <class F>
void dispatch_out(const OutFormat& o, F&& f) {
    using std::false_type;
    using std::true_type;
    const bool chw = o.layout == LLCOMP_MI_LAYOUT_CHW;
    if (o.plain)
        f(std::integral_constant<int, 1>{}, false_type{}, false_type{});
    else if (o.esize == 1)  // (U8 CHW: U8 HWC is plain)
        f(std::integral_constant<int, 1>{}, true_type{}, true_type{});
    else if (o.esize == 2)
        chw ? f(std::integral_constant<int, 2>{}, true_type{}, true_type{}) : f(std::integral_constant<int, 2>{}, false_type{}, true_type{});
    else
        chw ? f(std::integral_constant<int, 4>{}, true_type{}, true_type{}) : f(std::integral_constant<int, 4>{}, false_type{}, true_type{});
}

}  // namespace llcomp_mi
