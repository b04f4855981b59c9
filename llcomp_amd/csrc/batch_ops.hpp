// batch_ops.hpp -- what every batch call knows (llcomp_mi_codec_mix_batch, _orient_batch, _compose_batch, _paste_batch and, for the shape
// check, _label_boxes; DESIGN.md "Batch calls: what the three share"): the element's size, the most samples of a batch, the check that a dense batch is one, and the way from a call's
// dtype and layout to the templates compiled for them.  Header only, host and device, plain C++: the planners (*_plan.cpp), the kernels
// (*_kernels.hip), the drivers (codec.hip) and the stand-alone host checks all read it.  The 16-byte chunk of the kernels: batch_chunk.hpp.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/llcomp_mi.h"
#include "geometry.hpp"

namespace llcomp_mi {

constexpr uint32_t kBatchMaxSamples = 65535;  // of a batch: a sample, or a segment of samples, is a row or a layer of the kernels' grids

// The element's size in bytes, 0 for a dtype that is none
LLMI_HD constexpr uint32_t batch_esize(uint32_t dtype) {
    return dtype == LLCOMP_MI_DTYPE_U8 ? 1u : dtype == LLCOMP_MI_DTYPE_F32 ? 4u : (dtype == LLCOMP_MI_DTYPE_F16 || dtype == LLCOMP_MI_DTYPE_BF16) ? 2u : 0u;
}

// A dense batch is one: n samples of c channels and ow x oh pixels in a known dtype and layout; BAD_ARGS for anything else
LLMI_HD inline int batch_check_shape(uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout) {
    if (!n || n > kBatchMaxSamples || !c || !ow || !oh || !batch_esize(dtype)) return LLCOMP_MI_BAD_ARGS;
    if (layout != LLCOMP_MI_LAYOUT_HWC && layout != LLCOMP_MI_LAYOUT_CHW) return LLCOMP_MI_BAD_ARGS;
    if (((static_cast<unsigned __int128>(c) * ow * oh * batch_esize(dtype) * n) >> 62) != 0) return LLCOMP_MI_BAD_ARGS;  // (no address space holds it)
    return LLCOMP_MI_OK;
}

// f(dt, chw) with the call's dtype and layout as constants (decltype(dt)::value, decltype(chw)::value), for the templates that are
// compiled per <DT, CHW>; false, and f not called, for a dtype that is none
template <class F>
inline bool batch_dispatch(uint32_t dtype, bool chw, F&& f) {
    auto by_layout = [&](auto dt) { chw ? f(dt, std::true_type{}) : f(dt, std::false_type{}); };
    switch (dtype) {
        case LLCOMP_MI_DTYPE_U8: by_layout(std::integral_constant<uint32_t, LLCOMP_MI_DTYPE_U8>{}); return true;
        case LLCOMP_MI_DTYPE_F32: by_layout(std::integral_constant<uint32_t, LLCOMP_MI_DTYPE_F32>{}); return true;
        case LLCOMP_MI_DTYPE_F16: by_layout(std::integral_constant<uint32_t, LLCOMP_MI_DTYPE_F16>{}); return true;
        case LLCOMP_MI_DTYPE_BF16: by_layout(std::integral_constant<uint32_t, LLCOMP_MI_DTYPE_BF16>{}); return true;
        default: return false;
    }
}

}  // namespace llcomp_mi
