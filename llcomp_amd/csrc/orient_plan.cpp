// orient_plan.cpp -- the host half of the batch orientation (orient_plan.hpp) and llcomp_mi_orient_reference.  Plain C++, no GPU.
#include "orient_plan.hpp"

#include <cstring>

#include "orient_rule.hpp"

namespace llcomp_mi {

int orient_check_call(uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const uint8_t* codes) {
    if (!codes) return LLCOMP_MI_BAD_ARGS;
    if (int rc = batch_check_shape(n, c, ow, oh, dtype, layout)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (codes[i] >= kOrientCodes || (orient_transposes(codes[i]) && ow != oh)) return LLCOMP_MI_BAD_ARGS;
    return LLCOMP_MI_OK;
}

void orient_table(uint32_t n, const uint8_t* codes, std::vector<OrientEntry>& table) {
    table.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (codes[i] != LLCOMP_MI_ORIENT_NONE) table.push_back(OrientEntry{i, codes[i]});
}

int orient_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const uint8_t* codes,
                     void* out) {
    if (!batch || !out) return LLCOMP_MI_BAD_ARGS;
    if (int rc = orient_check_call(n, c, ow, oh, dtype, layout, codes)) return rc;
    const uint32_t esize = batch_esize(dtype);
    const uint64_t sample_bytes = uint64_t(c) * ow * oh * esize;
    const uint8_t* src = static_cast<const uint8_t*>(batch);
    std::vector<uint8_t> before;
    if (out == batch) {  // every pixel from the batch as it stands before the call: a copy of it
        before.assign(src, src + size_t(sample_bytes * n));
        src = before.data();
    }
    uint8_t* o = static_cast<uint8_t*>(out);
    // a pixel is `unit` bytes, `planes` of them apart in a sample: HWC moves c elements at once, CHW one element in each of c planes
    const bool chw = layout == LLCOMP_MI_LAYOUT_CHW;
    const uint32_t planes = chw ? c : 1u;
    const size_t unit = chw ? esize : size_t(esize) * c;
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t p = 0; p < planes; ++p) {
            const uint8_t* s = src + uint64_t(i) * sample_bytes + uint64_t(p) * ow * oh * esize;
            uint8_t* d = o + uint64_t(i) * sample_bytes + uint64_t(p) * ow * oh * esize;
            for (uint32_t y = 0; y < oh; ++y)
                for (uint32_t x = 0; x < ow; ++x) {
                    const OrientXY at = orient_src(codes[i], ow, oh, x, y);
                    std::memcpy(d + (uint64_t(y) * ow + x) * unit, s + (uint64_t(at.y) * ow + at.x) * unit, unit);
                }
        }
    }
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_orient_tile(void) { return llcomp_mi::kOrientTile; }

int llcomp_mi_orient_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                               const uint8_t* codes, void* out) {
    return llcomp_mi::orient_reference(batch, n, c, ow, oh, dtype, layout, codes, out);
}

}  // extern "C"
