// label_boxes.cpp -- the host half of the label boxes (include/llcomp_mi.h: "Label boxes"): llcomp_mi_label_boxes_reference, which walks
// the kernel's own bands and units (label_boxes_rule.hpp) on host memory, and the band's rows.  Plain C++, no GPU.
#include <cstring>

#include "label_boxes_rule.hpp"

namespace llcomp_mi {
namespace {

struct PlainMem {
    LabelChunk load16(uint64_t a) const {
        LabelChunk v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), 16);  // (little-endian hosts, like the containers)
        return v;
    }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) const {
        return *reinterpret_cast<const uint8_t*>(uintptr_t(a));
    }
};
struct PlainSink {
    llcomp_mi_label_box* recs;  // of the sample
    void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) { label_box_update(recs[id], x_first, x_end, y, length); }
};

}  // namespace
}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_label_boxes_rows(void) { return llcomp_mi::kLabelBoxRows; }

int llcomp_mi_label_boxes_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, llcomp_mi_label_box* out) {
    using namespace llcomp_mi;
    if (int rc = label_boxes_check_call(n, ow, oh)) return rc;
    if (!maps || !out) return LLCOMP_MI_BAD_ARGS;
    const LabelGeom g = label_geom(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    PlainMem mem;
    for (uint32_t i = 0; i < n; ++i) {
        PlainSink sink{out + size_t(i) * kLabelIds};
        for (uint32_t m = 0; m < kLabelIds; ++m) sink.recs[m] = label_box_identity(ow, oh);
        for (uint32_t b = 0; b < g.bands; ++b) {
            uint64_t sample, lo, hi;
            label_band(g, i, b, sample, lo, hi);
            for (uint64_t u = lo & ~uint64_t(15); u < hi; u += 16) label_boxes_unit(g, sample, lo, hi, u, mem, sink);
        }
    }
    return LLCOMP_MI_OK;
}

}  // extern "C"
