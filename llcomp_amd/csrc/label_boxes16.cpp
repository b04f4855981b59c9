// label_boxes16.cpp -- the host half of the label boxes of listed ids (include/llcomp_mi.h: "Label boxes of listed ids"):
// llcomp_mi_label_boxes16_reference, which walks the kernel's own bands and units (label_boxes16_rule.hpp) on host memory, the call's
// table, and the accessor of the longest list.  Plain C++, no GPU.
#include <cstring>

#include "label_boxes16_rule.hpp"

namespace llcomp_mi {
namespace {

struct PlainMem16 {
    LabelChunk load16(uint64_t a) const {
        LabelChunk v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), 16);  // (little-endian hosts, like the containers)
        return v;
    }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) const {
        uint16_t v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), 2);
        return v;
    }
};
struct PlainSink16 {
    LabelFinder<const uint16_t*> finder;
    llcomp_mi_label_box* recs;  // of the sample's list
    void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        const uint32_t j = finder.find(id);
        if (j != kLabel16None) label_box_update(recs[j], x_first, x_end, y, length);
    }
};

}  // namespace

void label16_table_put(uint32_t n, const uint16_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at) {
    const Label16Table tab(n, n_listed, first[n]);
    std::memcpy(at + tab.first_at, first, 4 * (size_t(n) + 1));
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (first[i + 1] != first[i]) std::memcpy(at + tab.samples_at + 4 * size_t(k++), &i, 4);
    std::memcpy(at + tab.ids_at, ids, 2 * size_t(first[n]));
}

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_label_boxes16_max_ids(void) { return llcomp_mi::kLabel16MaxIds; }

int llcomp_mi_label_boxes16_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids, const uint32_t* first,
                                      llcomp_mi_label_box* out) {
    using namespace llcomp_mi;
    if (int rc = label_boxes16_check_call(n, ow, oh, ids, first)) return rc;
    if (!maps || (reinterpret_cast<uintptr_t>(maps) & 1) || (!out && first[n])) return LLCOMP_MI_BAD_ARGS;
    const LabelGeom16 g = label_geom16(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    PlainMem16 mem;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t cnt = first[i + 1] - first[i];
        if (!cnt) continue;
        PlainSink16 sink{{ids + first[i], cnt}, out + first[i]};
        for (uint32_t j = 0; j < cnt; ++j) sink.recs[j] = label_box_identity(ow, oh);
        for (uint32_t b = 0; b < g.bands; ++b) {
            uint64_t sample, lo, hi;
            label_band16(g, i, b, sample, lo, hi);
            for (uint32_t t = 0; t < kLabel16Threads; ++t) label_boxes16_thread(g, sample, lo, hi, t, mem, sink);
        }
    }
    return LLCOMP_MI_OK;
}

}  // extern "C"
