// label_boxes.cpp -- the host half of the label boxes of both calls (include/llcomp_mi.h: "Label boxes", "Label boxes of listed ids"):
// llcomp_mi_label_boxes_reference and llcomp_mi_label_boxes16_reference, which walk the kernels' own bands, threads and units
// (label_boxes_rule.hpp) on host memory, the listed call's table, and the accessors.  Plain C++, no GPU.
#include <cstring>

#include "label_boxes_rule.hpp"
#include "label_lists.hpp"

namespace llcomp_mi {
namespace {

// the dense call's finder: the id is the slot
struct PlainIdentity {
    uint32_t find(uint32_t id) const { return id; }
};
template <class Finder>
struct PlainSink {
    Finder finder;
    llcomp_mi_label_box* recs;  // of the sample
    void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        const uint32_t j = finder.find(id);
        if (j != kLabel16None) label_box_update(recs[j], x_first, x_end, y, length);
    }
};
// sample i of a checked call: its cnt records to their identities, then every band's workgroup, thread by thread
template <uint32_t MB, class Sink>
void label_boxes_sample(const LabelGeom& g, uint32_t i, uint32_t cnt, Sink& sink) {
    PlainMem mem;  // (batch_chunk.hpp: host memory as it is)
    for (uint32_t j = 0; j < cnt; ++j) sink.recs[j] = label_box_identity(g.ow, g.oh);
    for (uint32_t b = 0; b < g.bands; ++b) {
        uint64_t sample, lo, hi;
        label_band<MB>(g, i, b, sample, lo, hi);
        for (uint32_t t = 0; t < kLabelThreads; ++t) label_boxes_thread<MB>(g, sample, lo, hi, t, mem, sink);
    }
}

}  // namespace

template <class Id>
static void label_table_put(uint32_t n, const Id* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at) {
    const Label16Table tab(n, n_listed, first[n], sizeof(Id));
    std::memcpy(at + tab.first_at, first, 4 * (size_t(n) + 1));
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (first[i + 1] != first[i]) std::memcpy(at + tab.samples_at + 4 * size_t(k++), &i, 4);
    std::memcpy(at + tab.ids_at, ids, sizeof(Id) * size_t(first[n]));
}
void label16_table_put(uint32_t n, const uint16_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at) { label_table_put(n, ids, first, n_listed, at); }
void label32_table_put(uint32_t n, const uint32_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at) { label_table_put(n, ids, first, n_listed, at); }

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_label_boxes_rows(void) { return llcomp_mi::kLabelBoxRows; }
uint32_t llcomp_mi_label_boxes16_max_ids(void) { return llcomp_mi::kLabel16MaxIds; }

int llcomp_mi_label_boxes_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, llcomp_mi_label_box* out) {
    using namespace llcomp_mi;
    if (int rc = label_boxes_check_call(n, ow, oh)) return rc;
    if (!maps || !out) return LLCOMP_MI_BAD_ARGS;
    const LabelGeom g = label_geom<1>(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    for (uint32_t i = 0; i < n; ++i) {
        PlainSink<PlainIdentity> sink{{}, out + size_t(i) * kLabelIds};
        label_boxes_sample<1>(g, i, kLabelIds, sink);
    }
    return LLCOMP_MI_OK;
}

int llcomp_mi_label_boxes16_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids, const uint32_t* first,
                                      llcomp_mi_label_box* out) {
    using namespace llcomp_mi;
    if (int rc = label_boxes16_check_call(n, ow, oh, ids, first)) return rc;
    if (!maps || (reinterpret_cast<uintptr_t>(maps) & 1) || (!out && first[n])) return LLCOMP_MI_BAD_ARGS;
    const LabelGeom g = label_geom<2>(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t cnt = first[i + 1] - first[i];
        if (!cnt) continue;
        PlainSink<LabelFinder<const uint16_t*>> sink{{ids + first[i], cnt}, out + first[i]};
        label_boxes_sample<2>(g, i, cnt, sink);
    }
    return LLCOMP_MI_OK;
}

int llcomp_mi_label_boxes32_reference(const void* maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint32_t* ids, const uint32_t* first,
                                      llcomp_mi_label_box* out) {
    using namespace llcomp_mi;
    if (int rc = label_boxes32_check_call(map_bytes, n, ow, oh, ids, first)) return rc;
    const uint64_t m = reinterpret_cast<uintptr_t>(maps);
    if (!maps || label_map32_misaligned(m, map_bytes) || (!out && first[n])) return LLCOMP_MI_BAD_ARGS;
    const LabelGeom g = map_bytes == 3 ? label_geom<3>(m, n, ow, oh) : label_geom<4>(m, n, ow, oh);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t cnt = first[i + 1] - first[i];
        if (!cnt) continue;
        PlainSink<LabelFinder<const uint32_t*>> sink{label_finder32(ids + first[i], cnt), out + first[i]};
        if (map_bytes == 3) label_boxes_sample<3>(g, i, cnt, sink);
        else label_boxes_sample<4>(g, i, cnt, sink);
    }
    return LLCOMP_MI_OK;
}

}  // extern "C"
