// label_targets.cpp -- the host half of the label targets (include/llcomp_mi.h: "Label targets", "Wide id maps"):
// llcomp_mi_label_targets_reference and llcomp_mi_label_targets32_reference, which walk the kernel's own workgroups, threads and units
// (label_targets_rule.hpp) on host memory, the call's table, and the accessors.  Plain C++, no GPU.
#include <cstring>
#include <vector>

#include "label_targets_rule.hpp"

namespace llcomp_mi {
namespace {

template <class T>
void table_put(uint32_t n, const T& t, const TargetCall& c, uint8_t* at) {
    constexpr size_t kIdBytes = sizeof(*t.ids);
    const bool planes = t.kind == LLCOMP_MI_TARGET_PLANES;
    const TargetTable tab(n, c.n_work, c.total, planes, kIdBytes);
    std::memcpy(at + tab.first_at, t.first, 4 * (size_t(n) + 1));
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (!planes || t.plane_first[i + 1] != t.plane_first[i]) std::memcpy(at + tab.samples_at + 4 * size_t(k++), &i, 4);
    if (planes) std::memcpy(at + tab.planes_at, t.plane_first, 4 * (size_t(n) + 1));
    if (c.total) {
        std::memcpy(at + tab.values_at, t.values, 4 * size_t(c.total));
        std::memcpy(at + tab.ids_at, t.ids, kIdBytes * size_t(c.total));
    }
}

// the reference of either struct: Id is its ids' type
template <class Id, class T>
int reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const T* targets, void* out) {
    TargetCall c;
    if (int rc = label_targets_check_any(n, ow, oh, targets, c)) return rc;
    const T& t = *targets;
    const uintptr_t m = reinterpret_cast<uintptr_t>(maps), o = reinterpret_cast<uintptr_t>(out);
    const uint32_t map_align = t.map_bytes == 3 ? 1u : t.map_bytes;
    if (!maps || !out || (m & (map_align - 1)) || (o & (c.esize - 1))) return LLCOMP_MI_BAD_ARGS;
    const TargetGeom g = target_geom(m, o, n, ow, oh, t.map_bytes);
    const TargetParams a{t.kind, c.esize, t.default_value, t.on_bits, t.off_bits};
    const uint32_t K = t.map_bytes == 1 ? 256u : label16_capacity(c.longest), chunks = target_plane_chunks(t.kind, c.most_planes);
    std::vector<Id> list(K);
    std::vector<uint32_t> vals(K), v(kTargetSegment);
    PlainMem mem;  // (batch_chunk.hpp: host memory as it is, for the maps and for the output)
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t seg = 0; seg < g.segments; ++seg)
            for (uint32_t z = 0; z < chunks; ++z)
                label_targets_host_workgroup(g, a, t.map_bytes, t.first, t.plane_first, t.values, t.ids, i, seg, z, mem, mem, list, vals, v);
    return LLCOMP_MI_OK;
}

}  // namespace

void target_table_put(uint32_t n, const llcomp_mi_label_targets& t, const TargetCall& c, uint8_t* at) { table_put(n, t, c, at); }
void target32_table_put(uint32_t n, const llcomp_mi_label_targets32& t, const TargetCall& c, uint8_t* at) { table_put(n, t, c, at); }

}  // namespace llcomp_mi

extern "C" {

uint32_t llcomp_mi_label_targets_segment(void) { return llcomp_mi::kTargetSegment; }
uint32_t llcomp_mi_label_targets_max_planes(void) { return llcomp_mi::kTargetMaxPlanes; }

uint64_t llcomp_mi_label_targets_out_bytes(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* targets) {
    llcomp_mi::TargetCall c;
    return llcomp_mi::label_targets_check_call(n, ow, oh, targets, c) == LLCOMP_MI_OK ? c.out_bytes : 0;
}
uint64_t llcomp_mi_label_targets32_out_bytes(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* targets) {
    llcomp_mi::TargetCall c;
    return llcomp_mi::label_targets32_check_call(n, ow, oh, targets, c) == LLCOMP_MI_OK ? c.out_bytes : 0;
}

int llcomp_mi_label_targets_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* targets, void* out) {
    return llcomp_mi::reference<uint16_t>(maps, n, ow, oh, targets, out);
}
int llcomp_mi_label_targets32_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* targets, void* out) {
    return llcomp_mi::reference<uint32_t>(maps, n, ow, oh, targets, out);
}

}  // extern "C"
