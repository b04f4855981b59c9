// label_lists.hpp -- the sorted id lists of a call, one per sample (include/llcomp_mi.h: "Label boxes of listed ids", "Label
// targets"): the check of a call's lists, the capacities a call runs at, the table the lists travel in, and the search of an id in a
// sample's list, for lists of uint16_t ids and, for the wide id maps (map_bytes 3 and 4), of uint32_t ids.  What the label boxes of
// listed ids (label_boxes_kernels.hip, label_boxes.cpp) and the label targets (label_targets_rule.hpp) share beside the unit rule
// (label_boxes_rule.hpp, batch_chunk.hpp).
#pragma once
#include <cstdint>

#include "../../include/llcomp_mi.h"
#include "batch_ops.hpp"

namespace llcomp_mi {

constexpr uint32_t kLabel16MaxIds = 4096;          // listed ids of a sample (llcomp_mi_label_boxes16_max_ids): 22 bytes of LDS per id
constexpr uint32_t kLabel16MaxTotal = 1u << 20;    // listed ids of a call
constexpr uint32_t kLabel16IdBytes = 2 + 5 * 4;    // of LDS per listed id: the id and the record's five words
constexpr uint32_t kLabel16None = 0xFFFFFFFFu;     // label_list_find: the id is not listed
constexpr uint32_t kLabel16Capacities[3] = {256, 1024, 4096};

// The capacity a call of lists of at most `longest` ids runs at
inline uint32_t label16_capacity(uint32_t longest) {
    return longest <= kLabel16Capacities[0] ? kLabel16Capacities[0] : longest <= kLabel16Capacities[1] ? kLabel16Capacities[1] : kLabel16Capacities[2];
}

constexpr uint32_t kLabel32IdBytes = 4 + 5 * 4;    // of LDS per listed id of the wide calls: a 4-byte id and the record's five words

// A whole call but for its device pointers, the ids of type Id and at most top_id, the shape checked with a pixel of the size of
// `dtype`'s element.  *longest: the longest list; *n_listed: the samples with a list that is not empty.
template <class Id>
inline int label_lists_check_call(uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype, const Id* ids, const uint32_t* first, uint32_t top_id, uint32_t* longest,
                                  uint32_t* n_listed) {
    if (int rc = batch_check_shape(n, 1, ow, oh, dtype, LLCOMP_MI_LAYOUT_HWC)) return rc;
    if (uint64_t(ow) * oh >= (1ull << 32) || !ids || !first || first[0] != 0) return LLCOMP_MI_BAD_ARGS;
    uint32_t most = 0, listed = 0;
    for (uint32_t i = 0; i < n; ++i) {  // (the bounds first: no id is read before first says where the ids end)
        if (first[i + 1] < first[i] || first[i + 1] > kLabel16MaxTotal) return LLCOMP_MI_BAD_ARGS;
        const uint32_t cnt = first[i + 1] - first[i];
        if (cnt > kLabel16MaxIds) return LLCOMP_MI_BAD_ARGS;
        most = cnt > most ? cnt : most, listed += cnt != 0;
    }
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t j = first[i] + 1; j < first[i + 1]; ++j)
            if (ids[j] <= ids[j - 1]) return LLCOMP_MI_BAD_ARGS;
        if (first[i + 1] != first[i] && ids[first[i + 1] - 1] > top_id) return LLCOMP_MI_BAD_ARGS;  // (ascending: the last id is the largest)
    }
    if (longest) *longest = most;
    if (n_listed) *n_listed = listed;
    return LLCOMP_MI_OK;
}
inline int label_boxes16_check_call(uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids, const uint32_t* first, uint32_t* longest = nullptr,
                                    uint32_t* n_listed = nullptr) {
    return label_lists_check_call(n, ow, oh, LLCOMP_MI_DTYPE_F16, ids, first, 0xFFFFu, longest, n_listed);  // (a 2-byte element)
}
// The wide calls' (map_bytes 3 or 4, uint32_t ids): a map_bytes that is neither and an id above 0xFFFFFF in a 3-byte map are refused too
inline int label_boxes32_check_call(uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint32_t* ids, const uint32_t* first,
                                    uint32_t* longest = nullptr, uint32_t* n_listed = nullptr) {
    if (map_bytes != 3 && map_bytes != 4) return LLCOMP_MI_BAD_ARGS;
    return label_lists_check_call(n, ow, oh, LLCOMP_MI_DTYPE_F32, ids, first, map_bytes == 3 ? 0xFFFFFFu : 0xFFFFFFFFu, longest, n_listed);  // (at most 4 bytes)
}
// a wide map at m: a 4-byte one is aligned to 4, a 3-byte one lies anywhere
inline bool label_map32_misaligned(uint64_t m, uint32_t map_bytes) { return map_bytes == 4 && (m & 3) != 0; }

// The table of a call in device memory: first[n + 1], then the n_listed samples that get workgroups, ascending, then the ids, of
// id_bytes each
struct Label16Table {
    uint64_t first_at, samples_at, ids_at, bytes;
    Label16Table(uint64_t n, uint64_t n_listed, uint64_t total, uint64_t id_bytes = 2)
        : first_at(0), samples_at(4 * (n + 1)), ids_at(samples_at + 4 * n_listed), bytes(ids_at + id_bytes * total) {}
};
inline uint64_t label16_table_bound(uint64_t n, uint64_t total_ids) { return Label16Table(n, n, total_ids).bytes; }
inline uint64_t label32_table_bound(uint64_t n, uint64_t total_ids) { return Label16Table(n, n, total_ids, 4).bytes; }

// id in the strictly ascending list[0 .. count): its index, or kLabel16None
template <class List>
LLMI_HD inline uint32_t label_list_find(const List& list, uint32_t count, uint32_t id) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uint32_t(list[mid]) < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < count && uint32_t(list[lo]) == id ? lo : kLabel16None;
}
// ... behind a comparison with the id of the thread's previous run, which neighbouring units mostly repeat
template <class List>
struct LabelFinder {
    List list;
    uint32_t count;
    uint32_t prev_id = kLabel16None, prev_slot = kLabel16None;  // (no 1- or 2-byte id is 0xFFFFFFFF; the wide calls: label_finder32)
    LLMI_HD inline uint32_t find(uint32_t id) {
        if (id != prev_id) prev_id = id, prev_slot = label_list_find(list, count, id);
        return prev_slot;
    }
};
// ... of a list of 4-byte ids, where 0xFFFFFFFF IS an id: the finder starts as if its previous run had been of that id -- listed
// exactly when it is the last of the ascending list
template <class List>
LLMI_HD inline LabelFinder<List> label_finder32(List list, uint32_t count) {
    return LabelFinder<List>{list, count, kLabel16None, count && uint32_t(list[count - 1]) == kLabel16None ? count - 1 : kLabel16None};
}

}  // namespace llcomp_mi
