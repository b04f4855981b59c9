// label_boxes.hpp -- the launchers of the label boxes' kernels (label_boxes_kernels.hip; codec.hip: llcomp_mi_codec_label_boxes and
// llcomp_mi_codec_label_boxes16; DESIGN.md "Label boxes", "Label boxes of listed ids") and the writer of the listed call's table
// (label_boxes.cpp).  The rule: label_boxes_rule.hpp; the lists: label_lists.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace llcomp_mi {

// One call: k_label_boxes_init over the n * 256 records, then k_label_boxes, one workgroup per band and sample.  d_maps: n samples of
// oh x ow bytes at any address; d_boxes: n * 256 records of 20 bytes, 4-byte aligned.  Checked (label_boxes_check_call).
hipError_t launch_label_boxes(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, uint8_t* d_boxes, hipStream_t stream);

// The listed call's table (Label16Table) at `at`: first[n + 1], the n_listed samples with a list, the ids.  Checked lists.
void label16_table_put(uint32_t n, const uint16_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at);

// One call: k_label_boxes_init over the `total` = first[n] records, then k_label_boxes16<K>, one workgroup per band and listed
// sample, K the smallest capacity that holds `longest` ids.  d_maps: n samples of oh x ow uint16_t, 2-byte aligned; d_table: the table
// above in device memory, 4-byte aligned; d_boxes: `total` records of 20 bytes, 4-byte aligned.  Checked (label_boxes16_check_call).
hipError_t launch_label_boxes16(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const uint8_t* d_table, uint32_t n_listed, uint32_t total,
                                uint32_t longest, uint8_t* d_boxes, hipStream_t stream);

// The same of maps of map_bytes 3 or 4 (k_label_boxes32<MB, K>; llcomp_mi_codec_label_boxes32): the table's ids are uint32_t.  d_maps:
// at any address for map_bytes 3, 4-byte aligned for 4.  Checked (label_boxes32_check_call).
void label32_table_put(uint32_t n, const uint32_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at);
hipError_t launch_label_boxes32(const uint8_t* d_maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint8_t* d_table, uint32_t n_listed,
                                uint32_t total, uint32_t longest, uint8_t* d_boxes, hipStream_t stream);

}  // namespace llcomp_mi
