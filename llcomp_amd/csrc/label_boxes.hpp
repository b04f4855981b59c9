// label_boxes.hpp -- the launcher of the label boxes' kernels (label_boxes_kernels.hip; codec.hip: llcomp_mi_codec_label_boxes; DESIGN.md
// "Label boxes").  The rule: label_boxes_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace llcomp_mi {

// One call: k_label_boxes_init over the n * 256 records, then k_label_boxes, one workgroup per band and sample.  d_maps: n samples of
// oh x ow bytes at any address; d_boxes: n * 256 records of 20 bytes, 4-byte aligned.  Checked (label_boxes_check_call).
hipError_t launch_label_boxes(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, uint8_t* d_boxes, hipStream_t stream);

}  // namespace llcomp_mi
