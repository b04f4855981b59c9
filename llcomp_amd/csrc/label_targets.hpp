// label_targets.hpp -- the launcher of the kernel of the label targets (label_targets_kernels.hip; codec.hip:
// llcomp_mi_codec_label_targets; DESIGN.md "Label targets") and the writer of the call's table (label_targets.cpp).  The rule:
// label_targets_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "label_targets_rule.hpp"

namespace llcomp_mi {

// The call's table (TargetTable) at `at`: first[n + 1], the c.n_work samples that get workgroups, plane_first[n + 1] for PLANES, the
// values, the ids.  A checked call (label_targets_check_call, which gave c).
void target_table_put(uint32_t n, const llcomp_mi_label_targets& t, const TargetCall& c, uint8_t* at);

// One call: k_label_targets<MB, K, KIND>, a workgroup per segment, sample that gets workgroups and plane chunk, K the smallest
// capacity that holds c.longest ids.  d_maps: n samples of oh x ow pixels of t.map_bytes, aligned to them; d_table: the table above in
// device memory, 4-byte aligned; d_out: c.out_bytes bytes aligned to c.esize, not overlapping the maps.  A checked call with
// c.n_work > 0.
hipError_t launch_label_targets(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets& t, const TargetCall& c,
                                const uint8_t* d_table, uint8_t* d_out, hipStream_t stream);

// The same for maps of t.map_bytes 3 or 4 (k_label_targets32<MB, K, KIND>; llcomp_mi_codec_label_targets32): the table's ids are
// uint32_t.  d_maps: at any address for map_bytes 3, 4-byte aligned for 4.
void target32_table_put(uint32_t n, const llcomp_mi_label_targets32& t, const TargetCall& c, uint8_t* at);
hipError_t launch_label_targets32(const uint8_t* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32& t, const TargetCall& c,
                                  const uint8_t* d_table, uint8_t* d_out, hipStream_t stream);

}  // namespace llcomp_mi
