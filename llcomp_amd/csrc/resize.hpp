// resize.hpp -- the resampling of a resized regions decode (resize_kernels.hip; codec.hip: llcomp_mi_codec_decode_resized_regions;
// DESIGN.md "Crops of different sizes, resized to one shape").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"

namespace llcomp_mi {

// One axis, in_len -> out_len, under filter LLCOMP_MI_FILTER_* (include/llcomp_mi.h: llcomp_mi_resize_filter_weights): the taps per
// output K (trailing taps that are zero for every output are left out), lo[out_len] and q[out_len][K] in Q22, zero-padded.  0 for
// in_len or out_len 0, an unknown filter, or a downscale above the filter's limit (resize_axis_ok): R * in_len > kResizeMaxDown * out_len
// with R = 1, but 2 for bicubic and 3 for Lanczos, so that the filter's support never passes kResizeMaxDown input samples and K <= 129.
constexpr uint32_t kResizeMaxDown = 64;
constexpr uint32_t kResizeFilters = 6;
bool resize_axis_ok(uint32_t filter, uint32_t in_len, uint32_t out_len);
uint32_t resize_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q);

// One frame of a resized regions decode, as the kernels see it.  The frame's box (the batch's largest rectangle size, bw x bh) is
// d_box[f]; its rectangle starts at (ox, oy) inside it.  The weights live in one int32 array: the horizontal pass's at hx -- lo[ow],
// then q tap-major [kx][ow] -- and the vertical pass's at vy -- lo[oh], then q [ky][oh].  Every lo is placed so that lo + k <= the
// rectangle's side (resize_weights' lo moved left over leading zero weights where needed): no tap reads outside the rectangle.
struct ResizeFrame {
    uint32_t ox, oy;  // the rectangle's origin inside the box
    uint32_t rw, rh;  // the rectangle
    uint32_t kx, ky;  // taps per output, horizontal / vertical
    uint32_t hx, vy;  // offsets of the weights, in int32 units
    uint32_t flags;   // bit 0: mirror the output horizontally; bits 4-6: the frame's filter (the kernels read bit 0 only)
    uint32_t pad[3];
};
static_assert(sizeof(ResizeFrame) == 48, "the kernels and the staging layout count on 48 bytes");
// Appends the weights of a rw x rh rectangle for ow x oh under `filter` to `w` and fills `e` (ox / oy / flags are the caller's).  An axis
// (filter, side -> output side) that an earlier frame of the call already put in `w` is shared: `seen` (empty at the start of a call)
// records them.  false for an unknown filter or a downscale above its limit.
bool resize_frame_weights(uint32_t filter, uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, ResizeFrame& e, std::vector<int32_t>& w,
                          std::vector<uint32_t>& seen);

// d_box [frames][bh][bw][c] -> d_mid [frames][bh][ow][c] (rows [0, rh) of every frame: the horizontal pass, rounded to u8) -> d_px
// [frames][oh][ow][c] (the vertical pass, then the mirror).  The caller guarantees ox + rw <= bw, oy + rh <= bh for every entry.
hipError_t launch_resize(const uint8_t* d_box, uint8_t* d_mid, uint8_t* d_px, const ResizeFrame* d_tab, const int32_t* d_w, uint32_t frames,
                         uint32_t c, uint32_t bw, uint32_t bh, uint32_t ow, uint32_t oh, hipStream_t stream);

// The output format of an _ex call (include/llcomp_mi.h: llcomp_mi_output_format), checked: dtype, layout, element size, and whether the
// output is anything but today's u8 HWC (`plain`: no table, the two kernels above).  BAD_ARGS for every case the header lists but the
// output pointer's alignment, which the caller checks against esize.  A NULL fmt is U8 HWC.
struct OutFormat {
    uint32_t dtype = 0, layout = 0, esize = 1;
    bool plain = true;
    uint64_t table_bytes(uint32_t c) const { return plain ? 0 : uint64_t(c) * 256 * esize; }
};
int check_output_format(const llcomp_mi_output_format* fmt, uint32_t c, OutFormat& o);
// The table of a checked format: table[ch * 256 + v], esize bytes each (include/llcomp_mi.h: the output rule).
void output_table(const llcomp_mi_output_format* fmt, uint32_t c, const OutFormat& o, uint8_t* table);

// launch_resize with the vertical pass writing fmt's table entries in its layout (o.plain is launch_resize itself): d_table is the
// table of output_table in device memory, 4-byte aligned; d_out is aligned to o.esize.
hipError_t launch_resize_out(const uint8_t* d_box, uint8_t* d_mid, void* d_out, const ResizeFrame* d_tab, const int32_t* d_w, const void* d_table,
                             const OutFormat& o, uint32_t frames, uint32_t c, uint32_t bw, uint32_t bh, uint32_t ow, uint32_t oh,
                             hipStream_t stream);

}  // namespace llcomp_mi
