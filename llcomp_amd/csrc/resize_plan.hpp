// resize_plan.hpp -- the host half of the resampling of a resized regions or views decode (resize_plan.cpp): the weights, the entries the
// kernels read, the checked output format and its table.  No HIP header: the planner (windows_plan.hpp) and its host check build with a
// plain compiler.  The launchers: resize.hpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "geometry.hpp"

namespace llcomp_mi {

// One axis, in_len -> out_len, under filter LLCOMP_MI_FILTER_* (include/llcomp_mi.h: llcomp_mi_resize_filter_weights): the taps per
// output K (trailing taps that are zero for every output are left out), lo[out_len] and q[out_len][K] in Q22, zero-padded.  0 for
// in_len or out_len 0, an unknown filter, or a downscale above the filter's limit (geometry.hpp: resize_axis_ok).
uint32_t resize_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q);

// One entry of a resample launch, as the kernels see it: a frame of a resized regions decode, or a view of a views decode.  Its
// rectangle starts at (ox, oy) inside box `box` of d_box (every box bw x bh: the call's largest rectangle, or largest union of a frame's
// views) -- the frame's own box for a resized regions decode, the box of the view's frame for a views decode, where the views of one
// frame share a box.  The weights live in one int32 array: the horizontal pass's at hx -- lo[ow], then q tap-major [kx][ow] -- and the
// vertical pass's at vy -- lo[oh], then q [ky][oh].  Every lo is placed so that lo + k <= the rectangle's side (resize_weights' lo
// moved left over leading zero weights where needed): no tap reads outside the rectangle, so an entry's output does not depend on what
// else its box holds.
struct ResizeFrame {
    uint32_t ox, oy;  // the rectangle's origin inside the box
    uint32_t rw, rh;  // the rectangle
    uint32_t kx, ky;  // taps per output, horizontal / vertical
    uint32_t hx, vy;  // offsets of the weights, in int32 units
    uint32_t flags;   // bit 0: mirror the output horizontally; bits 4-6: the entry's filter (the kernels read bit 0 only)
    uint32_t box;     // which box of d_box holds the rectangle
    uint32_t pad[2];  // 0 but in a launch of the kernels' bias forms: [0] the entry's bias arrays (horizontal [ow], then vertical [oh]), [1] the
                      // call's c fill values, both offsets in the weights
};
static_assert(sizeof(ResizeFrame) == 48, "the kernels and the staging layout count on 48 bytes");
// Appends the weights of a rw x rh rectangle for ow x oh under `filter` to `w` and fills `e` (ox / oy / flags / box are the caller's).  An axis
// (filter, side -> output side) that an earlier frame of the call already put in `w` is shared: `seen` (empty at the start of a call)
// records them.  false for an unknown filter or a downscale above its limit.
bool resize_frame_weights(uint32_t filter, uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, ResizeFrame& e, std::vector<int32_t>& w,
                          std::vector<uint32_t>& seen);

// ---- rectangles that leave the image (include/llcomp_mi.h: llcomp_mi_pad, the padded calls) ----------------------------------------
// One axis of side n and the rectangle [x, x + r) under pad mode LLCOMP_MI_PAD_*: the source interval [s0, s0 + s_len) -- the set of the
// index map m(t) over the rectangle, inside the image.  false for an unknown mode, n or r 0, a rectangle with no image pixel, or a pad
// above the mode's limit (n - 1 for REFLECT, else n).
bool pad_axis(uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t& s0, uint32_t& s_len);
// ... and its folded rule for r -> out_len under `filter`: every tap of resize_weights(filter, r, out_len) that lands on a padded index t is
// added to the weight of source pixel m(t), or, for CONSTANT, to the output's bias.  lo[out] relative to s0, q[out][k] row-major, zero
// taps trimmed on both sides, lo placed so that lo + k <= s_len; bias[out] (all 0 but for CONSTANT); any_bias: some bias is not 0.
// A rectangle inside the image gives s0 = x and the unpadded weights as the kernels' tables place them.
struct PaddedAxis {
    uint32_t s0 = 0, s_len = 0, k = 0;
    std::vector<int32_t> lo, q, bias;
    bool any_bias = false;
};
bool padded_axis(uint32_t filter, uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t out_len, PaddedAxis& a);

// The axes a padded call has already put into its weights: the unpadded ones as resize_frame_weights records them, the padded ones under
// (filter, mode, n, x, r, out) with what an entry takes from them, and the bias pairs by the two axes they belong to.
struct PaddedSeen {
    struct Axis {
        uint32_t filter, mode, n, r, out;
        int32_t x;
        uint32_t k, at, s0, s_len, bias_at;  // bias_at: the axis's bias[out] in `bias` below
        bool any_bias;
    };
    struct Pair {
        uint32_t hx, vy, at;
    };
    std::vector<uint32_t> plain;
    std::vector<Axis> axes;
    std::vector<int32_t> bias;
    std::vector<Pair> pairs;
};
// resize_frame_weights for a signed rectangle rect = {x, y, rw, rh} of a w x h image under pad mode `mode`: fills e.rw / e.rh with the
// SOURCE rectangle's size, e.kx / ky / hx / vy with the folded weights, and src = {s0x, s0y, s_len_x, s_len_y}.  with_bias (CONSTANT
// with a fill other than 0): the entry's bias pair [ow][oh] is appended too (shared by entries with the same two axes) -> e.pad[0], and
// *biased says whether any of it is not 0.  false for what pad_axis or resize_axis_ok (on rw -> ow, rh -> oh) refuses.
bool padded_frame_weights(uint32_t filter, uint32_t mode, uint32_t w, uint32_t h, const int32_t* rect, uint32_t ow, uint32_t oh, bool with_bias,
                          ResizeFrame& e, uint32_t src[4], bool* biased, std::vector<int32_t>& wts, PaddedSeen& seen);

// The output format of an _ex call (include/llcomp_mi.h: llcomp_mi_output_format), checked: dtype, layout, element size, and whether the
// output is anything but today's u8 HWC (`plain`: no table, the two kernels of launch_resize).  BAD_ARGS for every case the header lists but the
// output pointer's alignment, which the caller checks against esize.  A NULL fmt is U8 HWC.
struct OutFormat {
    uint32_t dtype = 0, layout = 0, esize = 1;
    bool plain = true;
    uint64_t table_bytes(uint32_t c) const { return plain ? 0 : uint64_t(c) * 256 * esize; }
};
int check_output_format(const llcomp_mi_output_format* fmt, uint32_t c, OutFormat& o);
// The table of a checked format: table[ch * 256 + v], esize bytes each (include/llcomp_mi.h: the output rule).
void output_table(const llcomp_mi_output_format* fmt, uint32_t c, const OutFormat& o, uint8_t* table);

}  // namespace llcomp_mi
