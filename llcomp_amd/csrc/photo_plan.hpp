// photo_plan.hpp -- the host half of the photometric chains (include/llcomp_mi.h: llcomp_mi_codec_decode_photo_views /
// _photo_warped_views): the limits, which groups run chains, how their views are chunked through the staging buffer, what the ops of
// each step are (PhotoStepInfo: the step's launches), and the block of chains the call's one copy carries behind its tail's block.  Plain C++
// (photo_plan.cpp), like windows_plan.cpp: it builds and runs under a host sanitizer (tests/helpers/photo_plan_check.cpp).  The rule
// itself: photo_rule.hpp.  The driver: codec.hip, photo_tail_of (views_call, warped_call) and windows_photo behind every chunk of
// windows_groups; where the block sits in the copy: windows_plan.hpp, CopyLayout.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "resize_plan.hpp"

namespace llcomp_mi {

// What a view's statistics take in HBM: the sum of L as u64, then c histograms of 256 u32 ...
inline uint64_t photo_stats_stride(uint32_t c) { return 8 + 1024 * uint64_t(c); }
// ... and its table, [c][256] u8
inline uint64_t photo_lut_stride(uint32_t c) { return 256 * uint64_t(c); }

// The sharpness kernel's geometry (photo_kernels.hip: k_photo_sharp), which the planner charges for.  A workgroup owns a BAND of whole
// rows of a view and walks down it; the rows next to a band -- the last of the band above, the first of the band below -- are saved AS
// THEY STAND into a halo area behind the chunk's views before any band is written: two rows of ow * c bytes per pair of neighbouring bands.
constexpr uint32_t kSharpBandRows = 16;    // the rows of a band where the staging bound leaves room for the halos
constexpr uint32_t kSharpRowBytes = 12288; // the bytes of a row that the kernel's ring in LDS holds: a longer row is walked in column pieces ...
constexpr uint32_t kSharpKeepRows = 4096;  // ... whose edge columns stay behind in LDS for the band's rows, which caps a band of such a view
inline uint32_t photo_sharp_bands(uint32_t oh, uint32_t band_rows) { return (oh + band_rows - 1) / band_rows; }
inline uint64_t photo_sharp_halo_bytes(uint32_t ow, uint32_t oh, uint32_t c, uint32_t band_rows) {
    return 2 * uint64_t(photo_sharp_bands(oh, band_rows) - 1) * ow * c;
}
// The rows of a band for views of ow x oh x c whose chains hold the op, under the staging bound `samples`: kSharpBandRows, or as many
// more as it takes for one view with its halos to fit -- in the limit the whole view is one band with no halo, so that a view of
// `samples` bytes needs no byte beyond itself.  (The one exception: a view with rows longer than kSharpRowBytes AND more than
// kSharpKeepRows of them keeps bands of kSharpKeepRows, whatever they take.)
uint32_t photo_sharp_band_rows(uint32_t ow, uint32_t oh, uint32_t c, uint64_t samples);

// What the views of a group do at one step of their chains, which is what the step launches (photo.hpp): bit K of `kinds` -- some
// view's op of the step is of PhotoKind K (photo_rule.hpp); stats -- some view's op reads the view's statistics.
enum class PhotoKind : uint32_t;  // (photo_rule.hpp's, which this header leaves to the files of the rule: its pragma is theirs)
struct PhotoStepInfo {
    uint32_t kinds = 0;
    bool stats = false;
    bool has(PhotoKind k) const { return (kinds >> uint32_t(k)) & 1u; }
};
constexpr uint64_t kPhotoNoHalo = ~uint64_t(0);

// One group of the call.  active: some view has a chain that is not empty -- the group's tail entry then writes plain U8 HWC into the
// staging buffer, `chunk` views at a time, and the chain's last step writes d_out in format `out` through the table at table_at of the
// tail's output tables (all three taken over from the tail's group).  first: the group's chains in the block.  steps: the longest chain.
// step[k]: what the views' ops k are, k < steps.  sharp_rows: the rows of a band of the sharpness kernel, 0 for a group without the
// op; a chunk of such a group is `chunk` views and behind them `chunk` halo areas of photo_sharp_halo_bytes each, and the two together
// stay within the planner's bound.  halo_at: where in the staging buffer those areas begin -- behind the `chunk` views of a full
// chunk -- or kPhotoNoHalo for a group that saves no rows (no sharpness, or one band per view).
struct PhotoGroup {
    bool active = false;
    uint32_t n = 0, ow = 0, oh = 0, first = 0, chunk = 0, steps = 0, sharp_rows = 0;
    uint64_t halo_at = kPhotoNoHalo;
    PhotoStepInfo step[LLCOMP_MI_PHOTO_MAX_OPS];
    OutFormat out;
    void* d_out = nullptr;
    uint64_t table_at = 0;
};
// The chains' part of a call: the block -- llcomp_mi_photo_chain per view of every ACTIVE group, group by group -- and what the driver
// allocates: the staging buffer (the largest chunk's U8 HWC views) and the statistics and tables of the largest chunk's views.
struct PhotoTail {
    std::vector<llcomp_mi_photo_chain> chains;
    std::vector<PhotoGroup> groups;  // one per group of the call
    uint64_t stage_bytes = 0, tab_views = 0;
    bool any() const { return !chains.empty(); }
    uint64_t bytes() const { return uint64_t(chains.size()) * sizeof(llcomp_mi_photo_chain); }
    void put(uint8_t* at) const;
};
// What the chains add to a call's one copy at most: 16 bytes of alignment and one chain per view
uint64_t photo_tables_bound(uint64_t total_views);

// The limits of one chain on a codec of c channels: OK, or BAD_ARGS for more than LLCOMP_MI_PHOTO_MAX_OPS ops, an unknown op, a
// parameter outside its limits, and any op at all where c is neither 1 nor 3.
int photo_check_chain(const llcomp_mi_photo_chain& ch, uint32_t c);
// Everything of the chains the host decides.  photo: n_groups entries or null; n_views / ow / oh: per group of the call.  samples: the
// staging buffer's bound, frames * w * h * c -- a group of more views than fit is chunked, and one view always goes through.  A group
// whose chains hold the sharpness is chunked with every view charged its halo area too (photo_sharp_band_rows).
// BAD_ARGS: a struct_size that is not the struct's, and photo_check_chain's cases.
int photo_setup(uint32_t c, uint64_t samples, const llcomp_mi_photo_group* photo, uint32_t n_groups, const uint32_t* n_views, const uint32_t* ow,
                const uint32_t* oh, PhotoTail& t);

// The rule on a host image: src [h][w][c] -> out [h][w][c] (out may be src).
int photo_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_photo_op* ops, uint32_t n_ops, uint8_t* out);

}  // namespace llcomp_mi
