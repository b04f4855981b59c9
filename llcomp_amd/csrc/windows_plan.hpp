// windows_plan.hpp -- everything the host decides for the windowed decodes of a batch (llcomp_mi_codec_decode_regions, _resized_regions,
// _views and their _host forms; DESIGN.md "Region decode"): every frame's window, class and box, the bytes the call's one copy carries
// and their bounds, and the resample entries, weights and output tables.  Plain C++ (windows_plan.cpp): functions of the codec's geometry
// and tuning hooks alone, so that what sizes the pinned slot and d_stage builds and runs under a host sanitizer
// (tests/helpers/windows_plan_check.cpp).  The driver that lays a plan into a slot by CopyLayout and queues it: codec.hip, decode_windows,
// which takes one WindowsCall from the four bodies behind the entry points (regions_call, resized_call, views_call, warped_call).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "container.hpp"
#include "geometry.hpp"
#include "resize_plan.hpp"

namespace llcomp_mi {

// One class of a regions decode: its sub-geometry, and its frames = entries [first, first + sub.frames) of the table.
struct RegionsClass {
    Geometry sub;
    uint32_t first;
};
// Every frame's window and class (geometry.hpp: regions_window) -> `tab` (g.frames entries, class by class, frame order inside a class)
// and the classes that have frames, in class order.  BAD_ARGS for a rectangle a frame does not hold; HIP_ERROR if a class's
// sub-geometry would not fit the codec's workspace (regions_fits: never by default, checked all the same).
int regions_setup(const Geometry& g, const Tuning& tune, const uint32_t* xy, uint32_t rw, uint32_t rh, RegionsFrame* tab, RegionsClass* classes,
                  uint32_t& n_classes);
// ... with a rectangle of its own size per frame (rects = {x, y, rw, rh} per frame): every window is sized for the largest, wmax x hmax
// (regions_window_sized), and the table's crop is a wmax x hmax BOX inside the window that contains the frame's rectangle, at
// min(the rectangle's origin, the window's side - wmax) -- the rectangle's own origin when all sizes are equal.
// used != nullptr (a views decode): a FRAME LIST -- only the n_used frames it names, in its order, get a table entry (`tab` holds n_used
// of them), rects is still indexed by frame, and entry i's box goes to output slot i, not to its frame's: a frame that is not listed
// has no entry, so none of its slices is touched.
int regions_setup_sized(const Geometry& g, const Tuning& tune, const uint32_t* rects, uint32_t wmax, uint32_t hmax, RegionsFrame* tab,
                        RegionsClass* classes, uint32_t& n_classes, const uint32_t* used = nullptr, uint32_t n_used = 0);

// What a host-staged regions decode copies to the GPU in one piece (pinned slot -> d_stage): the per-frame table, the window slices'
// lengths and payload offsets (in the order of the table: class by class, llcomp_mi_regions_gather), then their payload bytes.
struct StageLayout {
    uint64_t len_at, off_at, pay_at, bytes;
    StageLayout(uint32_t frames, uint64_t slices, uint64_t payload) {
        len_at = uint64_t(frames) * sizeof(RegionsFrame);
        off_at = (len_at + 4 * slices + 7) & ~7ull;
        pay_at = off_at + 8 * slices;
        bytes = pay_at + payload;
    }
};
// ... at most: every slice of the batch, each at the SLICED entry limit (the gather refuses a window entry above it)
uint64_t stage_bound(const Geometry& g);
// What a resized regions decode adds to the one copy at most, for outputs no larger than the image (ow <= w, oh <= h): 16 bytes of
// alignment, and per frame its ResizeFrame and its weights -- out * (K + 1) int32 per axis, K <= 2 * S * max(in / out, 1) + 3 with the
// filter's radius S <= 3 (Lanczos), so at most 6 * max(in, out) + 4 * out <= 10 * side of the image -- and the output format's table
// behind them (16 bytes of alignment, at most 256 * c elements of 4 bytes).
uint64_t resized_tables_bound(const Geometry& g);
// What the staged tables of a views decode add per view beyond `frames` (include/llcomp_mi.h: llcomp_mi_codec_views_workspace_bytes): its
// entry, its weights at resized_tables_bound's upper bound, and an output table with its alignment.
uint64_t view_term(const Geometry& g);
uint64_t views_tables_bound(const Geometry& g, uint64_t total_views);
// ... of the padded calls (include/llcomp_mi.h: llcomp_mi_codec_padded_workspace_bytes): a rectangle's side r reaches 3 * side, so an axis takes
// out * (K' + 1) of weights and `out` of bias, K' <= 6 * max(r / out, 1) + 3: at most 6 * max(r, out) + 5 * out <= 23 * side int32 for
// out <= side, where the unpadded bound has 10 * side; and c int32 of fill values per call.
uint64_t padded_term(const Geometry& g);  // what an entry adds to view_term / a frame to resized_tables_bound
uint64_t padded_tables_bound(const Geometry& g, uint64_t total_views);

// The windows of a call, as the driver takes them: the regions table, its classes, and the size every class crops per entry -- the
// rectangle itself for a plain regions decode, the box (the largest rectangle, or the largest union of a frame's views) otherwise.
struct WindowsPlan {
    std::vector<RegionsFrame> tab;
    RegionsClass classes[kRegionsClasses];
    uint32_t n_classes = 0, wmax = 0, hmax = 0;
};

// The resample block: what the one copy carries behind the regions table (or behind the staged payload), at a multiple of 16 --
// [ResizeFrame[entries]][int32 weights], then the output tables at the next multiple of 16, each table at a multiple of 16 of its own.
// A resized regions decode has one table, at 0 of the tables (none for the plain u8 HWC output); a views decode one per formatted group.
struct ResampleBlock {
    std::vector<ResizeFrame> rs;
    std::vector<int32_t> w;
    std::vector<uint8_t> tables;
    std::vector<uint8_t> biased;  // host only, a padded call with a constant fill other than 0: per entry, whether any of its bias is not 0
    uint64_t w_at() const { return uint64_t(rs.size()) * sizeof(ResizeFrame); }
    uint64_t tables_at() const { return (w_at() + 4 * uint64_t(w.size()) + 15) & ~15ull; }
    uint64_t bytes() const { return tables.empty() ? w_at() + 4 * uint64_t(w.size()) : tables_at() + tables.size(); }
    void put(uint8_t* at) const;
    // appends the table of the checked format `o` (nothing for a plain one); its offset in `tables`
    uint64_t add_table(const llcomp_mi_output_format* fmt, uint32_t c, const OutFormat& o);
};
// One output of the resample passes: entries [first, first + n) of the block to d_out [n][oh][ow][c] in format `out`, `chunk` entries
// per launch over rows of pitch mh (the group's largest rectangle height) in d_mid.
struct ResampleGroup {
    uint32_t n = 0, ow = 0, oh = 0, mh = 0, chunk = 0, first = 0;
    OutFormat out;
    void* d_out = nullptr;
    uint64_t table_at = 0;  // in the block's tables
};
// The tail of a resized or views decode: the classes crop every entry's box into d_box (box_bytes), then every group is resampled from
// the boxes through d_mid (mid_bytes: the largest chunk's rows).
struct ResampleTail {
    ResampleBlock block;
    std::vector<ResampleGroup> groups;
    uint64_t box_bytes = 0, mid_bytes = 0;
};

// Where everything sits in a call's one copy, in the pinned slot and in HBM alike: the table, the gather's arrays behind it for a host
// source (`stage`: the table alone without one); where the call has a tail, its block of block_bytes (ResampleBlock::bytes, or
// WarpTail::bytes -- warp_plan.hpp includes this header, so the layout takes the number) at rs_at, the next multiple of 16; and the
// chain_bytes of photometric chains (PhotoTail::bytes, 0 for a call without chains) at chains_at, the next multiple of 16 behind the
// block's end -- the slot's bytes [block_end, chains_at) are zeroed.  bytes: the whole copy.
struct CopyLayout {
    StageLayout stage;
    uint64_t rs_at, block_end, chains_at, bytes;
    CopyLayout(size_t entries, const RegionsGather* gather, bool tail, uint64_t block_bytes, uint64_t chain_bytes)
        : stage(uint32_t(entries), gather ? gather->n_slices : 0, gather ? gather->payload_bytes : 0),
          rs_at((stage.bytes + 15) & ~15ull),
          block_end(tail ? rs_at + block_bytes : stage.bytes),
          chains_at((block_end + 15) & ~15ull),
          bytes(chain_bytes ? chains_at + chain_bytes : block_end) {}
    // ... of a call with a resample tail or none, and no chains
    CopyLayout(size_t entries, const RegionsGather* gather, const ResampleTail* tail)
        : CopyLayout(entries, gather, tail != nullptr, tail ? tail->block.bytes() : 0, 0) {}
};

// Everything of a resized regions decode the host decides: every frame's window, class and box (regions_setup_sized, sized for the
// batch's largest rectangle wmax x hmax), its rectangle inside the box, its flags, its weights (resize_plan.hpp) and the output format's
// table.  One group of all frames in one chunk: d_mid is frames * hmax * ow * c bytes, also for outputs larger than the image.
// BAD_ARGS for a null rects, an output side of 0, any rectangle outside the image, a filter code above 5 in a frame's flags, a downscale
// above the frame's filter's limit on either axis (geometry.hpp: resize_axis_ok), a bad output format (check_output_format) and an
// output not aligned to the format's element size.
struct ResizedPlan : WindowsPlan {
    ResampleTail tail;  // block.rs in frame order
};
int resized_setup(const Geometry& g, const Tuning& tune, const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                  const llcomp_mi_output_format* fmt, void* d_out, ResizedPlan& p);

// Everything of a views decode the host decides (include/llcomp_mi.h: llcomp_mi_codec_decode_views): the union rectangle of every used
// frame (container.cpp: views_union), the regions table of the USED frames alone (regions_setup_sized with the frame list, sized for the
// largest union: entry i cuts its frame's box into d_box[i]), and per group its views' entries -- each names its frame's box and its
// rectangle inside it -- with the weights of the whole call in one array (an axis is shared across views AND groups) and the groups'
// output tables.  A group whose rows [n][mh][ow][c] (mh: ITS largest view height) would pass frames * w * h * c is resampled `chunk`
// views at a time, so d_mid keeps its bound for ow <= w (one view: mh * ow * c <= h * w * c).
// BAD_ARGS: views_union's cases, a bad output format, a group's d_out NULL or not aligned to its element size.
struct ViewsPlan : WindowsPlan {
    ViewsUnion u;
    ResampleTail tail;  // block.rs group by group, view order
};
int views_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_view_group* groups, uint32_t n_groups, ViewsPlan& p);

// The two plans for rectangles that may leave the image (include/llcomp_mi.h: llcomp_mi_pad): every rectangle's SOURCE rectangle first
// (resize_plan.hpp: pad_axis); then regions_setup_sized resp. views_union, unchanged, on the source rectangles -- the windows, classes,
// boxes and the gather are those of the unpadded call for them -- and a block whose entries describe the source rectangles with folded
// weights.  A CONSTANT pad with a fill other than 0 also puts every entry's bias pair and the call's fill values (c int32) into the
// weights and marks the entries with a bias in block.biased: the driver launches the kernels' bias forms for a chunk that has one.
// rects = {x, y, rw, rh} per frame, signed; a view's x / y are read as int32.  src: the source rectangles, 4 per frame (what the gather
// of a host source is planned over; a views plan has its unions in p.u).  BAD_ARGS: the unpadded plan's cases, a NULL pad, a
// struct_size below the struct's, a mode above 3, a size below 1, a pad above the mode's limit, a rectangle with no image pixel on an axis.
int check_pad(const llcomp_mi_pad* pad);
int padded_setup(const Geometry& g, const Tuning& tune, const int32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                 const llcomp_mi_pad* pad, const llcomp_mi_output_format* fmt, void* d_out, ResizedPlan& p, std::vector<uint32_t>& src);
int padded_views_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                       ViewsPlan& p);

}  // namespace llcomp_mi
