// warp_plan.hpp -- the host half of the warped views (include/llcomp_mi.h: llcomp_mi_codec_decode_warped_views): the limits, a view's
// source rectangle, the unions and windows -- those of a views decode on the source rectangles, through views_union and
// regions_setup_sized unchanged -- and what the gather kernel reads: one entry per view, the pure-scale index tables, the groups' fill
// values and output tables.  Plain C++ (warp_plan.cpp), like windows_plan.cpp: it builds and runs under a host sanitizer
// (tests/helpers/warp_plan_check.cpp).  The rule itself: warp_rule.hpp.  The driver: codec.hip, warped_call -> decode_windows with a warp
// tail -> windows_warp.  The perspective views (llcomp_mi_codec_decode_perspective_views) are planned here too: the same unions, windows
// and tail around a source rectangle that is a bound (persp_source_rect) and an entry type of their own (PerspEntry).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "windows_plan.hpp"

namespace llcomp_mi {

// One view as the kernel sees it.  form (flags bits 8-9): kWarpSmooth -- m is the matrix; kWarpFixed -- a holds PIL's six 16.16 integers;
// kWarpTable -- t = {offset of xi[ow], offset of yi[oh]} in the block's int32 tables; kWarpEmpty -- no pixel inside, all fill, no box.
// (bx, by): the origin of box `box` in its frame, so frame pixel (col, row) is box pixel (col - bx, row - by).
struct WarpEntry {
    union {
        double m[6];
        int32_t a[6];
        uint32_t t[2];
    };
    int32_t bx, by;
    uint32_t box;
    uint32_t flags;  // bit 0: mirror the output horizontally; bits 4-6: the filter; bits 8-9: the form
};
static_assert(sizeof(WarpEntry) == 64, "the kernel and the staging layout count on 64 bytes");
constexpr uint32_t kWarpFormShift = 8;
// One PERSPECTIVE view as the kernel sees it: the eight coefficients do not fit WarpEntry, so a perspective call stages entries of its
// own kind and the affine calls' bytes stay what they were.  flags bit 0: mirror; bits 4-6: the filter; bit 8: empty -- no pixel inside,
// all fill, no box.  (bx, by), box: as in WarpEntry.
struct PerspEntry {
    double a[8];
    int32_t bx, by;
    uint32_t box;
    uint32_t flags;
};
static_assert(sizeof(PerspEntry) == 80, "the kernel and the staging layout count on 80 bytes");
constexpr uint32_t kPerspEmpty = 1u << 8;

// One output of the gather kernel: entries [first, first + n) -> d_out [n][oh][ow][c] in format `out`
struct WarpOut {
    uint32_t n = 0, ow = 0, oh = 0, first = 0;
    OutFormat out;
    void* d_out = nullptr;
    uint64_t table_at = 0;  // in the block's output tables
    uint32_t fill_at = 0;   // the group's c fill bytes in the block's fills
};
// The third kind of tail of decode_windows: the classes crop every used frame's box into d_box, then ONE launch per group gathers its
// views from the boxes.  The block the one copy carries, at a multiple of 16: [WarpEntry[views]][int32 index tables][fill bytes, c per
// group], then the output tables at the next multiple of 16, each at a multiple of 16 of its own.
// A perspective call has PerspEntry[views] (ps) in place of the WarpEntry (ws stays empty, and there are no index tables).
struct WarpTail {
    std::vector<WarpEntry> ws;
    std::vector<PerspEntry> ps;
    std::vector<int32_t> tabs;
    std::vector<uint8_t> fills, tables;
    std::vector<WarpOut> groups;
    uint64_t box_bytes = 0;
    uint64_t tabs_at() const { return uint64_t(ws.size()) * sizeof(WarpEntry) + uint64_t(ps.size()) * sizeof(PerspEntry); }
    uint64_t fills_at() const { return tabs_at() + 4 * uint64_t(tabs.size()); }
    uint64_t tables_at() const { return (fills_at() + fills.size() + 15) & ~15ull; }
    uint64_t bytes() const { return tables.empty() ? fills_at() + fills.size() : tables_at() + tables.size(); }
    void put(uint8_t* at) const;
};
// What the block takes at most for outputs no larger than the image, per view: its entry, two index tables (ow + oh <= w + h int32), and
// -- every view may be a group of its own -- c fill bytes, an output table and the alignment of both.
uint64_t warp_view_term(const Geometry& g);
uint64_t warp_tables_bound(const Geometry& g, uint64_t total_views);
// ... and for a perspective call: the entry is 16 bytes longer
uint64_t persp_tables_bound(const Geometry& g, uint64_t total_views);

// The limits of the header: OK, or BAD_ARGS for a coefficient that is not finite, a filter other than NEAREST, BILINEAR and BICUBIC, an
// output side of 0, or coordinates beyond what the rule reproduces.
int warp_check(const double* m, uint32_t filter, uint32_t ow, uint32_t oh);
// The rectangle {x, y, rw, rh} of image pixels the view reads -- exactly the bounding box of the rule's taps over the output pixels that
// lie inside the image -- or empty = true (rect zeroed) when no output pixel does.  Every row's inside pixels are an interval (the
// coordinates are monotone in x and in y under the rule's rounding), found by bisection; the taps' extremes sit at its two ends.
int warp_source_rect(uint32_t w, uint32_t h, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4], bool& empty);
// The rule on a host image: src [h][w][c] -> out [oh][ow][c]; fill = c bytes or null for zeros.
int warp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, const uint8_t* fill, uint32_t ow,
                   uint32_t oh, uint8_t* out);

// Everything of a warped views decode the host decides.  Every view's source rectangle; views_union over them (one rectangle per view
// that has one) and regions_setup_sized with the frame list: p.tab, p.classes, p.wmax x p.hmax exactly as views_setup gives them for
// those rectangles; no used frame at all -- every view empty -- leaves the table empty and the call decodes nothing.
struct WarpPlan : WindowsPlan {
    ViewsUnion u;  // u.total_views counts the views that read pixels
    WarpTail tail;
    uint64_t total_views = 0;
};
// every check on the groups and their views, and the unions (the part llcomp_mi_warp_views_plan shares with the decode); rects: per view
// of the call, in order, {x, y, rw, rh, empty}
int warp_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_warp_group* groups, uint32_t n_groups, ViewsUnion& u,
               std::vector<uint32_t>& rects, uint64_t& total_views);
int warp_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_warp_group* groups, uint32_t n_groups, WarpPlan& p);

// Perspective views (include/llcomp_mi.h: "Views under a projective map").  The limits: OK, or BAD_ARGS for a coefficient that is not
// finite, a filter other than the three, an output side of 0, a denominator that is not > 0 at one of the four corner pixels, or a
// coordinate of a corner pixel not below 2^30.
int persp_check(const double* a, uint32_t filter, uint32_t ow, uint32_t oh);
// A rectangle that CONTAINS every tap of every output pixel inside the image, at most a pixel beyond the taps of the first and the last
// inside pixel of every output row; empty exactly when no output pixel is inside (persp_rect in warp_plan.cpp says why).
int persp_source_rect(uint32_t w, uint32_t h, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4], bool& empty);
int persp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* a, uint32_t filter, const uint8_t* fill, uint32_t ow,
                    uint32_t oh, uint8_t* out);
// warp_union and warp_setup for perspective groups: the same plan on the views' source rectangles, PerspEntry in the tail
int persp_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_perspective_group* groups, uint32_t n_groups, ViewsUnion& u,
                std::vector<uint32_t>& rects, uint64_t& total_views);
int persp_setup(const Geometry& g, const Tuning& tune, const llcomp_mi_perspective_group* groups, uint32_t n_groups, WarpPlan& p);

}  // namespace llcomp_mi
