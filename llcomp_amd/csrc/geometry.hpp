// geometry.hpp -- slice geometry shared by host and device code.
//
// A "slice" is the unit the serial entropy coder runs over: a tile_w x tile_h rectangle of one frame, either
// with all channels interleaved in one stream (planar == 0; payload == reference stream of the cropped
// sub-image, llcomp.hpp:390-449) or one colour-transformed channel plane of it (planar == 1).  Slices have
// fresh adaptive state and slice-local border rules, so they are independent: one GPU lane each.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#if defined(__HIPCC__)
#define LLMI_HD __host__ __device__
#else
#define LLMI_HD
#endif

namespace llcomp_mi {

constexpr uint32_t kMaxChannels = 255;  // one byte in both headers; 1..4 run the specialised kernels, more the generic ones

struct Geometry {
    uint32_t frames, w, h, c;
    uint32_t tile_w, tile_h, planar;
    uint32_t ntx, nty;          // tiles per row / column of one frame
    uint32_t slices_per_frame;  // ntx*nty*(planar ? c : 1)
    uint32_t n_slices;          // frames * slices_per_frame
    uint32_t slice_cap;         // scratch bytes reserved per slice (worst case, multiple of 16)
    uint32_t nch;               // channels coded inside one slice: planar ? 1 : c
    uint32_t lane_shift;        // log2 of the lane-group width (64 lanes, fewer when there are fewer slices)
    uint32_t slice_samples;     // sample capacity of one slice: tile_w * tile_h * nch
    uint32_t lpw;               // slices per wavefront = active lanes (a power of two <= the group width)
    uint32_t flags;             // kernel family, fixed when the codec object is created (kGeo* below)
};
enum : uint32_t {
    kGeoRows = 1u,         // 1-row slices: the three reachable contexts' states live in LDS
    kGeoLdsTable = 2u,     // one slice per wavefront: its 63 KB state table lives in LDS
    kGeoForceReplay = 4u,  // test hook: every decoded sample also goes through rollback + checked replay
    kGeoSmallModel = 8u,   // bitstream variant: the reference built with LargeModel = false (llcomp.hpp:21, 26-32, 427-429)
    kGeoSnapshot = 16u,    // 2-D slices of at most kSnapMaxSamples * kSnapMaxChunks samples: the ENCODER streams state snapshots
                           // (snapshot_kernels.hip) instead of read-modify-writing a 63 KB table per slice in HBM per SAMPLE; the decoder
                           // still needs that table, and so does the pass itself between the chunks of a slice above 4096 samples
    kGeoBankCache = 32u,   // 2-D decoder with tables in HBM: per-lane write-back cache of 32 state banks in LDS (slice_kernels.hip)
};
constexpr uint32_t kSnapMaxSamples = 4096;  // a slice's samples are sorted by context inside one workgroup's LDS, 4096 at a time ...
constexpr uint32_t kSnapMaxChunks = 4;      // ... and a bigger slice (up to 16384 samples: 64x64 interleaved RGB, 128x128 planes) goes through the
                                            // pass in chunks of 4096 consecutive samples whose contexts' states are carried from chunk to chunk
                                            // through the slice's table in HBM (snapshot_kernels.hip).  Beyond that the table encoder stays:
                                            // 256x256 planes (16 chunks, a few thousand slices per launch) are one wavefront's dependent chain
                                            // whatever feeds it, and 48 more launches in front of it cost 9 % (profiles/r06_chunked_snapshot_ab.txt)

// Test / tuning hooks.  They are read from the environment ONCE per process (codec.hip: current_tuning; a test that
// changes them calls llcomp_mi_reload_tuning), they select the kernel family when a codec object is created, and none
// of them changes a single output byte.
struct Tuning {
    int lane_shift = -1;       // LLCOMP_MI_LANE_SHIFT: force the lane-group width (0..6)
    int lpw = 0;               // LLCOMP_MI_LPW: fewer active lanes per wavefront
    bool norows = false;       // LLCOMP_MI_NOROWS=1: 1-row slices through the general table-per-slice kernels
    bool noldstab = false;     // LLCOMP_MI_NOLDSTAB=1: single-slice launches keep their table in HBM
    bool force_replay = false; // LLCOMP_MI_FORCE_REPLAY=1
    bool nosnap = false;       // LLCOMP_MI_NOSNAP=1: the 2-D encoder keeps its state tables in HBM (the path before round 4)
    bool nocache = false;      // LLCOMP_MI_NOCACHE=1: the 2-D decoder fetches and writes every state bank in HBM (the path before round 5)
    int overlap = 2;           // LLCOMP_MI_OVERLAP: slices above 4096 samples -- 2 (default): the snapshot pass of chunk c + 1 runs beside the coding of
                               // chunk c on ONE second stream per device, shared by all codec objects; 1: on a second stream of the codec's own
                               // (fine for one or two pipelines, 25 % below in-order with three: too many queues); 0: in order on the caller's
                               // stream (profiles/r06_chunked_snapshot_ab.txt)
    bool nofeedback = false;   // LLCOMP_MI_NOFEEDBACK=1: the bank cache stays on in every launch, whatever the last one's wavefronts did with it (A/B)
};
inline Tuning tuning_from_env() {
    Tuning t;
    auto num = [](const char* name, long lo, long hi, int dflt) {
        const char* e = std::getenv(name);
        if (!e || !*e) return dflt;
        const long v = std::strtol(e, nullptr, 10);
        return (v >= lo && v <= hi) ? int(v) : dflt;
    };
    auto flag = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; };
    t.lane_shift = num("LLCOMP_MI_LANE_SHIFT", 0, 6, -1);
    t.lpw = num("LLCOMP_MI_LPW", 1, 64, 0);
    t.norows = flag("LLCOMP_MI_NOROWS");
    t.noldstab = flag("LLCOMP_MI_NOLDSTAB");
    t.force_replay = flag("LLCOMP_MI_FORCE_REPLAY");
    t.nosnap = flag("LLCOMP_MI_NOSNAP");
    t.nocache = flag("LLCOMP_MI_NOCACHE");
    t.nofeedback = flag("LLCOMP_MI_NOFEEDBACK");
    t.overlap = num("LLCOMP_MI_OVERLAP", 0, 2, 2);
    return t;
}

// snapshot pass (2-D encoder): chunks of a slice, and its sample capacity in the piece-layout arrays (a multiple of 16; whole chunks
// when there are several, so that chunk c starts at sample c * 4096 = piece boundaries of every array)
LLMI_HD inline uint32_t snapshot_chunks(const Geometry& g) { return (g.slice_samples + kSnapMaxSamples - 1) / kSnapMaxSamples; }
LLMI_HD inline uint32_t snapshot_cap(const Geometry& g) {
    return g.slice_samples <= kSnapMaxSamples ? (g.slice_samples + 15u) & ~15u : snapshot_chunks(g) * kSnapMaxSamples;
}

constexpr int kBankCacheLog2 = 5;  // entries per lane of the 2-D decoder's bank cache (slice_kernels.hip): ONE constant for flag, launcher, kernel
inline int bank_cache_log2(const Geometry& g) { return (g.flags & kGeoBankCache) ? kBankCacheLog2 : 0; }

// ---- the row encoder's pixel reads (planar 1-row slices that the encoder reads from the pixel batch: rows_encoder_reads_pixels) ----
// A lane reads sample k of its slice as ONE dword at tile_base + k*C.  That dword stays inside the caller's batch of T bytes iff
// tile_base + k*C + 4 <= T.  Only the last u = ceil(4/C) - 1 pixels of the batch fail that (3 for C = 1, 1 for C = 2 and 3, none for
// C = 4), and each of them is among the last u samples of its own slice (the pixels behind it in the batch include the rest of its
// tile).  rows_px_dwords: how many leading samples of a slice may be read as a dword -- at least samples - u, since sample
// samples - 1 - u ends at tile_base + (samples - 1 - u)*C + 4 <= T - (u + 1)*C + 4 <= T; the rest are read byte by byte.
LLMI_HD inline uint32_t rows_px_dwords(uint64_t tile_base, uint32_t samples, uint32_t c, uint64_t batch_bytes) {
    if (tile_base + 4 > batch_bytes) return 0;
    const uint64_t k = (batch_bytes - 4 - tile_base) / c + 1;  // samples 0 .. k-1 end at or before the batch's end
    return k < samples ? uint32_t(k) : samples;
}
// The samples at the end of a slice that the encoder's bulk loop (no per-lane tests; sample i + 2 is loaded while sample i is coded)
// leaves to the loop with tests: it loads samples up to samples - rows_px_tail(c) + 1 = samples - 1 - u, all of them dwords by the above.
LLMI_HD inline uint32_t rows_px_tail(uint32_t c) { return 1 + (4 + c - 1) / c; }

// lane order: element k of slice `id` inside an array laid out [group][k][group width]
LLMI_HD inline size_t lane_order_index(const Geometry& g, uint32_t id, uint32_t k) {
    const uint32_t gw = 1u << g.lane_shift;
    return ((size_t(id >> g.lane_shift) * g.slice_samples + k) << g.lane_shift) + (id & (gw - 1));
}

struct SliceRect {
    uint32_t frame, x0, y0, sw, sh, ch;  // ch = first channel of the slice (planar) or 0
};

LLMI_HD inline SliceRect slice_rect(const Geometry& g, uint32_t id) {
    SliceRect r;
    r.frame = id / g.slices_per_frame;
    uint32_t s = id - r.frame * g.slices_per_frame;
    uint32_t tile = s;
    r.ch = 0;
    if (g.planar) {
        tile = s / g.c;
        r.ch = s - tile * g.c;
    }
    const uint32_t ty = tile / g.ntx, tx = tile - ty * g.ntx;
    r.x0 = tx * g.tile_w;
    r.y0 = ty * g.tile_h;
    r.sw = g.w - r.x0 < g.tile_w ? g.w - r.x0 : g.tile_w;
    r.sh = g.h - r.y0 < g.tile_h ? g.h - r.y0 : g.tile_h;
    return r;
}

// Width of a lane group = slices per wavefront.  A wavefront owns whole rows of the lane-order arrays (rows shared
// between wavefronts on different XCDs are false sharing across non-coherent L2s: measured 2x slower), so the only
// knob for "few slices" is a narrower group: full 64-lane groups as soon as that still gives >= kMinWaves wavefronts.
inline uint32_t default_lane_shift(uint32_t n_slices) {
    constexpr uint32_t kMinWaves = 96;
    uint32_t s = 6;
    while (s > 0 && (n_slices >> s) < kMinWaves) --s;
    return s;
}

inline bool make_geometry(Geometry& g, uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w,
                          uint32_t tile_h, uint32_t planar, const Tuning& tune = Tuning{}, bool small_model = false) {
    if (!frames || !w || !h || c < 1 || c > kMaxChannels) return false;
    if (tile_w == 0 || tile_w > w) tile_w = w;
    if (tile_h == 0 || tile_h > h) tile_h = h;
    const uint64_t samples = uint64_t(w) * h * c;
    if (samples >= (1ull << 31)) return false;
    g.frames = frames; g.w = w; g.h = h; g.c = c;
    g.tile_w = tile_w; g.tile_h = tile_h; g.planar = planar ? 1 : 0;
    g.ntx = (w + tile_w - 1) / tile_w;
    g.nty = (h + tile_h - 1) / tile_h;
    const uint64_t spf = uint64_t(g.ntx) * g.nty * (g.planar ? c : 1);
    if (spf * frames >= (1ull << 31)) return false;
    g.slices_per_frame = uint32_t(spf);
    g.n_slices = uint32_t(spf * frames);
    g.nch = g.planar ? 1 : c;
    // 13 B/sample bound + slack.  A slice beyond 165 M samples (only a legacy whole-image stream can be that big) gets
    // the largest capacity the kernels' 32-bit stream positions allow; real streams stay below 1.3 B/sample and an
    // overflow would be reported, never written.
    const uint64_t cap = (uint64_t(tile_w) * tile_h * g.nch * 13 + 32 + 15) & ~15ull;
    g.slice_cap = uint32_t(cap < 0x7FFFFFF0ull ? cap : 0x7FFFFFF0ull);
    g.slice_samples = tile_w * tile_h * g.nch;
    g.lane_shift = tune.lane_shift >= 0 ? uint32_t(tune.lane_shift) : default_lane_shift(g.n_slices);
    // A few hundred BIG slices (whole-image streams in bulk, one frame in 256x256 tiles): one slice per wavefront, so that every
    // slice's 63 KB state table sits in LDS (two per CU: 512 fit the GPU at once) instead of HBM -- +13 % measured on 512 legacy
    // streams and on one 4K frame in 256x256 tiles; smaller slices have the snapshot encoder and stay several to a wavefront.
    if (tune.lane_shift < 0 && g.tile_h > 1 && g.slice_samples > kSnapMaxSamples && g.n_slices <= 512) g.lane_shift = 0;
    const uint32_t gw = 1u << g.lane_shift;
    g.lpw = gw;
    if (tune.lpw >= 1) {  // rounded down to a power of two: a wavefront never straddles lane groups
        uint32_t p = 1;
        while (p * 2 <= uint32_t(tune.lpw) && p * 2 <= gw) p *= 2;
        g.lpw = p;
    }
    g.flags = 0;
    if (g.tile_h == 1 && !tune.norows && g.nch <= 4) g.flags |= kGeoRows;  // (the register-resident row kernels exist for 1..4 channels)
    else if (g.lpw == 1 && !tune.noldstab) g.flags |= kGeoLdsTable;
    else if (g.slice_samples <= kSnapMaxSamples * kSnapMaxChunks && !tune.nosnap) g.flags |= kGeoSnapshot;
    // The decoder of the families with tables in HBM (1..4 channels per slice): bank cache in LDS.
    if (!(g.flags & (kGeoRows | kGeoLdsTable)) && g.nch <= 4 && !tune.nocache) g.flags |= kGeoBankCache;
    if (tune.force_replay) g.flags |= kGeoForceReplay;
    if (small_model) g.flags |= kGeoSmallModel;
    return true;
}

// A LEGACY stream has no length on the wire: it is whatever follows the header.  No decoder reads more than 2 bytes + 65 a sample of
// it (the range decoder takes at most one byte per bin; a sample is at most the zero flag, 31 ones and the closing zero, 31 mantissa
// bits and the sign, and a run of 32 ones ends the stream), so bytes beyond that bound are never read and the length is clamped to it.
// (64-bit: the bound passes 2^32 beyond 66 M samples.)
inline uint64_t legacy_read_bound(uint64_t samples) { return 65 * samples + 2; }
// A geometry whose one slice can stage a LEGACY stream of `bytes` (already clamped to legacy_read_bound): the decoder's TRUNCATED
// limit, slice_cap - 16, must not cut a stream the reference reads whole.  Beyond the kernels' 32-bit stream positions it stays
// capped (a > 2 GB stream is TRUNCATED).
inline void fit_legacy_stream(Geometry& g, uint64_t bytes) {
    const uint64_t cap = (bytes + 16 + 15) & ~15ull;
    if (cap > g.slice_cap) g.slice_cap = uint32_t(cap < 0x7FFFFFF0ull ? cap : 0x7FFFFFF0ull);
}

// ---- region decode (DESIGN.md "Region decode") ----------------------------------------------------------------------------
// A rectangle (x, y, rw, rh) of one frame is rebuilt from the slices of the tiles it touches alone: every slice is the reference
// stream of its own crop, with fresh state and slice-local borders.  Tile columns [tx0, tx1) x tile rows [ty0, ty1) are covered.
struct RegionBox {
    uint32_t tx0, ty0, tx1, ty1;
};
// false for an empty rectangle or one that leaves the image (the sums are taken in 64 bits: an x + rw that wraps is refused);
// tile_w / tile_h 0 (or beyond the image) = the whole width / height
inline bool region_box(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                       RegionBox& b) {
    if (!w || !h || !rw || !rh || uint64_t(x) + rw > w || uint64_t(y) + rh > h) return false;
    if (tile_w == 0 || tile_w > w) tile_w = w;
    if (tile_h == 0 || tile_h > h) tile_h = h;
    const uint64_t ntx = (uint64_t(w) + tile_w - 1) / tile_w, nty = (uint64_t(h) + tile_h - 1) / tile_h;
    b.tx0 = x / tile_w;
    b.ty0 = y / tile_h;
    b.tx1 = uint32_t(std::min<uint64_t>((uint64_t(x) + rw + tile_w - 1) / tile_w, ntx));
    b.ty1 = uint32_t(std::min<uint64_t>((uint64_t(y) + rh + tile_h - 1) / tile_h, nty));
    return true;
}
// The geometry of the covered sub-image: same frames, channels, tiling, planar setting, tuning and small model as `full`, width
// min(tx1 * tile_w, w) - tx0 * tile_w (height alike).  Sub-slice j IS covered slice j of `full`, with the same dimensions (ids run
// frame-major, then tile row, tile column, plane; region_full_id).  When only the partial last tile column / row is covered,
// make_geometry clamps tile_w / tile_h to the sub-image and the kernel family may change (a 1-row remainder of 2-row tiles runs the
// row kernels): the bytes cannot, each slice being the reference stream of its crop.
// The sub-geometry keeps the full one's bytes per slice: the same TRUNCATED limit as a full decode (the nominal tile's, also for a
// partial tile alone), and a LEGACY stream longer than 13 B/sample (fit_legacy_stream) stages whole.
inline bool region_geometry(const Geometry& full, const RegionBox& b, const Tuning& tune, Geometry& sub) {
    const uint32_t w = std::min<uint64_t>(uint64_t(b.tx1) * full.tile_w, full.w) - b.tx0 * full.tile_w;
    const uint32_t h = std::min<uint64_t>(uint64_t(b.ty1) * full.tile_h, full.h) - b.ty0 * full.tile_h;
    if (!make_geometry(sub, full.frames, w, h, full.c, full.tile_w, full.tile_h, full.planar, tune, (full.flags & kGeoSmallModel) != 0))
        return false;
    sub.slice_cap = full.slice_cap;
    return true;
}
LLMI_HD inline uint32_t region_full_id(const Geometry& full, const Geometry& sub, const RegionBox& b, uint32_t j) {
    const uint32_t f = j / sub.slices_per_frame, s = j - f * sub.slices_per_frame;
    const uint32_t planes = full.planar ? full.c : 1u;
    const uint32_t tile = s / planes, ch = s - tile * planes;
    const uint32_t ty = tile / sub.ntx, tx = tile - ty * sub.ntx;
    return f * full.slices_per_frame + ((b.ty0 + ty) * full.ntx + b.tx0 + tx) * planes + ch;
}
// Does every array the decoder touches for `sub` fit the one the codec sized for `full`?  Lane groups x group width (scratch, state
// tables), x samples per slice (lane-order arrays), bytes per slice (scratch).  default_lane_shift is monotone, so this holds by
// default; forced LLCOMP_MI_LANE_SHIFT / LLCOMP_MI_LPW and the "few big slices: one per wavefront" rule are checked, not assumed.
// A sub-geometry that needs the image-order intermediate needs it of a codec that has one (`full` not on the fused row path).
// (region_fits: the same frames; regions_fits: a class of them)
inline bool sub_arrays_fit(const Geometry& full, const Geometry& sub) {
    auto lanes = [](const Geometry& g) { return ((uint64_t(g.n_slices) + (1u << g.lane_shift) - 1) >> g.lane_shift) << g.lane_shift; };
    auto fused = [](const Geometry& g) { return g.planar && (g.flags & kGeoRows) && g.c <= 4; };
    if (sub.c != full.c || sub.n_slices > full.n_slices) return false;
    if (lanes(sub) > lanes(full)) return false;
    if (lanes(sub) * sub.slice_samples > lanes(full) * full.slice_samples) return false;
    if (uint64_t(lanes(sub)) * sub.slice_cap > uint64_t(lanes(full)) * full.slice_cap) return false;
    if (!fused(sub) && fused(full)) return false;
    return true;
}
inline bool region_fits(const Geometry& full, const Geometry& sub) { return sub.frames == full.frames && sub_arrays_fit(full, sub); }

// ---- region update (DESIGN.md "Region update"): the ENCODER on the covered box's sub-geometry ---------------------------------------
// region_full_id the other way round: the sub-slice that full slice `id` is, or ~0u for a slice outside the box
LLMI_HD inline uint32_t region_sub_id(const Geometry& full, const Geometry& sub, const RegionBox& b, uint32_t id) {
    const uint32_t f = id / full.slices_per_frame, s = id - f * full.slices_per_frame;
    const uint32_t planes = full.planar ? full.c : 1u;
    const uint32_t tile = s / planes, ch = s - tile * planes;
    const uint32_t ty = tile / full.ntx, tx = tile - ty * full.ntx;
    if (tx < b.tx0 || tx >= b.tx1 || ty < b.ty0 || ty >= b.ty1) return ~0u;
    return f * sub.slices_per_frame + ((ty - b.ty0) * sub.ntx + tx - b.tx0) * planes + ch;
}
// is the rectangle exactly the box's pixels (tile-aligned, or reaching the image edge)?  Then nothing of the old box is needed.
inline bool region_is_whole_box(const Geometry& full, const Geometry& sub, const RegionBox& b, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh) {
    return x == b.tx0 * full.tile_w && y == b.ty0 * full.tile_h && rw == sub.w && rh == sub.h;
}
// elements per snapshot array of `g` (snapshot_kernels.hip: snapshot_elems), 0 for a family without the pass
inline uint64_t snapshot_elems_of(const Geometry& g) {
    if (!(g.flags & kGeoSnapshot)) return 0;
    return (((uint64_t(g.n_slices) + (1u << g.lane_shift) - 1) >> g.lane_shift) * snapshot_cap(g)) << g.lane_shift;
}
// The most elements the snapshot arrays of a sub-geometry of `full` can take (what the codec counts in its workspace): the codec's own
// arrays when it runs the pass itself; else a sub-image of clamped tiles, or of more slices per wavefront, may run it where the codec's
// family does not (tables in LDS, or slices above 16384 samples) -- at most the full geometry's lanes x the full slice's capacity in the
// arrays, 16384 samples at the most.  None for 1-row slices (they stay 1-row slices) and where LLCOMP_MI_NOSNAP took the pass away.
inline uint64_t region_snapshot_bound(const Geometry& full) {
    if (full.flags & kGeoSnapshot) return snapshot_elems_of(full);
    if (full.flags & kGeoRows) return 0;
    if (!(full.flags & kGeoLdsTable) && full.slice_samples <= kSnapMaxSamples * kSnapMaxChunks) return 0;
    const uint64_t lanes = ((uint64_t(full.n_slices) + (1u << full.lane_shift) - 1) >> full.lane_shift) << full.lane_shift;
    const uint64_t cap = full.slice_samples <= kSnapMaxSamples ? (full.slice_samples + 15u) & ~15u
                                                               : uint64_t(std::min(snapshot_chunks(full), kSnapMaxChunks)) * kSnapMaxSamples;
    return lanes * cap;
}
// Does every array the ENCODER touches for `sub` fit what the codec sized for `full`?  What the decoder touches (sub_arrays_fit) and:
//   * the lane-order array, which is also the snapshot pass's entries (u32 per element): bytes, not samples -- a fused codec holds 16-bit
//     symbols, and the pass's capacity per slice is rounded up (to 16 samples, or to whole chunks of 4096);
//   * the snapshot arrays, against region_snapshot_bound;
//   * the coder's parking records (64 B per slice) and the group offsets: the sub-geometry can have MORE lane groups than the full one
//     (a narrower lane group for fewer slices), so the encoder's offsets go to an array of n_slices + 1 entries of its own, which
//     always holds them: lane groups <= slices of the sub-geometry <= slices of the full one.
inline bool region_encode_fits(const Geometry& full, const Geometry& sub) {
    if (!region_fits(full, sub)) return false;
    auto lanes = [](const Geometry& g) { return ((uint64_t(g.n_slices) + (1u << g.lane_shift) - 1) >> g.lane_shift) << g.lane_shift; };
    auto fused = [](const Geometry& g) { return g.planar && (g.flags & kGeoRows) && g.c <= 4; };
    auto lane_bytes = [&](const Geometry& g) { return std::max(lanes(g) * g.slice_samples * (fused(g) ? 2u : 4u), snapshot_elems_of(g) * 4); };
    if (lane_bytes(sub) > lane_bytes(full)) return false;
    if (snapshot_elems_of(sub) > region_snapshot_bound(full)) return false;
    if (lanes(sub) >> sub.lane_shift > uint64_t(full.n_slices)) return false;
    return true;
}

// ---- regions decode: a rectangle of one size at an offset of its own in every frame (DESIGN.md "Region decode") -----------------
// To run the decoder on ONE sub-geometry, every frame decodes a WINDOW of tiles of a fixed size instead of its exact covered box:
// Wx = min(ntx, (rw + tile_w - 2) / tile_w + 1) tile columns, the most a rectangle of width rw can touch, from
// wx0 = min(x / tile_w, ntx - Wx) (rows alike).  The window always contains region_box's box.  Where the window holds the partial
// last tile column (row) its pixel width (height) differs, so frames fall into at most 2 x 2 classes: bit 0 = the window ends at
// a partial last tile column, bit 1 = at a partial last tile row.  Each class is one sub-geometry.
constexpr uint32_t kRegionsClasses = 4;
// The window of a rectangle (x, y, rw, rh) sized for a batch whose largest rectangle is wmax x hmax (rw <= wmax <= w, rh <= hmax <= h):
// Wx from wmax, wx0 = min(x / tile_w, ntx - Wx).  It contains the rectangle's box, and a wmax x hmax box that contains the rectangle
// fits in it.  false for an empty rectangle, one that leaves the image (region_box), or a size above wmax / hmax.
inline bool regions_window_sized(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                                 uint32_t wmax, uint32_t hmax, RegionBox& win, uint32_t& cls) {
    RegionBox b;
    if (!region_box(w, h, tile_w, tile_h, x, y, rw, rh, b) || rw > wmax || rh > hmax || wmax > w || hmax > h) return false;
    if (tile_w == 0 || tile_w > w) tile_w = w;
    if (tile_h == 0 || tile_h > h) tile_h = h;
    const uint32_t ntx = uint32_t((uint64_t(w) + tile_w - 1) / tile_w), nty = uint32_t((uint64_t(h) + tile_h - 1) / tile_h);
    const uint32_t wx = uint32_t(std::min<uint64_t>(ntx, (uint64_t(wmax) + tile_w - 2) / tile_w + 1));
    const uint32_t wy = uint32_t(std::min<uint64_t>(nty, (uint64_t(hmax) + tile_h - 2) / tile_h + 1));
    win.tx0 = std::min(x / tile_w, ntx - wx);
    win.ty0 = std::min(y / tile_h, nty - wy);
    win.tx1 = win.tx0 + wx;
    win.ty1 = win.ty0 + wy;
    cls = (w % tile_w != 0 && win.tx1 == ntx ? 1u : 0u) | (h % tile_h != 0 && win.ty1 == nty ? 2u : 0u);
    return true;
}
// false for an empty rectangle or one that leaves the image (region_box); tile_w / tile_h 0 (or beyond the image) = the whole width / height
inline bool regions_window(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                           RegionBox& win, uint32_t& cls) {
    return regions_window_sized(w, h, tile_w, tile_h, x, y, rw, rh, rw, rh, win, cls);
}
// One class's sub-geometry: region_geometry of its window, with the class's frame count.
inline bool regions_geometry(const Geometry& full, const RegionBox& win, uint32_t frames, const Tuning& tune, Geometry& sub) {
    const uint32_t w = std::min<uint64_t>(uint64_t(win.tx1) * full.tile_w, full.w) - win.tx0 * full.tile_w;
    const uint32_t h = std::min<uint64_t>(uint64_t(win.ty1) * full.tile_h, full.h) - win.ty0 * full.tile_h;
    if (!make_geometry(sub, frames, w, h, full.c, full.tile_w, full.tile_h, full.planar, tune, (full.flags & kGeoSmallModel) != 0))
        return false;
    sub.slice_cap = full.slice_cap;
    return true;
}
// One frame of a class, as the kernels see it (kernels.hpp): the class's frames are entries [first, first + frames) of one table.
struct RegionsFrame {
    uint32_t frame;     // the frame of the full batch whose slices are read
    uint32_t wx0, wy0;  // the window's first tile column / row
    uint32_t cx0, cy0;  // the rectangle's origin inside the window, in pixels
    uint32_t out;       // output frame: the rectangle goes to d_px[out]
    uint32_t cls, pad;
};
// sub-slice j of a class -> its slice of the full batch (frame-major, then tile row, tile column, plane, as region_full_id)
LLMI_HD inline uint32_t regions_full_id(const Geometry& full, const Geometry& sub, const RegionsFrame* tab, uint32_t j) {
    const uint32_t f = j / sub.slices_per_frame, s = j - f * sub.slices_per_frame;
    const uint32_t planes = full.planar ? full.c : 1u;
    const uint32_t tile = s / planes, ch = s - tile * planes;
    const uint32_t ty = tile / sub.ntx, tx = tile - ty * sub.ntx;
    return tab[f].frame * full.slices_per_frame + ((tab[f].wy0 + ty) * full.ntx + tab[f].wx0 + tx) * planes + ch;
}
// region_fits for a class: its frames are some of the batch's
inline bool regions_fits(const Geometry& full, const Geometry& sub) { return sub.frames <= full.frames && sub_arrays_fit(full, sub); }

// ---- resampling limits of the resized calls and the views plan (resize_plan.hpp; container.cpp: views_union) --------------------------
// An axis in_len -> out_len under filter code `filter` (LLCOMP_MI_FILTER_*) is refused for in_len or out_len 0, an unknown filter, or a
// downscale above the filter's limit: R * in_len > kResizeMaxDown * out_len with R = 1, but 2 for bicubic and 3 for Lanczos, so that the
// filter's support never passes kResizeMaxDown input samples and K <= 129.
constexpr uint32_t kResizeMaxDown = 64;
constexpr uint32_t kResizeFilters = 6;
inline bool resize_axis_ok(uint32_t filter, uint32_t in_len, uint32_t out_len) {
    constexpr uint32_t kReach[kResizeFilters] = {1, 1, 1, 1, 2, 3};
    return filter < kResizeFilters && in_len && out_len && uint64_t(kReach[filter]) * in_len <= uint64_t(kResizeMaxDown) * out_len;
}

}  // namespace llcomp_mi
