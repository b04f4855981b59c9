// container.cpp -- parsing / assembling the two wire formats and the multi-GPU band concatenator.
// Host-only logic (no kernels, no coded bytes are produced here): it moves slice tables and payloads around.
#include "container.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "host_result.hpp"

namespace llcomp_mi {

void write_legacy_header(uint8_t* o, uint32_t w, uint32_t h, uint32_t c) {
    o[0] = LLCOMP_MI_MAGIC_LEGACY;  // llcomp.hpp:375-378
    o[1] = uint8_t(c);
    o[2] = uint8_t(w & 0xFF); o[3] = uint8_t((w >> 8) & 0xFF);
    o[4] = uint8_t(h & 0xFF); o[5] = uint8_t((h >> 8) & 0xFF);
}

void write_sliced_header(uint8_t* o, const Geometry& g) {
    o[0] = LLCOMP_MI_MAGIC_SLICED; o[1] = 1; o[2] = uint8_t(g.c);
    o[3] = uint8_t((g.planar ? 1 : 0) | ((g.flags & kGeoSmallModel) ? 2 : 0));
    put_u32le(o + 4, g.w); put_u32le(o + 8, g.h);
    put_u32le(o + 12, g.tile_w); put_u32le(o + 16, g.tile_h);
    put_u32le(o + 20, g.slices_per_frame);
}

PayloadSpan covered_span(const llcomp_mi_info& info, const uint8_t* data, size_t len, const uint32_t box[4]) {
    const uint64_t payload = len - info.payload_offset;
    if (info.format == LLCOMP_MI_FORMAT_LEGACY) return {0, payload};
    const uint32_t planes = info.planar ? info.channels : 1u, ntx = (info.width + info.tile_w - 1) / info.tile_w;
    const uint64_t first = (uint64_t(box[1]) * ntx + box[0]) * planes, last = ((uint64_t(box[3]) - 1) * ntx + box[2] - 1) * planes + planes - 1;
    const uint8_t* tab = data + info.table_offset;  // (probe has made sure the table is all there)
    uint64_t begin = 0, pos = 0;
    for (uint64_t i = 0; i <= last; ++i) {
        if (i == first) begin = pos;
        pos += get_u32le(tab + 4 * i);
    }
    return {std::min(begin, payload), std::min(pos, payload)};
}

int regions_gather_plan(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* xy, uint32_t rw, uint32_t rh,
                        RegionsGather& p) {
    p = RegionsGather{};
    if (!data || !lens || !xy || !n) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> rects(4 * size_t(n));
    for (uint32_t f = 0; f < n; ++f) {
        rects[4 * f + 0] = xy[2 * f];
        rects[4 * f + 1] = xy[2 * f + 1];
        rects[4 * f + 2] = rw;
        rects[4 * f + 3] = rh;
    }
    return regions_gather_plan_sized(data, lens, n, rects.data(), rw, rh, p);
}

int regions_gather_plan_sized(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* rects, uint32_t wmax, uint32_t hmax,
                              RegionsGather& p, const uint32_t* used, uint32_t n_used) {
    p = RegionsGather{};
    if (!data || !lens || !rects || !n || (used && !n_used)) return LLCOMP_MI_BAD_ARGS;
    const uint32_t m = used ? n_used : n;  // the frames that take part: entry i is frame used[i], or frame i
    llcomp_mi_info i0{};
    std::vector<uint32_t> cls(m), first_run(m + 1);
    std::vector<GatherRun> runs;  // frame order
    uint32_t limit = 0, seen = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t f = used ? used[i] : i;
        if (f >= n || !data[f]) return LLCOMP_MI_BAD_ARGS;
        llcomp_mi_info a;
        if (int rc = llcomp_mi_probe(data[f], lens[f], &a)) return rc;
        if (a.format != LLCOMP_MI_FORMAT_SLICED) return LLCOMP_MI_BAD_ARGS;
        if (i == 0) {
            i0 = a;
            if (!make_geometry(p.g, 1, a.width, a.height, a.channels, a.tile_w, a.tile_h, a.planar, Tuning{}, a.small_model != 0))
                return LLCOMP_MI_BAD_ARGS;
            limit = p.g.slice_cap - 16;  // the SLICED per-entry limit (LLCOMP_MI_TRUNCATED; the decoders' own check)
        } else if (a.width != i0.width || a.height != i0.height || a.channels != i0.channels || a.tile_w != i0.tile_w ||
                   a.tile_h != i0.tile_h || a.planar != i0.planar || a.small_model != i0.small_model) {
            return LLCOMP_MI_BAD_ARGS;
        }
        RegionBox win;
        if (!regions_window_sized(a.width, a.height, a.tile_w, a.tile_h, rects[4 * size_t(f)], rects[4 * size_t(f) + 1], rects[4 * size_t(f) + 2],
                                  rects[4 * size_t(f) + 3], wmax, hmax, win, cls[i]))
            return LLCOMP_MI_BAD_ARGS;
        seen |= 1u << cls[i];
        // one window tile row = (wx1 - wx0) * planes consecutive slices; the table is summed up to the end of the last one only
        const uint32_t planes = a.planar ? a.channels : 1u, per_row = (win.tx1 - win.tx0) * planes;
        const uint8_t* tab = data[f] + a.table_offset;
        first_run[i] = uint32_t(runs.size());
        uint64_t off = 0;
        uint32_t s = 0;
        for (uint32_t ty = win.ty0; ty < win.ty1; ++ty) {
            const uint32_t first = (ty * p.g.ntx + win.tx0) * planes;
            for (; s < first; ++s) off += get_u32le(tab + 4ull * s);
            uint64_t bytes = 0;
            for (uint32_t j = 0; j < per_row; ++j, ++s) {
                const uint32_t l = get_u32le(tab + 4ull * s);
                if (l > limit) return LLCOMP_MI_TRUNCATED;
                bytes += l;
            }
            if (a.payload_offset + off + bytes > lens[f]) return LLCOMP_MI_TRUNCATED;
            runs.push_back(GatherRun{f, first, per_row, a.payload_offset + off, bytes});
            off += bytes;
        }
    }
    first_run[m] = uint32_t(runs.size());
    uint64_t slices = 0;
    p.runs.reserve(runs.size());
    for (uint32_t c = 0; c < kRegionsClasses; ++c)
        for (uint32_t i = 0; i < m; ++i)
            if (cls[i] == c)
                for (uint32_t r = first_run[i]; r < first_run[i + 1]; ++r) {
                    p.runs.push_back(runs[r]);
                    slices += runs[r].count;
                    p.payload_bytes += runs[r].bytes;
                }
    if (slices >= (1ull << 31)) return LLCOMP_MI_OUT_OF_RANGE;
    p.n_slices = uint32_t(slices);
    p.n_classes = uint32_t(__builtin_popcount(seen));
    return LLCOMP_MI_OK;
}

const llcomp_mi_view_group* view_group_at(const llcomp_mi_view_group* groups, uint32_t i) {
    return reinterpret_cast<const llcomp_mi_view_group*>(reinterpret_cast<const uint8_t*>(groups) + size_t(i) * groups->struct_size);
}

int views_union(uint32_t w, uint32_t h, uint32_t frames, const llcomp_mi_view_group* groups, uint32_t n_groups, ViewsUnion& u) {
    u = ViewsUnion{};
    if (!groups || !n_groups || !frames || !w || !h || groups->struct_size != sizeof(llcomp_mi_view_group)) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> x1(frames, 0), y1(frames, 0);  // (exclusive ends; rects holds the origins until the end)
    u.rects.assign(4 * size_t(frames), 0);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_view_group& gr = *view_group_at(groups, gi);
        if (gr.struct_size != sizeof(llcomp_mi_view_group) || !gr.n_views || gr.n_views > 65535 || !gr.views || !gr.ow || !gr.oh)
            return LLCOMP_MI_BAD_ARGS;
        for (uint32_t i = 0; i < gr.n_views; ++i) {
            const llcomp_mi_view& v = gr.views[i];
            const uint32_t filter = LLCOMP_MI_FLAG_FILTER_OF(v.flags & 0xFFu);
            if (v.frame >= frames || !v.rw || !v.rh || uint64_t(v.x) + v.rw > w || uint64_t(v.y) + v.rh > h) return LLCOMP_MI_BAD_ARGS;
            if (!resize_axis_ok(filter, v.rw, gr.ow) || !resize_axis_ok(filter, v.rh, gr.oh)) return LLCOMP_MI_BAD_ARGS;
            uint32_t* r = u.rects.data() + 4 * size_t(v.frame);
            if (!x1[v.frame]) {
                r[0] = v.x;
                r[1] = v.y;
            } else {
                r[0] = std::min(r[0], v.x);
                r[1] = std::min(r[1], v.y);
            }
            x1[v.frame] = std::max(x1[v.frame], v.x + v.rw);
            y1[v.frame] = std::max(y1[v.frame], v.y + v.rh);
        }
        u.total_views += gr.n_views;
    }
    for (uint32_t f = 0; f < frames; ++f) {
        if (!x1[f]) continue;
        uint32_t* r = u.rects.data() + 4 * size_t(f);
        r[2] = x1[f] - r[0];
        r[3] = y1[f] - r[1];
        u.wmax = std::max(u.wmax, r[2]);
        u.hmax = std::max(u.hmax, r[3]);
        u.used.push_back(f);
    }
    return LLCOMP_MI_OK;
}

void regions_gather_copy(const RegionsGather& p, const uint8_t* const* data, uint8_t* payload, uint32_t* slice_len, uint64_t* slice_off) {
    uint64_t at = 0;
    uint32_t k = 0;
    for (const GatherRun& r : p.runs) {
        const uint8_t* tab = data[r.frame] + LLCOMP_MI_SLICED_HEADER_BYTES + 4ull * r.first;
        for (uint32_t j = 0; j < r.count; ++j) slice_len[k + j] = get_u32le(tab + 4ull * j);
        if (slice_off) {
            uint64_t o = at;
            for (uint32_t j = 0; j < r.count; ++j) {
                slice_off[k + j] = o;
                o += slice_len[k + j];
            }
        }
        if (r.bytes) std::memcpy(payload + at, data[r.frame] + r.src, r.bytes);
        at += r.bytes;
        k += r.count;
    }
}

// llcomp_mi_replace_slices(_into): every check first, then the header, the new table, and the payload as runs of unchanged slices (one
// memcpy each) with the new slices in between.  out != nullptr: the caller's buffer of out_cap bytes, else malloc'ed -> *out_alloc.
static int replace_slices_common(const uint8_t* data, size_t len, const uint32_t* box, const uint32_t* new_len, const uint8_t* new_payload,
                                 uint8_t* out, size_t out_cap, uint8_t** out_alloc, size_t* out_len) {
    if (!data || !box || !new_len || !new_payload || !out_len || (!out && !out_alloc)) return LLCOMP_MI_BAD_ARGS;
    llcomp_mi_info a;
    if (int rc = llcomp_mi_probe(data, len, &a)) return rc;
    if (a.format != LLCOMP_MI_FORMAT_SLICED) return LLCOMP_MI_BAD_ARGS;
    Geometry g;
    if (!make_geometry(g, 1, a.width, a.height, a.channels, a.tile_w, a.tile_h, a.planar, Tuning{}, a.small_model != 0)) return LLCOMP_MI_BAD_ARGS;
    if (box[0] >= box[2] || box[1] >= box[3] || box[2] > g.ntx || box[3] > g.nty) return LLCOMP_MI_BAD_ARGS;
    const uint32_t limit = g.slice_cap - 16, planes = g.planar ? g.c : 1u;
    const uint8_t* tab = data + a.table_offset;
    const uint64_t old_payload = len - a.payload_offset;
    auto covered = [&](uint32_t i) {
        const uint32_t tile = i / planes, ty = tile / g.ntx, tx = tile - ty * g.ntx;
        return tx >= box[0] && tx < box[2] && ty >= box[1] && ty < box[3];
    };
    uint64_t old_off = 0, total = 0;
    uint32_t j = 0;
    for (uint32_t i = 0; i < g.slices_per_frame; ++i) {
        const uint32_t l = get_u32le(tab + 4ull * i);
        if (covered(i)) {
            if (new_len[j] > limit) return LLCOMP_MI_TRUNCATED;
            total += new_len[j++];
        } else {
            if (old_off + l > old_payload) return LLCOMP_MI_TRUNCATED;
            total += l;
        }
        old_off += l;  // (a covered slice's old bytes are skipped, never read)
    }
    HostOut res(out, out_cap, out_alloc, out_len);
    uint8_t* o = nullptr;
    if (int rc = res.take(size_t(a.payload_offset + total), o)) return rc;
    std::memcpy(o, data, LLCOMP_MI_SLICED_HEADER_BYTES);
    uint8_t* otab = o + LLCOMP_MI_SLICED_HEADER_BYTES;
    uint8_t* pay = o + a.payload_offset;
    const uint8_t* src = data + a.payload_offset;
    uint64_t run_at = 0, run = 0, new_at = 0;  // the pending run of unchanged slices: old payload bytes [run_at, run_at + run)
    old_off = 0;
    j = 0;
    for (uint32_t i = 0; i < g.slices_per_frame; ++i) {
        const uint32_t l = get_u32le(tab + 4ull * i);
        if (covered(i)) {
            if (run) std::memcpy(pay, src + run_at, run);
            pay += run;
            run = 0;
            put_u32le(otab + 4ull * i, new_len[j]);
            if (new_len[j]) std::memcpy(pay, new_payload + new_at, new_len[j]);
            pay += new_len[j];
            new_at += new_len[j++];
        } else {
            if (!run) run_at = old_off;
            run += l;
            put_u32le(otab + 4ull * i, l);
        }
        old_off += l;
    }
    if (run) std::memcpy(pay, src + run_at, run);
    res.commit();
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

using namespace llcomp_mi;

extern "C" {

// FNV-1a-64 (offset 1469598103934665603, prime 1099511628211): the checksum the golden vectors of this project are
// recorded in; `seed` = 0 starts a new hash, the previous result continues one over several pieces.
uint64_t llcomp_mi_fnv1a64(const uint8_t* data, size_t len, uint64_t seed) {
    uint64_t h = seed ? seed : 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) h = (h ^ data[i]) * 1099511628211ull;
    return h;
}

// Width of one-row slices (tile_h == 1) for a call that codes `frames` frames at once: the widest slice that still gives
// the GPU about four wavefronts per SIMD (1024 SIMDs x 64 lanes x 4 = 262 144 slices), never narrower than 64 pixels
// (narrow slices cost compression: every slice starts with fresh models) and never wider than 480 (the throughput
// default of bench.py).  Few-frame calls are latency-bound with wide slices: one 4K frame in 480x1 planes is 51 840
// slices = 0.8 wavefronts per SIMD (2.1 ms); the width this returns, 80, gives 4 per SIMD.
uint32_t llcomp_mi_suggest_tile_w(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t planar) {
    if (!frames || !w || !h || !c) return 0;
    const uint64_t target = 262144;
    const uint64_t rows = uint64_t(frames) * h * (planar ? c : 1);  // slices per tile column
    uint64_t cols = (target + rows - 1) / rows;                     // tile columns wanted
    if (cols < 1) cols = 1;
    uint64_t tw = (w + cols - 1) / cols;
    if (tw > 480) tw = 480;
    if (tw < 64) tw = 64;
    if (tw > w) tw = w;
    // prefer a width that divides the image width when one is near (no ragged last column)
    for (uint64_t d = tw; 4 * d >= 3 * tw && d >= 64; --d)
        if (w % d == 0) return uint32_t(d);
    return uint32_t(tw);
}

// The work split of the multi-GPU paths (multidev.hip: device lists; llcomp_amd/sharding.py: ranks, through ctypes).  A chunk is a
// run of whole tile rows: slices have fresh state and slice-local borders, so a band of whole tile rows coded as an image of its own
// yields exactly the full image's slices.  Chunk i belongs to part i % n_parts (fine interleaving: the cost of a slice follows its
// entropy, not its pixels).
int llcomp_mi_plan_chunks(uint32_t height, uint32_t tile_h, uint32_t n_parts, uint32_t chunks_per_part, uint32_t* triples,
                          uint32_t cap_chunks, uint32_t* n_chunks) {
    if (!height || !n_parts || !n_chunks) return LLCOMP_MI_BAD_ARGS;
    if (tile_h == 0 || tile_h > height) tile_h = height;
    if (chunks_per_part == 0) chunks_per_part = 4;
    const uint64_t nty = (uint64_t(height) + tile_h - 1) / tile_h;
    const uint64_t want = uint64_t(n_parts) * chunks_per_part;
    const uint64_t n = nty < want ? nty : want;  // >= 1
    *n_chunks = uint32_t(n);
    if (!triples) return LLCOMP_MI_OK;
    if (n > cap_chunks) return LLCOMP_MI_OUTPUT_OVERFLOW;
    uint64_t t = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t cnt = nty / n + (i < nty % n ? 1 : 0);
        triples[3 * i + 0] = uint32_t(t);
        triples[3 * i + 1] = uint32_t(t + cnt);
        triples[3 * i + 2] = uint32_t(i % n_parts);
        t += cnt;
    }
    return LLCOMP_MI_OK;
}

uint32_t llcomp_mi_slice_count(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar) {
    Geometry g;
    if (!make_geometry(g, 1, w, h, c, tile_w, tile_h, planar)) return 0;
    return g.slices_per_frame;
}

int llcomp_mi_region_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t x, uint32_t y,
                          uint32_t rw, uint32_t rh, uint32_t box[4], uint32_t* slices_per_frame) {
    if (!box || !slices_per_frame || c < 1 || c > kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    RegionBox b;
    if (!region_box(w, h, tile_w, tile_h, x, y, rw, rh, b)) return LLCOMP_MI_BAD_ARGS;
    const uint64_t n = uint64_t(b.tx1 - b.tx0) * (b.ty1 - b.ty0) * (planar ? c : 1u);
    if (n >= (1ull << 31)) return LLCOMP_MI_OUT_OF_RANGE;
    box[0] = b.tx0;
    box[1] = b.ty0;
    box[2] = b.tx1;
    box[3] = b.ty1;
    *slices_per_frame = uint32_t(n);
    return LLCOMP_MI_OK;
}

// The window loop of the three plans below: the windows (sized for wmax x hmax) of the n rectangles rects[4 * f ..], f = used[i], or i
// where there is no frame list.  Every rectangle is checked before anything is written; then frame f's window goes to windows[4 * f ..]
// (`clear` frames of zeros first, for the frames a list does not name) and the number of classes met to *n_classes.
static int plan_windows(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, const uint32_t* rects, const uint32_t* used, uint32_t n,
                        uint32_t wmax, uint32_t hmax, uint32_t clear, uint32_t* windows, uint32_t* n_classes) {
    uint32_t seen = 0;
    for (int pass = 0; pass < (windows ? 2 : 1); ++pass) {
        if (pass && clear) std::memset(windows, 0, 16 * size_t(clear));
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t f = used ? used[i] : i;
            const uint32_t* r = rects + 4 * size_t(f);
            RegionBox b;
            uint32_t cls = 0;
            if (!regions_window_sized(w, h, tile_w, tile_h, r[0], r[1], r[2], r[3], wmax, hmax, b, cls)) return LLCOMP_MI_BAD_ARGS;
            seen |= 1u << cls;
            if (!pass) continue;
            windows[4 * size_t(f) + 0] = b.tx0;
            windows[4 * size_t(f) + 1] = b.ty0;
            windows[4 * size_t(f) + 2] = b.tx1;
            windows[4 * size_t(f) + 3] = b.ty1;
        }
    }
    *n_classes = uint32_t(__builtin_popcount(seen));
    return LLCOMP_MI_OK;
}

int llcomp_mi_regions_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t rw, uint32_t rh,
                           const uint32_t* xy, uint32_t n, uint32_t* windows, uint32_t* n_classes) {
    (void)planar;
    if (!xy || !n || !n_classes || c < 1 || c > kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    std::vector<uint32_t> rects(4 * size_t(n));
    for (uint32_t f = 0; f < n; ++f) {
        rects[4 * size_t(f) + 0] = xy[2 * size_t(f)];
        rects[4 * size_t(f) + 1] = xy[2 * size_t(f) + 1];
        rects[4 * size_t(f) + 2] = rw;
        rects[4 * size_t(f) + 3] = rh;
    }
    return plan_windows(w, h, tile_w, tile_h, rects.data(), nullptr, n, rw, rh, 0, windows, n_classes);
}

int llcomp_mi_resized_regions_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, const uint32_t* rects,
                                   uint32_t n, uint32_t* windows, uint32_t* n_classes) {
    (void)planar;
    if (!rects || !n || !n_classes || c < 1 || c > kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    uint32_t wmax = 0, hmax = 0;
    for (uint32_t f = 0; f < n; ++f) {
        wmax = std::max(wmax, rects[4 * size_t(f) + 2]);
        hmax = std::max(hmax, rects[4 * size_t(f) + 3]);
    }
    return plan_windows(w, h, tile_w, tile_h, rects, nullptr, n, wmax, hmax, 0, windows, n_classes);
}

int llcomp_mi_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                         const llcomp_mi_view_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows, uint32_t* n_used,
                         uint32_t* n_classes) {
    (void)planar;
    if (!n_used || !n_classes || c < 1 || c > kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    ViewsUnion u;
    if (int rc = views_union(w, h, frames, groups, n_groups, u)) return rc;
    // (the union of rectangles inside the image is inside the image: regions_window_sized cannot refuse one)
    if (int rc = plan_windows(w, h, tile_w, tile_h, u.rects.data(), u.used.data(), uint32_t(u.used.size()), u.wmax, u.hmax, frames, windows, n_classes))
        return rc;
    if (unions) std::memcpy(unions, u.rects.data(), u.rects.size() * 4);
    *n_used = uint32_t(u.used.size());
    return LLCOMP_MI_OK;
}

int llcomp_mi_regions_gather(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* xy, uint32_t rw, uint32_t rh,
                             uint8_t* payload, uint64_t payload_cap, uint32_t* slice_len, uint32_t len_cap, uint64_t* payload_bytes,
                             uint32_t* n_slices, uint32_t* n_classes) {
    if (!payload_bytes || !n_slices || !n_classes) return LLCOMP_MI_BAD_ARGS;
    *payload_bytes = 0;
    *n_slices = *n_classes = 0;
    RegionsGather p;
    if (int rc = regions_gather_plan(data, lens, n, xy, rw, rh, p)) return rc;
    *payload_bytes = p.payload_bytes;
    *n_slices = p.n_slices;
    *n_classes = p.n_classes;
    if (!payload || !slice_len) return LLCOMP_MI_OK;
    if (payload_cap < p.payload_bytes || len_cap < p.n_slices) return LLCOMP_MI_OUTPUT_OVERFLOW;
    regions_gather_copy(p, data, payload, slice_len, nullptr);
    return LLCOMP_MI_OK;
}

int llcomp_mi_replace_slices(const uint8_t* data, size_t len, const uint32_t box[4], const uint32_t* new_len, const uint8_t* new_payload,
                             uint8_t** out, size_t* out_len) {
    if (!out || !out_len) return LLCOMP_MI_BAD_ARGS;
    uint8_t* o = nullptr;
    size_t n = 0;
    if (int rc = replace_slices_common(data, len, box, new_len, new_payload, nullptr, 0, &o, &n)) return rc;
    *out = o;
    *out_len = n;
    return LLCOMP_MI_OK;
}

int llcomp_mi_replace_slices_into(const uint8_t* data, size_t len, const uint32_t box[4], const uint32_t* new_len, const uint8_t* new_payload,
                                  uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!out || !out_len) return LLCOMP_MI_BAD_ARGS;
    return replace_slices_common(data, len, box, new_len, new_payload, out, out_cap, nullptr, out_len);
}

int llcomp_mi_probe(const uint8_t* data, size_t len, llcomp_mi_info* info) {
    if (!data || !info) return LLCOMP_MI_BAD_ARGS;
    std::memset(info, 0, sizeof(*info));
    if (len < 1) return LLCOMP_MI_TRUNCATED;
    if (data[0] == LLCOMP_MI_MAGIC_LEGACY) {
        if (len < 6) return LLCOMP_MI_TRUNCATED;  // reference reads these bytes unchecked (D5)
        info->format = LLCOMP_MI_FORMAT_LEGACY;
        info->channels = data[1];
        info->width = uint32_t(data[2]) | (uint32_t(data[3]) << 8);
        info->height = uint32_t(data[4]) | (uint32_t(data[5]) << 8);
        info->tile_w = info->width;
        info->tile_h = info->height;
        info->planar = 0;
        info->n_slices = 1;
        info->table_offset = 0;
        info->payload_offset = 6;
        return LLCOMP_MI_OK;
    }
    if (data[0] == LLCOMP_MI_MAGIC_SLICED) {
        if (len < LLCOMP_MI_SLICED_HEADER_BYTES) return LLCOMP_MI_TRUNCATED;
        if (data[1] != 1) return LLCOMP_MI_BAD_ARGS;
        info->format = LLCOMP_MI_FORMAT_SLICED;
        info->channels = data[2];
        if (data[3] & ~3u) return LLCOMP_MI_BAD_ARGS;  // unknown flag bits
        info->planar = data[3] & 1;
        info->small_model = (data[3] >> 1) & 1;
        info->width = get_u32le(data + 4);
        info->height = get_u32le(data + 8);
        info->tile_w = get_u32le(data + 12);
        info->tile_h = get_u32le(data + 16);
        info->n_slices = get_u32le(data + 20);
        Geometry g;
        if (info->tile_w == 0 || info->tile_h == 0 || info->tile_w > info->width || info->tile_h > info->height ||
            !make_geometry(g, 1, info->width, info->height, info->channels, info->tile_w, info->tile_h, info->planar) ||
            g.slices_per_frame != info->n_slices)
            return LLCOMP_MI_BAD_ARGS;
        info->table_offset = LLCOMP_MI_SLICED_HEADER_BYTES;
        info->payload_offset = uint64_t(LLCOMP_MI_SLICED_HEADER_BYTES) + 4ull * info->n_slices;
        if (len < info->payload_offset) return LLCOMP_MI_TRUNCATED;
        return LLCOMP_MI_OK;
    }
    return LLCOMP_MI_BAD_MAGIC;
}

int llcomp_mi_merge_bands(const uint8_t* const* bands, const size_t* band_lens, uint32_t n_bands, uint8_t** out,
                          size_t* out_len) {
    if (!bands || !band_lens || !n_bands || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    *out = nullptr;
    *out_len = 0;
    std::vector<llcomp_mi_info> infos(n_bands);
    uint64_t height = 0, n_slices = 0, payload = 0;
    for (uint32_t i = 0; i < n_bands; ++i) {
        if (int rc = llcomp_mi_probe(bands[i], band_lens[i], &infos[i])) return rc;
        const llcomp_mi_info& a = infos[i];
        const llcomp_mi_info& f = infos[0];
        if (a.format != LLCOMP_MI_FORMAT_SLICED) return LLCOMP_MI_BAD_ARGS;
        if (a.width != f.width || a.channels != f.channels || a.planar != f.planar || a.tile_w != f.tile_w || a.small_model != f.small_model)
            return LLCOMP_MI_BAD_ARGS;
        // every band but the last must be whole tile rows of the common tile height; the last may be shorter
        // (then its own tile_h was clamped to its height)
        if (i + 1 < n_bands) {
            if (a.tile_h != f.tile_h || a.height % f.tile_h != 0) return LLCOMP_MI_BAD_ARGS;
        } else if (a.tile_h != f.tile_h && !(a.height < f.tile_h && a.tile_h == a.height)) {
            return LLCOMP_MI_BAD_ARGS;
        }
        uint64_t sum = 0;
        for (uint32_t s = 0; s < a.n_slices; ++s) sum += get_u32le(bands[i] + a.table_offset + 4ull * s);
        if (a.payload_offset + sum > band_lens[i]) return LLCOMP_MI_TRUNCATED;
        height += a.height;
        n_slices += a.n_slices;
        payload += sum;
    }
    if (height >= (1ull << 31) || n_slices >= (1ull << 31)) return LLCOMP_MI_OUT_OF_RANGE;
    Geometry g;
    if (!make_geometry(g, 1, infos[0].width, uint32_t(height), infos[0].channels, infos[0].tile_w, infos[0].tile_h,
                       infos[0].planar, Tuning{}, infos[0].small_model != 0) ||
        g.slices_per_frame != n_slices)
        return LLCOMP_MI_BAD_ARGS;
    const size_t head = LLCOMP_MI_SLICED_HEADER_BYTES + 4 * size_t(n_slices);
    uint8_t* o = static_cast<uint8_t*>(std::malloc(head + payload + 1));
    if (!o) return LLCOMP_MI_NOMEM;
    write_sliced_header(o, g);
    uint8_t* tab = o + LLCOMP_MI_SLICED_HEADER_BYTES;
    uint8_t* pay = o + head;
    for (uint32_t i = 0; i < n_bands; ++i) {
        const llcomp_mi_info& a = infos[i];
        std::memcpy(tab, bands[i] + a.table_offset, 4 * size_t(a.n_slices));
        tab += 4 * size_t(a.n_slices);
        uint64_t sum = 0;
        for (uint32_t s = 0; s < a.n_slices; ++s) sum += get_u32le(bands[i] + a.table_offset + 4ull * s);
        std::memcpy(pay, bands[i] + a.payload_offset, sum);
        pay += sum;
    }
    *out = o;
    *out_len = head + payload;
    return LLCOMP_MI_OK;
}

int llcomp_mi_split_band(const uint8_t* data, size_t len, uint32_t tile_row0, uint32_t tile_row1, uint8_t** out,
                         size_t* out_len) {
    if (!data || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    *out = nullptr;
    *out_len = 0;
    llcomp_mi_info a;
    if (int rc = llcomp_mi_probe(data, len, &a)) return rc;
    if (a.format != LLCOMP_MI_FORMAT_SLICED) return LLCOMP_MI_BAD_ARGS;
    const uint32_t nty = (a.height + a.tile_h - 1) / a.tile_h;
    if (tile_row0 >= tile_row1 || tile_row1 > nty) return LLCOMP_MI_BAD_ARGS;
    const uint32_t per_row = a.n_slices / nty;  // slices per tile row
    const uint32_t s0 = tile_row0 * per_row, s1 = tile_row1 * per_row;
    uint64_t before = 0, inside = 0;
    for (uint32_t s = 0; s < s1; ++s) {
        const uint64_t l = get_u32le(data + a.table_offset + 4ull * s);
        (s < s0 ? before : inside) += l;
    }
    if (a.payload_offset + before + inside > len) return LLCOMP_MI_TRUNCATED;
    const uint32_t y0 = tile_row0 * a.tile_h;
    const uint32_t y1 = tile_row1 * a.tile_h < a.height ? tile_row1 * a.tile_h : a.height;
    Geometry g;
    const uint32_t band_h = y1 - y0;
    if (!make_geometry(g, 1, a.width, band_h, a.channels, a.tile_w, a.tile_h < band_h ? a.tile_h : band_h, a.planar, Tuning{}, a.small_model != 0) ||
        g.slices_per_frame != s1 - s0)
        return LLCOMP_MI_BAD_ARGS;
    const size_t head = LLCOMP_MI_SLICED_HEADER_BYTES + 4 * size_t(s1 - s0);
    uint8_t* o = static_cast<uint8_t*>(std::malloc(head + inside + 1));
    if (!o) return LLCOMP_MI_NOMEM;
    write_sliced_header(o, g);
    std::memcpy(o + LLCOMP_MI_SLICED_HEADER_BYTES, data + a.table_offset + 4ull * s0, 4 * size_t(s1 - s0));
    std::memcpy(o + head, data + a.payload_offset + before, inside);
    *out = o;
    *out_len = head + inside;
    return LLCOMP_MI_OK;
}

}  // extern "C"
