// photo_plan.cpp -- the host planner of the photometric chains (photo_plan.hpp) and llcomp_mi_photo_reference.  Plain C++, no GPU.
#include "photo_plan.hpp"

#include <algorithm>
#include <cstring>

#include "photo_rule.hpp"

namespace llcomp_mi {

uint64_t photo_tables_bound(uint64_t total_views) { return 16 + std::max<uint64_t>(total_views, 1) * sizeof(llcomp_mi_photo_chain); }

void PhotoTail::put(uint8_t* at) const {
    if (!chains.empty()) std::memcpy(at, chains.data(), chains.size() * sizeof(llcomp_mi_photo_chain));
}

int photo_check_chain(const llcomp_mi_photo_chain& ch, uint32_t c) {
    if (ch.n_ops > LLCOMP_MI_PHOTO_MAX_OPS) return LLCOMP_MI_BAD_ARGS;
    if (ch.n_ops && c != 1 && c != 3) return LLCOMP_MI_BAD_ARGS;
    for (uint32_t k = 0; k < ch.n_ops; ++k)
        if (!photo_op_ok(ch.ops[k].op, ch.ops[k].param)) return LLCOMP_MI_BAD_ARGS;
    return LLCOMP_MI_OK;
}

uint32_t photo_sharp_band_rows(uint32_t ow, uint32_t oh, uint32_t c, uint64_t samples) {
    const uint64_t pitch = uint64_t(ow) * c, view = pitch * oh;
    if (ow < 3 || oh < 3) return oh;  // (the identity: nothing reads a neighbour)
    uint32_t rows = std::min(oh, kSharpBandRows);
    if (view + photo_sharp_halo_bytes(ow, oh, c, rows) > samples) {
        // the most bands whose halos still fit beside the view, one where the view alone fills the bound or exceeds it
        const uint64_t bands = view < samples ? 1 + (samples - view) / (2 * pitch) : 1;
        rows = uint32_t((oh + bands - 1) / bands);  // (bands <= oh / kSharpBandRows here, so rows >= kSharpBandRows)
    }
    if (pitch > kSharpRowBytes) rows = std::min(rows, kSharpKeepRows);
    return rows;
}

int photo_setup(uint32_t c, uint64_t samples, const llcomp_mi_photo_group* photo, uint32_t n_groups, const uint32_t* n_views, const uint32_t* ow,
                const uint32_t* oh, PhotoTail& t) {
    t = PhotoTail{};
    t.groups.resize(n_groups);
    if (!photo) return LLCOMP_MI_OK;
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const llcomp_mi_photo_group& pg = photo[gi];
        if (pg.struct_size != sizeof(llcomp_mi_photo_group)) return LLCOMP_MI_BAD_ARGS;
        if (!pg.chains) continue;
        PhotoGroup& g = t.groups[gi];
        for (uint32_t i = 0; i < n_views[gi]; ++i) {
            const llcomp_mi_photo_chain& ch = pg.chains[i];
            if (int rc = photo_check_chain(ch, c)) return rc;
            g.steps = std::max(g.steps, ch.n_ops);
            for (uint32_t k = 0; k < ch.n_ops; ++k) {
                g.step[k].kinds |= 1u << uint32_t(photo_kind(ch.ops[k].op));
                g.step[k].stats |= photo_needs_stats(ch.ops[k].op);
            }
        }
        if (!g.steps) continue;  // (every chain empty: the group takes the extended call's path)
        g.active = true;
        g.n = n_views[gi];
        g.ow = ow[gi];
        g.oh = oh[gi];
        g.first = uint32_t(t.chains.size());
        for (uint32_t i = 0; i < g.n; ++i) {
            llcomp_mi_photo_chain ch;
            std::memset(&ch, 0, sizeof ch);  // (what lies behind a chain's ops does not travel)
            ch.n_ops = pg.chains[i].n_ops;
            std::memcpy(ch.ops, pg.chains[i].ops, ch.n_ops * sizeof(llcomp_mi_photo_op));
            t.chains.push_back(ch);
        }
        const uint64_t view = uint64_t(g.oh) * g.ow * c;
        uint64_t halo = 0;
        if (std::any_of(g.step, g.step + g.steps, [](const PhotoStepInfo& s) { return s.has(PhotoKind::kSharp); })) {  // (every view alike: a chunk is its views, then their halo areas)
            g.sharp_rows = photo_sharp_band_rows(g.ow, g.oh, c, samples);
            halo = photo_sharp_halo_bytes(g.ow, g.oh, c, g.sharp_rows);
        }
        g.chunk = uint32_t(std::min<uint64_t>(g.n, std::max<uint64_t>(samples / std::max<uint64_t>(view + halo, 1), 1)));
        if (halo) g.halo_at = g.chunk * view;
        t.stage_bytes = std::max(t.stage_bytes, g.chunk * (view + halo));
        t.tab_views = std::max<uint64_t>(t.tab_views, g.chunk);
    }
    return LLCOMP_MI_OK;
}

namespace {
// One box pass over the line p[0], p[stride], ..., p[(n - 1) * stride], in place through tmp[n]
void blur_line(uint8_t* p, uint32_t n, uint64_t stride, uint32_t r, uint32_t ww, uint32_t fw, uint8_t* tmp) {
    const int64_t last = int64_t(n) - 1;
    auto at = [&](int64_t i) -> uint32_t { return p[uint64_t(i < 0 ? 0 : (i > last ? last : i)) * stride]; };
    for (int64_t x = 0; x <= last; ++x) {
        uint32_t acc = 0;
        for (int64_t k = -int64_t(r); k <= int64_t(r); ++k) acc += at(x + k);
        tmp[x] = uint8_t(photo_blur_tap(acc, at(x - int64_t(r) - 1) + at(x + int64_t(r) + 1), ww, fw));
    }
    for (int64_t x = 0; x <= last; ++x) p[uint64_t(x) * stride] = tmp[x];
}
}  // namespace

int photo_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_photo_op* ops, uint32_t n_ops, uint8_t* out) {
    if (!src || !out || !w || !h || (c != 1 && c != 3) || (n_ops && !ops) || n_ops > LLCOMP_MI_PHOTO_MAX_OPS) return LLCOMP_MI_BAD_ARGS;
    for (uint32_t k = 0; k < n_ops; ++k)
        if (!photo_op_ok(ops[k].op, ops[k].param)) return LLCOMP_MI_BAD_ARGS;
    const uint64_t n = uint64_t(w) * h;
    if (out != src) std::memmove(out, src, size_t(n * c));
    std::vector<uint32_t> hist(size_t(256) * c);
    std::vector<uint8_t> line, before;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t op = ops[k].op;
        const float a = ops[k].param;
        switch (photo_kind(op)) {
            case PhotoKind::kBlur: {
                uint32_t r, ww, fw;
                photo_blur_weights(a, r, ww, fw);
                line.resize(std::max(w, h));
                for (int pass = 0; pass < 3; ++pass)  // along every row
                    for (uint64_t y = 0; y < h; ++y)
                        for (uint32_t ch = 0; ch < c; ++ch) blur_line(out + y * w * c + ch, w, c, r, ww, fw, line.data());
                for (int pass = 0; pass < 3; ++pass)  // along every column
                    for (uint64_t x = 0; x < w; ++x)
                        for (uint32_t ch = 0; ch < c; ++ch) blur_line(out + x * c + ch, h, uint64_t(w) * c, r, ww, fw, line.data());
                break;
            }
            case PhotoKind::kSharp: {  // every sample from the view as it stands before the op: a copy of it
                before.assign(out, out + size_t(n * c));
                const uint64_t pitch = uint64_t(w) * c;
                for (uint64_t y = 0; y < h; ++y)
                    for (uint64_t x = 0; x < w; ++x)
                        for (uint32_t ch = 0; ch < c; ++ch) {
                            const uint8_t* const p = before.data() + y * pitch + x * c + ch;
                            uint32_t d = *p;
                            if (photo_smooth_interior(x, y, w, h)) {
                                uint32_t sum9 = 0;
                                for (int dy = -1; dy <= 1; ++dy)
                                    for (int dx = -1; dx <= 1; ++dx) sum9 += p[int64_t(dy) * int64_t(pitch) + dx * int64_t(c)];
                                d = photo_smooth(sum9, *p);
                            }
                            out[y * pitch + x * c + ch] = uint8_t(photo_blend(d, *p, a));
                        }
                break;
            }
            case PhotoKind::kPixel: {  // (one channel: nothing to mix)
                if (c != 3) break;
                const uint32_t shift = op == LLCOMP_MI_PHOTO_ADJUST_HUE ? photo_hue_shift(a) : 0u;
                for (uint64_t i = 0; i < n; ++i) {
                    uint8_t* p = out + 3 * i;
                    uint32_t r = p[0], g = p[1], b = p[2];
                    photo_pixel(op, a, shift, r, g, b);
                    p[0] = uint8_t(r);
                    p[1] = uint8_t(g);
                    p[2] = uint8_t(b);
                }
                break;
            }
            case PhotoKind::kTable: {
                uint64_t sum_l = 0;
                if (photo_needs_stats(op)) {
                    std::fill(hist.begin(), hist.end(), 0u);
                    for (uint64_t i = 0; i < n; ++i) {
                        const uint8_t* p = out + c * i;
                        for (uint32_t ch = 0; ch < c; ++ch) ++hist[256 * ch + p[ch]];
                        sum_l += c == 3 ? photo_luma(p[0], p[1], p[2]) : p[0];
                    }
                }
                uint8_t lut[3][256];
                for (uint32_t ch = 0; ch < c; ++ch) photo_table(op, a, hist.data() + 256 * ch, sum_l, n, lut[ch]);
                for (uint64_t i = 0; i < n; ++i)
                    for (uint32_t ch = 0; ch < c; ++ch) out[c * i + ch] = lut[ch][out[c * i + ch]];
                break;
            }
        }
    }
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

extern "C" int llcomp_mi_photo_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_photo_op* ops, uint32_t n_ops,
                                         uint8_t* out) {
    return llcomp_mi::photo_reference(src, w, h, c, ops, n_ops, out);
}
