// photo_kernels.hip -- the kernels of the photometric chains (llcomp_mi_codec_decode_photo_views / _photo_warped_views): the
// statistics of every view whose op of the step reads them, and the kernels of each kind of op (photo_rule.hpp: PhotoKind) -- the table
// of every view whose op is one and the per-pixel pass, the row and the column kernel of the blur, the band kernel of the sharpness.  A
// view takes part in a step as the kind of its op (photo_step_as); what a step launches is its PhotoStep's (photo.hpp).  All views of a
// chunk run a step together; nothing goes back to the host in between.  The arithmetic is photo_rule.hpp's -- the functions
// llcomp_mi_photo_reference runs on the host -- with NO fused multiply-add: the header's pragma holds for this whole file.
#include "photo_rule.hpp"

#include "out_store.hpp"
#include "photo.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace llcomp_mi {

namespace {

constexpr uint32_t kPhotoNoOp = 0xFFFFFFFFu;  // the step of an empty chain: the view goes to the output as it is

// Does the view of chain `ch` take part in `step` as `kind` (or as `also`: the per-pixel pass takes two), and if so with which op and
// parameter, and is the step its chain's last?  False where the chain has ended or its op is of another kind: every kernel asks for
// its own, so a view is one kernel family's in a step.  An empty chain has one step, step 0, which only writes the output: kPhotoNoOp
// is no op code, so it is of kPixel (photo_rule.hpp), for which k_photo_apply alone asks.
struct PhotoPart { uint32_t op; float param; bool last; };
__device__ __forceinline__ bool photo_step_as(const llcomp_mi_photo_chain& ch, uint32_t step, PhotoKind kind, PhotoPart& me, PhotoKind also = PhotoKind(~0u)) {
    const uint32_t n = ch.n_ops < LLCOMP_MI_PHOTO_MAX_OPS ? ch.n_ops : uint32_t(LLCOMP_MI_PHOTO_MAX_OPS);
    if (step >= (n ? n : 1u)) return false;
    me.op = n ? ch.ops[step].op : kPhotoNoOp;
    me.param = n ? ch.ops[step].param : 0.0f;
    me.last = step + 1 >= n;
    return photo_kind(me.op) == kind || photo_kind(me.op) == also;
}

// N result bytes of view v, val[0 .. N): the chain's last step stores them through the group's output format to o (out_store.hpp:
// channels ch .. ch + N - 1 of pixel px, plane = oh * ow), any other step back in place at back[0 .. N).
template <class T, bool CHW, bool LUT, int N = 1>
__device__ __forceinline__ void photo_store(bool last, T* o, const T* lut, size_t v, uint32_t c, size_t plane, size_t px, uint32_t ch, uint8_t* back,
                                            const uint32_t* val) {
    if (last)
        for (int k = 0; k < N; ++k) out_store<T, CHW, LUT>(o, lut, v, c, plane, px, ch + k, val[k]);
    else
        for (int k = 0; k < N; ++k) back[k] = uint8_t(val[k]);
}

// Statistics: blockIdx.y the view, gridDim.x workgroups share its pixels.  Each wavefront counts into a histogram of its own in LDS
// (LDS atomics; four copies keep the four wavefronts of a constant image off one counter), the workgroup adds the four into the view's
// histogram in HBM -- only the bins it has seen -- and its sum of L into the view's u64, with integer atomics: no order changes the
// result.  CONTRAST reads the sum alone and skips the histograms.
template <int C>
__global__ __launch_bounds__(256) void k_photo_stats(const uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                     uint8_t* __restrict__ stats, uint64_t npix, uint32_t step) {
    __shared__ uint32_t s_hist[4][C * 256];
    __shared__ unsigned long long s_sum;
    const uint32_t v = blockIdx.y;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kTable, me) || !photo_needs_stats(me.op)) return;  // (the whole workgroup alike)
    const bool hist = me.op != LLCOMP_MI_PHOTO_CONTRAST;
    for (uint32_t j = threadIdx.x; j < uint32_t(4 * C * 256); j += 256) (&s_hist[0][0])[j] = 0;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint8_t* p = px + size_t(v) * npix * C;
    uint32_t* h = s_hist[threadIdx.x >> 6];
    unsigned long long sum = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < npix; i += uint64_t(gridDim.x) * 256) {
        if constexpr (C == 3) {
            const uint32_t r = p[3 * i], g = p[3 * i + 1], b = p[3 * i + 2];
            sum += photo_luma(r, g, b);
            if (hist) {
                atomicAdd(&h[r], 1u);
                atomicAdd(&h[256 + g], 1u);
                atomicAdd(&h[512 + b], 1u);
            }
        } else {
            const uint32_t s = p[i];
            sum += s;
            if (hist) atomicAdd(&h[s], 1u);
        }
    }
    if (sum) atomicAdd(&s_sum, sum);
    __syncthreads();
    unsigned long long* g_sum = reinterpret_cast<unsigned long long*>(stats + size_t(v) * (8 + 1024 * C));
    uint32_t* g_hist = reinterpret_cast<uint32_t*>(g_sum + 1);
    if (hist)
        for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 256) {
            const uint32_t t = s_hist[0][j] + s_hist[1][j] + s_hist[2][j] + s_hist[3][j];
            if (t) atomicAdd(&g_hist[j], t);
        }
    if (threadIdx.x == 0 && s_sum) atomicAdd(g_sum, s_sum);
}

// Tables: one wavefront per view.  The view's histograms come to LDS, thread ch builds channel ch's table with photo_table -- the very
// function of the host's reference, binary64 where the rule says so -- and the wavefront stores the view's [C][256] bytes.
template <int C>
__global__ __launch_bounds__(64) void k_photo_lut(const llcomp_mi_photo_chain* __restrict__ chains, const uint8_t* __restrict__ stats,
                                                  uint8_t* __restrict__ luts, uint64_t npix, uint32_t step) {
    __shared__ uint32_t s_hist[C * 256];
    __shared__ uint8_t s_lut[C * 256];
    const uint32_t v = blockIdx.x;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kTable, me)) return;
    const bool need = photo_needs_stats(me.op);
    const unsigned long long* g_sum = reinterpret_cast<const unsigned long long*>(stats + size_t(v) * (8 + 1024 * C));
    const uint32_t* g_hist = reinterpret_cast<const uint32_t*>(g_sum + 1);
    for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 64) s_hist[j] = need ? g_hist[j] : 0u;
    __syncthreads();
    if (threadIdx.x < uint32_t(C)) photo_table(me.op, me.param, s_hist + 256 * threadIdx.x, need ? uint64_t(*g_sum) : 0ull, npix, s_lut + 256 * threadIdx.x);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 64) luts[size_t(v) * (C * 256) + j] = s_lut[j];
}

// The per-pixel pass: blockIdx.y the view, a workgroup takes 1024 of its pixels.  A table op looks every channel up in the view's table
// (copied to LDS), an op of kPixel is computed from the pixel (photo_pixel), the step of an empty chain changes nothing, and a view
// whose op is of another kind sits out: the blur's or the sharpness's kernels run it.  The value goes back in place, or -- the chain's
// last step -- through the group's output format to `out` (photo_store).  E, CHW, LUT as in the gather of the warped views.
template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_photo_apply(uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                     const uint8_t* __restrict__ luts, const void* __restrict__ table, void* __restrict__ out,
                                                     uint64_t npix, uint32_t step) {
    using T = typename OutElem<E>::T;
    __shared__ uint8_t s_lut[C * 256];
    const uint32_t v = blockIdx.y;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kPixel, me, PhotoKind::kTable)) return;  // (the whole workgroup alike)
    const bool tab = photo_kind(me.op) == PhotoKind::kTable;
    const uint32_t shift = me.op == LLCOMP_MI_PHOTO_ADJUST_HUE ? photo_hue_shift(me.param) : 0u;
    if (tab) {
        for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 256) s_lut[j] = luts[size_t(v) * (C * 256) + j];
        __syncthreads();
    }
    uint8_t* const p = px + size_t(v) * npix * C;
    T* const o = static_cast<T*>(out);
    const T* const lut = static_cast<const T*>(table);
    const uint64_t base = uint64_t(blockIdx.x) * 1024, end = base + 1024 < npix ? base + 1024 : npix;
    for (uint64_t i = base + threadIdx.x; i < end; i += 256) {
        uint32_t s[C];
        for (int ch = 0; ch < C; ++ch) s[ch] = p[i * C + ch];
        if (tab) {
            for (int ch = 0; ch < C; ++ch) s[ch] = s_lut[ch * 256 + s[ch]];
        } else if constexpr (C == 3) {
            photo_pixel(me.op, me.param, shift, s[0], s[1], s[2]);
        }
        photo_store<T, CHW, LUT, C>(me.last, o, lut, v, C, npix, i, 0, p + i * C, s);
    }
}

// The blur (LLCOMP_MI_PHOTO_GAUSSIAN_BLUR): three box passes along every row, then three along every column, each kernel with its
// three passes inside LDS and IN PLACE on px -- lines of one direction do not read each other.  A line, or a piece of one, lies in
// LDS with at most kBlurLine samples.  A longer line is done in pieces of kBlurSeg output samples, one after the other by the same
// workgroup: a piece is loaded with photo_blur_reach(r) <= kBlurHalo samples to each side, every pass clamps its taps to the piece, so
// that what a cut end spoils -- r + 1 samples per pass -- stays inside the halo, and a true end of the line is clamped as the rule
// says.  The samples the piece's store overwrites, and the next pieces still have to read as they were, stay behind in s_keep.
constexpr uint32_t kBlurLine = 256;                        // samples of a line in LDS, halo included
constexpr uint32_t kBlurHalo = 3 * (LLCOMP_MI_PHOTO_MAX_RADIUS + 1);  // 99
constexpr uint32_t kBlurSeg = kBlurLine - 2 * kBlurHalo;   // 58
constexpr uint32_t kBlurRowSlots = 1024;                   // pixels of the row kernel's tile: as many rows (pieces) as fit
constexpr uint32_t kBlurStrip = 32;                        // byte columns of the column kernel's tile
static_assert(kBlurSeg >= 1 && kBlurRowSlots % kBlurLine == 0 && kBlurStrip % 4 == 0, "the blur's tiles");

// the pieces of a line of n samples: their count, and piece `seg` as outputs [s, e) inside loaded samples [lo, hi)
__host__ __device__ inline uint32_t blur_pieces(uint32_t n) { return n <= kBlurLine ? 1u : (n + kBlurSeg - 1) / kBlurSeg; }
__device__ __forceinline__ void blur_piece(uint32_t n, uint32_t seg, uint32_t reach, uint32_t& s, uint32_t& e, uint32_t& lo, uint32_t& hi) {
    if (n <= kBlurLine) {
        s = lo = 0;
        e = hi = n;
        return;
    }
    s = seg * kBlurSeg;
    e = s + kBlurSeg < n ? s + kBlurSeg : n;
    lo = s > reach ? s - reach : 0u;
    hi = n - e > reach ? e + reach : n;
}
// rows of a view the row kernel's workgroup takes: as many as fit, a multiple of its four wavefronts
__host__ __device__ inline uint32_t blur_rows_per_group(uint32_t ow) { return (kBlurRowSlots / (ow < kBlurLine ? ow : kBlurLine)) & ~3u; }

// Rows: blockIdx.y the view, a workgroup takes blur_rows_per_group(ow) whole rows of it, wavefront w the rows w, w + 4, ...  Lane per
// byte: byte b of a row's piece is channel b % C of sample b / C, and its taps lie C bytes apart.
template <int C>
__global__ __launch_bounds__(256) void k_photo_blur_rows(uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains, uint32_t ow,
                                                         uint32_t oh, uint32_t step) {
    __shared__ uint8_t s_a[kBlurRowSlots * C], s_b[kBlurRowSlots * C], s_keep[(kBlurRowSlots / kBlurLine) * kBlurHalo * C];
    const uint32_t v = blockIdx.y;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kBlur, me)) return;  // (the whole workgroup alike)
    uint32_t r, ww, fw;
    photo_blur_weights(me.param, r, ww, fw);
    const uint32_t reach = photo_blur_reach(r);
    const uint32_t rows = blur_rows_per_group(ow), row0 = blockIdx.x * rows;
    const uint32_t nrows = oh - row0 < rows ? oh - row0 : rows;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t pitch = size_t(ow) * C;
    uint8_t* const p = px + (size_t(v) * oh + row0) * pitch;
    const uint32_t pieces = blur_pieces(ow);
    for (uint32_t seg = 0; seg < pieces; ++seg) {
        uint32_t s, e, lo, hi;
        blur_piece(ow, seg, reach, s, e, lo, hi);
        const uint32_t len = hi - lo, lb = len * C;  // (len <= kBlurLine, nrows * len <= kBlurRowSlots)
        const uint32_t kb = (s - lo) * C;            // bytes of a row that come from s_keep
        for (uint32_t row = wave; row < nrows; row += 4)
            for (uint32_t b = lane; b < lb; b += 64)
                s_a[row * lb + b] = seg && b < kb ? s_keep[row * (kBlurHalo * C) + b] : p[row * pitch + size_t(lo) * C + b];
        __syncthreads();
        if (seg + 1 < pieces) {  // what the next piece reads below its own outputs: [e - reach, e) as it is now
            const uint32_t klo = e > reach ? e - reach : 0u, kl = (e - klo) * C;
            for (uint32_t row = wave; row < nrows; row += 4)
                for (uint32_t b = lane; b < kl; b += 64) s_keep[row * (kBlurHalo * C) + b] = s_a[row * lb + (klo - lo) * C + b];
        }
        for (int pass = 0; pass < 3; ++pass) {
            const uint8_t* const src = pass == 1 ? s_b : s_a;
            uint8_t* const dst = pass == 1 ? s_a : s_b;
            for (uint32_t row = wave; row < nrows; row += 4)
                for (uint32_t b = lane; b < lb; b += 64) {
                    const int32_t x = int32_t(b / C), ch = int32_t(b) - x * C, top = int32_t(len) - 1;
                    const uint8_t* const line = src + row * lb + ch;
                    uint32_t acc = 0;
                    for (int32_t k = x - int32_t(r); k <= x + int32_t(r); ++k) acc += line[(k < 0 ? 0 : (k > top ? top : k)) * C];
                    const int32_t fl = x - int32_t(r) - 1, fh = x + int32_t(r) + 1;
                    const uint32_t far = uint32_t(line[(fl < 0 ? 0 : fl) * C]) + line[(fh > top ? top : fh) * C];
                    dst[row * lb + b] = uint8_t(photo_blur_tap(acc, far, ww, fw));
                }
            __syncthreads();
        }
        const uint32_t ob = (e - s) * C;
        for (uint32_t row = wave; row < nrows; row += 4)
            for (uint32_t b = lane; b < ob; b += 64) p[row * pitch + size_t(s) * C + b] = s_b[row * lb + kb + b];
    }
}

// Columns: blockIdx.y the view, a workgroup takes a strip of kBlurStrip adjacent byte columns of it -- one row of the strip is one
// contiguous run of bytes in HBM -- held as [rows][kBlurStrip] in LDS.  In the passes a thread takes FOUR adjacent columns as one
// dword: a wavefront reads 64 consecutive dwords (eight rows of the strip), every bank once in each half, where a thread per byte
// column would read a byte per lane.  The four sums ride in two registers as 16-bit fields (67 samples of 255 at most).  The strip is
// narrow because a view has few of them and a workgroup walks its strip's whole height: 32 columns gave 25 us per launch where 64
// gave 38 (DESIGN.md "Blur and hue").  The chain's last step stores through the group's output table and layout to `out`
// (out_store.hpp), as k_photo_apply does; E, CHW, LUT as there.
template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_photo_blur_cols(uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                         const void* __restrict__ table, void* __restrict__ out, uint32_t ow, uint32_t oh,
                                                         uint32_t step) {
    using T = typename OutElem<E>::T;
    constexpr uint32_t W4 = kBlurStrip / 4;
    __shared__ uint32_t s_a[kBlurLine * W4], s_b[kBlurLine * W4], s_keep[kBlurHalo * W4];
    const uint32_t v = blockIdx.y;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kBlur, me)) return;  // (the whole workgroup alike)
    uint32_t r, ww, fw;
    photo_blur_weights(me.param, r, ww, fw);
    const uint32_t reach = photo_blur_reach(r);
    const size_t pitch = size_t(ow) * C, plane = size_t(oh) * ow;
    const size_t col0 = size_t(blockIdx.x) * kBlurStrip;
    const uint32_t sw = pitch - col0 < kBlurStrip ? uint32_t(pitch - col0) : kBlurStrip;  // the strip's byte columns
    uint8_t* const p = px + size_t(v) * plane * C + col0;
    uint8_t* const a8 = reinterpret_cast<uint8_t*>(s_a);
    uint8_t* const k8 = reinterpret_cast<uint8_t*>(s_keep);
    const uint8_t* const b8 = reinterpret_cast<const uint8_t*>(s_b);
    T* const o = static_cast<T*>(out);
    const T* const lut = static_cast<const T*>(table);
    const uint32_t pieces = blur_pieces(oh);
    for (uint32_t seg = 0; seg < pieces; ++seg) {
        uint32_t s, e, lo, hi;
        blur_piece(oh, seg, reach, s, e, lo, hi);
        const uint32_t len = hi - lo;  // (<= kBlurLine)
        for (uint32_t j = threadIdx.x; j < len * kBlurStrip; j += 256) {
            const uint32_t row = j / kBlurStrip, col = j % kBlurStrip;
            if (col < sw) a8[j] = seg && lo + row < s ? k8[j] : p[(size_t(lo) + row) * pitch + col];
        }
        __syncthreads();
        if (seg + 1 < pieces) {  // what the next piece reads above its own outputs: rows [e - reach, e) as they are now
            const uint32_t klo = e > reach ? e - reach : 0u;
            for (uint32_t j = threadIdx.x; j < (e - klo) * W4; j += 256) s_keep[j] = s_a[(klo - lo) * W4 + j];
        }
        for (int pass = 0; pass < 3; ++pass) {
            const uint32_t* const src = pass == 1 ? s_b : s_a;
            uint32_t* const dst = pass == 1 ? s_a : s_b;
            for (uint32_t j = threadIdx.x; j < len * W4; j += 256) {
                const int32_t y = int32_t(j / W4), top = int32_t(len) - 1;
                const uint32_t* const line = src + j % W4;
                uint32_t even = 0, odd = 0;  // the sums of bytes 0 and 2, and of bytes 1 and 3, as two 16-bit fields each
                for (int32_t k = y - int32_t(r); k <= y + int32_t(r); ++k) {
                    const uint32_t d = line[(k < 0 ? 0 : (k > top ? top : k)) * W4];
                    even += d & 0x00FF00FFu;
                    odd += (d >> 8) & 0x00FF00FFu;
                }
                const int32_t fl = y - int32_t(r) - 1, fh = y + int32_t(r) + 1;
                const uint32_t d0 = line[(fl < 0 ? 0 : fl) * W4], d1 = line[(fh > top ? top : fh) * W4];
                const uint32_t feven = (d0 & 0x00FF00FFu) + (d1 & 0x00FF00FFu), fodd = ((d0 >> 8) & 0x00FF00FFu) + ((d1 >> 8) & 0x00FF00FFu);
                dst[j] = photo_blur_tap(even & 0xFFFFu, feven & 0xFFFFu, ww, fw) | photo_blur_tap(odd & 0xFFFFu, fodd & 0xFFFFu, ww, fw) << 8 |
                         photo_blur_tap(even >> 16, feven >> 16, ww, fw) << 16 | photo_blur_tap(odd >> 16, fodd >> 16, ww, fw) << 24;
            }
            __syncthreads();
        }
        for (uint32_t j = threadIdx.x; j < (e - s) * kBlurStrip; j += 256) {
            const uint32_t row = j / kBlurStrip, col = j % kBlurStrip;
            if (col >= sw) continue;
            const uint32_t val = b8[(s - lo + row) * kBlurStrip + col];
            const size_t bx = col0 + col, x = bx / C;
            photo_store<T, CHW, LUT>(me.last, o, lut, v, C, plane, (size_t(s) + row) * ow + x, uint32_t(bx - x * C), p + (size_t(s) + row) * pitch + col, &val);
        }
    }
}

// The sharpness (LLCOMP_MI_PHOTO_ADJUST_SHARPNESS): an output sample reads its eight neighbours as they were BEFORE the op, and the op
// runs in place on px, so no sample may be written while another workgroup still has to read it.  A workgroup therefore owns a BAND of
// band_rows whole rows of one view -- no edge between workgroups inside a row -- and the two rows a band reads outside itself, the one
// above its first and the one below its last, are saved as they stand by k_photo_sharp_save, a launch before this one, into the
// view's halo area: rows (j + 1) * band_rows - 1 and (j + 1) * band_rows, which lie next to each other in px, for every pair of
// neighbouring bands j, j + 1.  A band reads px only inside its own rows, and the halo area is not written after the save.
//   The workgroup walks down its band with a ring of kSharpSlots original rows in LDS: load row y + 1, barrier, compute row y from
// rows y - 1, y, y + 1 of the ring, store row y.  With four slots the load of row y + 1 overwrites row y - 3, and a wavefront that
// is still behind the barrier before computes row y - 1 from rows y - 2 .. y: one barrier a row is enough (three slots would need
// two).  Lane per byte, taps C bytes apart, integers (photo_smooth).  A row comes
// into its slot by dwords between the first and the last aligned address of its span in HBM and by bytes before and after; the slot
// keeps the address's low two bits, so that byte q of the span lies at q + (address & 3): the three rows of a window may differ in it.
//   A row longer than kSharpRowBytes is walked in column PIECES of that many bytes, one after the other by the same workgroup, each
// loaded with C more bytes to each side.  The piece to the left has overwritten the C bytes a piece reads left of itself: those stay
// behind in LDS for every row of the band (s_keep; photo_plan.hpp caps such a band at kSharpKeepRows), the halo rows are read again
// from the halo area.  The chain's last step stores through the group's output table and layout to `out` (out_store.hpp); E, CHW,
// LUT as in k_photo_apply.  The thresholds -- kSharpBandRows, kSharpRowBytes, kSharpKeepRows -- are photo_plan.hpp's, because the
// planner charges the halo areas to the staging buffer by them.
constexpr uint32_t kSharpSlots = 4;
// the bytes of a ring slot: a row's span with C bytes to each side and up to 3 of misalignment, in whole 16s
__host__ __device__ inline uint32_t sharp_slot_bytes(uint64_t pitch) {
    return (uint32_t(pitch < kSharpRowBytes ? pitch : kSharpRowBytes) + 2u * 3u + 3u + 15u) & ~15u;
}
__host__ __device__ inline uint64_t sharp_pieces(uint64_t pitch) { return pitch <= kSharpRowBytes ? 1 : (pitch + kSharpRowBytes - 1) / kSharpRowBytes; }
static_assert(kSharpSlots * ((kSharpRowBytes + 24u) & ~15u) + kSharpKeepRows * 3u <= 65536u, "the ring and the kept columns in 64 KiB of LDS");

template <int C>
__global__ __launch_bounds__(256) void k_photo_sharp_save(const uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                          uint8_t* __restrict__ halo, uint32_t ow, uint32_t oh, uint32_t band_rows,
                                                          uint64_t halo_stride, uint32_t step) {
    const uint32_t v = blockIdx.y, j = blockIdx.x;  // the pair of rows between bands j and j + 1
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kSharp, me)) return;  // (the whole workgroup alike)
    const size_t pitch = size_t(ow) * C;
    const uint8_t* const src = px + (size_t(v) * oh + (size_t(j) + 1) * band_rows - 1) * pitch;
    uint8_t* const dst = halo + size_t(v) * halo_stride + size_t(j) * 2 * pitch;
    for (size_t b = threadIdx.x; b < 2 * pitch; b += 256) dst[b] = src[b];
}

template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_photo_sharp(uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                     const uint8_t* __restrict__ halo, const void* __restrict__ table, void* __restrict__ out,
                                                     uint32_t ow, uint32_t oh, uint32_t band_rows, uint64_t halo_stride, uint32_t step) {
    using T = typename OutElem<E>::T;
    extern __shared__ __align__(16) uint8_t s_sharp[];  // kSharpSlots slots, then -- a row in pieces -- band_rows * C kept bytes
    const uint32_t v = blockIdx.y, band = blockIdx.x;
    PhotoPart me;
    if (!photo_step_as(chains[v], step, PhotoKind::kSharp, me)) return;  // (the whole workgroup alike)
    const size_t pitch = size_t(ow) * C, plane = size_t(oh) * ow;
    const uint32_t slot_bytes = sharp_slot_bytes(pitch);
    const uint32_t r0 = band * band_rows, r1 = oh - r0 < band_rows ? oh : r0 + band_rows;
    uint8_t* const p = px + size_t(v) * plane * C;
    const uint8_t* const hv = halo + size_t(v) * halo_stride;
    uint8_t* const s_keep = s_sharp + kSharpSlots * slot_bytes;
    T* const o = static_cast<T*>(out);
    const T* const lut = static_cast<const T*>(table);
    const uint64_t pieces = sharp_pieces(pitch);
    // row yy of r0 - 1 .. r1 as it stood before the op: the band's own from px, the two beside it from the halo area
    auto row_of = [&](uint32_t yy) -> const uint8_t* {
        if (yy + 1 == r0) return hv + (size_t(band) - 1) * 2 * pitch;
        if (yy == r1) return hv + size_t(band) * 2 * pitch + pitch;
        return p + size_t(yy) * pitch;
    };
    for (uint64_t piece = 0; piece < pieces; ++piece) {
        // the piece's outputs are bytes [s, e) of a row, its slot holds [lo, hi)
        const size_t s = size_t(piece) * kSharpRowBytes, e = pitch - s < kSharpRowBytes ? pitch : s + kSharpRowBytes;
        const size_t lo = piece ? s - C : 0, hi = pitch - e < size_t(C) ? pitch : e + C;
        auto fetch = [&](uint32_t yy) {
            const bool own = yy >= r0 && yy < r1;
            const uint8_t* const row = row_of(yy);
            uint8_t* const sl = s_sharp + ((yy + 1 - r0) & (kSharpSlots - 1)) * slot_bytes;
            const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(row + lo) & 3u);
            const size_t q0 = own && piece ? s : lo;  // (px no longer has an own row's bytes left of s as they were)
            const uint8_t* const b = row + q0;
            const uint32_t at = uint32_t(q0 - lo) + sh, n = uint32_t(hi - q0);  // (at = b mod 4)
            uint32_t head = uint32_t(-reinterpret_cast<uintptr_t>(b)) & 3u;
            head = head < n ? head : n;
            const uint32_t body = (n - head) >> 2, tail = n - head - 4 * body;
            const uint32_t* const b4 = reinterpret_cast<const uint32_t*>(b + head);
            uint32_t* const s4 = reinterpret_cast<uint32_t*>(sl + at + head);
            for (uint32_t t = threadIdx.x; t < body; t += 256) s4[t] = b4[t];
            if (threadIdx.x < head) sl[at + threadIdx.x] = b[threadIdx.x];
            if (threadIdx.x < tail) sl[at + head + 4 * body + threadIdx.x] = b[head + 4 * body + threadIdx.x];
            if (own && pieces > 1 && threadIdx.x < uint32_t(C)) {  // (the same thread reads a kept byte and replaces it)
                uint8_t* const k = s_keep + size_t(yy - r0) * C + threadIdx.x;
                if (piece) sl[sh + threadIdx.x] = *k;
                if (piece + 1 < pieces) *k = row[e - C + threadIdx.x];
            }
        };
        if (piece) __syncthreads();  // (the last row of the piece before is still being computed from the ring)
        if (r0) fetch(r0 - 1);
        fetch(r0);
        for (uint32_t y = r0; y < r1; ++y) {
            if (y + 1 < oh) fetch(y + 1);
            __syncthreads();
            const bool inner = y >= 1 && y + 1 < oh;
            const uint8_t* const sc = s_sharp + ((y + 1 - r0) & (kSharpSlots - 1)) * slot_bytes + (reinterpret_cast<uintptr_t>(row_of(y) + lo) & 3u);
            const uint8_t* su = sc;
            const uint8_t* sd = sc;
            if (inner) {
                su = s_sharp + ((y - r0) & (kSharpSlots - 1)) * slot_bytes + (reinterpret_cast<uintptr_t>(row_of(y - 1) + lo) & 3u);
                sd = s_sharp + ((y + 2 - r0) & (kSharpSlots - 1)) * slot_bytes + (reinterpret_cast<uintptr_t>(row_of(y + 1) + lo) & 3u);
            }
            for (size_t q = s + threadIdx.x; q < e; q += 256) {
                const size_t x = q / C;
                const uint32_t ch = uint32_t(q - x * C), i = uint32_t(q - lo);
                const uint32_t val = sc[i];
                uint32_t d = val;
                if (inner && x >= 1 && x + 1 < ow) {
                    const uint32_t sum9 = uint32_t(su[i - C]) + su[i] + su[i + C] + sc[i - C] + val + sc[i + C] + sd[i - C] + sd[i] + sd[i + C];
                    d = photo_smooth(sum9, val);
                }
                const uint32_t res = photo_blend(d, val, me.param);
                photo_store<T, CHW, LUT>(me.last, o, lut, v, C, plane, size_t(y) * ow + x, ch, p + size_t(y) * pitch + q, &res);
            }
        }
    }
}

template <int C>
hipError_t launch_step_c(const PhotoStep& p, hipStream_t s) {
    const uint32_t views = p.views, ow = p.ow, oh = p.oh, step = p.step;
    const uint64_t npix = uint64_t(oh) * ow;
    if (p.info.stats) {
        if (hipError_t err = hipMemsetAsync(p.d_stats, 0, size_t(views) * photo_stats_stride(C), s)) return err;
        // (4096 pixels per workgroup and round, at most 32 workgroups per view: a 224 x 224 view takes 13)
        const uint32_t gx = uint32_t(std::min<uint64_t>((npix + 4095) / 4096, 32));
        k_photo_stats<C><<<dim3(gx, views), dim3(256), 0, s>>>(p.d_px, p.d_chains, p.d_stats, npix, step);
    }
    if (p.info.has(PhotoKind::kTable)) k_photo_lut<C><<<dim3(views), dim3(64), 0, s>>>(p.d_chains, p.d_stats, p.d_luts, npix, step);
    const dim3 grid(uint32_t((npix + 1023) / 1024), views);
    dispatch_out(p.out, [&](auto E, auto CHW, auto LUT) {
        k_photo_apply<C, E(), CHW(), LUT()><<<grid, dim3(256), 0, s>>>(p.d_px, p.d_chains, p.d_luts, p.d_table, p.d_out, npix, step);
    });
    if (p.info.has(PhotoKind::kBlur)) {  // the views that blur in this step sat the pass above out: rows in place, then columns, in place or to d_out
        k_photo_blur_rows<C><<<dim3((oh + blur_rows_per_group(ow) - 1) / blur_rows_per_group(ow), views), dim3(256), 0, s>>>(p.d_px, p.d_chains, ow, oh, step);
        const dim3 cols(uint32_t((uint64_t(ow) * C + kBlurStrip - 1) / kBlurStrip), views);
        dispatch_out(p.out, [&](auto E, auto CHW, auto LUT) {
            k_photo_blur_cols<C, E(), CHW(), LUT()><<<cols, dim3(256), 0, s>>>(p.d_px, p.d_chains, p.d_table, p.d_out, ow, oh, step);
        });
    }
    if (p.info.has(PhotoKind::kSharp)) {  // the views that sharpen in this step: the rows between the bands first, as they stand, then the bands
        const uint32_t rows = p.sharp_rows, bands = photo_sharp_bands(oh, rows);
        const uint64_t pitch = uint64_t(ow) * C, halo_stride = photo_sharp_halo_bytes(ow, oh, C, rows);
        if (bands > 1) k_photo_sharp_save<C><<<dim3(bands - 1, views), dim3(256), 0, s>>>(p.d_px, p.d_chains, p.d_halo, ow, oh, rows, halo_stride, step);
        const uint32_t lds = kSharpSlots * sharp_slot_bytes(pitch) + (sharp_pieces(pitch) > 1 ? rows * C : 0u);
        const dim3 grid_s(bands, views);
        dispatch_out(p.out, [&](auto E, auto CHW, auto LUT) {
            k_photo_sharp<C, E(), CHW(), LUT()><<<grid_s, dim3(256), lds, s>>>(p.d_px, p.d_chains, p.d_halo, p.d_table, p.d_out, ow, oh, rows, halo_stride, step);
        });
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_photo_step(const PhotoStep& p, hipStream_t stream) {
    if (!p.views || p.views > 65535 || (p.c != 1 && p.c != 3) || !p.ow || !p.oh || p.step >= LLCOMP_MI_PHOTO_MAX_OPS) return hipErrorInvalidValue;
    if (!p.d_px || !p.d_chains || !p.d_out || (reinterpret_cast<uintptr_t>(p.d_chains) & 3u)) return hipErrorInvalidValue;
    if ((p.info.stats || p.info.has(PhotoKind::kTable)) && (!p.d_stats || !p.d_luts || (reinterpret_cast<uintptr_t>(p.d_stats) & 7u))) return hipErrorInvalidValue;
    if (!p.out.plain && (!p.d_table || (reinterpret_cast<uintptr_t>(p.d_table) & (p.out.esize - 1)))) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(p.d_out) & (p.out.esize - 1)) return hipErrorInvalidValue;
    const uint64_t npix = uint64_t(p.oh) * p.ow;
    if ((npix + 1023) / 1024 > 0x7FFFFFFFull) return hipErrorInvalidValue;  // (an output of 2^41 pixels: no buffer holds it)
    if (p.info.has(PhotoKind::kBlur) && uint64_t(p.ow) * p.c > 0x7FFFFFFFull * kBlurStrip) return hipErrorInvalidValue;  // (the column kernel's grid; a row of 2^37 bytes)
    if (p.info.has(PhotoKind::kSharp)) {  // (the band's grid; the halo area of a view in bands; the kept columns of a row in pieces, which are LDS)
        if (!p.sharp_rows || p.sharp_rows > p.oh || (photo_sharp_bands(p.oh, p.sharp_rows) > 1 && !p.d_halo)) return hipErrorInvalidValue;
        if (sharp_pieces(uint64_t(p.ow) * p.c) > 1 && p.sharp_rows > kSharpKeepRows) return hipErrorInvalidValue;
    }
    return p.c == 3 ? launch_step_c<3>(p, stream) : launch_step_c<1>(p, stream);
}

}  // namespace llcomp_mi
