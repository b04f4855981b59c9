// photo_kernels.hip -- the three kernels of the photometric chains (llcomp_mi_codec_decode_photo_views / _photo_warped_views): the
// statistics of every view whose op of the step reads them, the table of every view whose op is one, and the per-pixel pass.  All views
// of a chunk run a step together; nothing goes back to the host in between.  The arithmetic is photo_rule.hpp's -- the functions
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

// The op of chain `ch` at `step` and whether it is the chain's last; false when the view sits this step out.  An empty chain has one
// step, step 0, which only writes the output.
__device__ __forceinline__ bool photo_step_op(const llcomp_mi_photo_chain& ch, uint32_t step, uint32_t& op, float& param, bool& last) {
    const uint32_t n = ch.n_ops < LLCOMP_MI_PHOTO_MAX_OPS ? ch.n_ops : uint32_t(LLCOMP_MI_PHOTO_MAX_OPS);
    if (step >= (n ? n : 1u)) return false;
    op = n ? ch.ops[step].op : kPhotoNoOp;
    param = n ? ch.ops[step].param : 0.0f;
    last = step + 1 >= n;
    return true;
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
    uint32_t op;
    float param;
    bool last;
    if (!photo_step_op(chains[v], step, op, param, last) || !photo_needs_stats(op)) return;  // (the whole workgroup alike)
    const bool hist = op != LLCOMP_MI_PHOTO_CONTRAST;
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
    uint32_t op;
    float param;
    bool last;
    if (!photo_step_op(chains[v], step, op, param, last) || !photo_is_table(op)) return;
    const bool need = photo_needs_stats(op);
    const unsigned long long* g_sum = reinterpret_cast<const unsigned long long*>(stats + size_t(v) * (8 + 1024 * C));
    const uint32_t* g_hist = reinterpret_cast<const uint32_t*>(g_sum + 1);
    for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 64) s_hist[j] = need ? g_hist[j] : 0u;
    __syncthreads();
    if (threadIdx.x < uint32_t(C)) photo_table(op, param, s_hist + 256 * threadIdx.x, need ? uint64_t(*g_sum) : 0ull, npix, s_lut + 256 * threadIdx.x);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < uint32_t(C * 256); j += 64) luts[size_t(v) * (C * 256) + j] = s_lut[j];
}

// The per-pixel pass: blockIdx.y the view, a workgroup takes 1024 of its pixels.  A table op looks every channel up in the view's table
// (copied to LDS), COLOR and GRAYSCALE are computed from the pixel, the step of an empty chain changes nothing.  The value goes back in
// place, or -- the chain's last step -- through the group's output format to `out`.  E, CHW, LUT as in the gather of the warped views.
template <int C, int E, bool CHW, bool LUT>
__global__ __launch_bounds__(256) void k_photo_apply(uint8_t* __restrict__ px, const llcomp_mi_photo_chain* __restrict__ chains,
                                                     const uint8_t* __restrict__ luts, const void* __restrict__ table, void* __restrict__ out,
                                                     uint64_t npix, uint32_t step) {
    using T = typename OutElem<E>::T;
    __shared__ uint8_t s_lut[C * 256];
    const uint32_t v = blockIdx.y;
    uint32_t op;
    float param;
    bool last;
    if (!photo_step_op(chains[v], step, op, param, last)) return;  // (the whole workgroup alike)
    const bool tab = op != kPhotoNoOp && photo_is_table(op);
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
            if (op == LLCOMP_MI_PHOTO_COLOR)
                photo_color(s[0], s[1], s[2], param);
            else if (op == LLCOMP_MI_PHOTO_GRAYSCALE)
                photo_grayscale(s[0], s[1], s[2]);
        }
        if (last) {
            for (int ch = 0; ch < C; ++ch) out_store<T, CHW, LUT>(o, lut, v, C, npix, i, ch, s[ch]);
        } else {
            for (int ch = 0; ch < C; ++ch) p[i * C + ch] = uint8_t(s[ch]);
        }
    }
}

template <int C, int E, bool CHW, bool LUT>
void launch_apply(dim3 grid, hipStream_t s, uint8_t* d_px, const llcomp_mi_photo_chain* d_chains, const uint8_t* d_luts, const void* d_table,
                  void* d_out, uint64_t npix, uint32_t step) {
    k_photo_apply<C, E, CHW, LUT><<<grid, dim3(256), 0, s>>>(d_px, d_chains, d_luts, d_table, d_out, npix, step);
}

template <int C>
hipError_t launch_step_c(uint8_t* d_px, const llcomp_mi_photo_chain* d_chains, uint8_t* d_stats, uint8_t* d_luts, const void* d_table,
                         const OutFormat& o, void* d_out, uint32_t views, uint64_t npix, uint32_t step, bool stats, bool table, hipStream_t s) {
    if (stats) {
        if (hipError_t err = hipMemsetAsync(d_stats, 0, size_t(views) * photo_stats_stride(C), s)) return err;
        // (4096 pixels per workgroup and round, at most 32 workgroups per view: a 224 x 224 view takes 13)
        const uint32_t gx = uint32_t(std::min<uint64_t>((npix + 4095) / 4096, 32));
        k_photo_stats<C><<<dim3(gx, views), dim3(256), 0, s>>>(d_px, d_chains, d_stats, npix, step);
    }
    if (table) k_photo_lut<C><<<dim3(views), dim3(64), 0, s>>>(d_chains, d_stats, d_luts, npix, step);
    const dim3 grid(uint32_t((npix + 1023) / 1024), views);
    const bool chw = o.layout == LLCOMP_MI_LAYOUT_CHW;
#define LLMI_PHOTO(E, CHW, LUT) launch_apply<C, E, CHW, LUT>(grid, s, d_px, d_chains, d_luts, d_table, d_out, npix, step)
    if (o.plain)
        LLMI_PHOTO(1, false, false);
    else if (o.esize == 1)  // (U8 CHW: U8 HWC is plain)
        LLMI_PHOTO(1, true, true);
    else if (o.esize == 2)
        chw ? LLMI_PHOTO(2, true, true) : LLMI_PHOTO(2, false, true);
    else
        chw ? LLMI_PHOTO(4, true, true) : LLMI_PHOTO(4, false, true);
#undef LLMI_PHOTO
    return hipGetLastError();
}

}  // namespace

hipError_t launch_photo_step(uint8_t* d_px, const llcomp_mi_photo_chain* d_chains, void* d_stats, uint8_t* d_luts, const void* d_table,
                             const OutFormat& o, void* d_out, uint32_t views, uint32_t c, uint32_t ow, uint32_t oh, uint32_t step, bool stats,
                             bool table, hipStream_t stream) {
    if (!views || views > 65535 || (c != 1 && c != 3) || !ow || !oh || step >= LLCOMP_MI_PHOTO_MAX_OPS) return hipErrorInvalidValue;
    if (!d_px || !d_chains || !d_out || (reinterpret_cast<uintptr_t>(d_chains) & 3u)) return hipErrorInvalidValue;
    if ((stats || table) && (!d_stats || !d_luts || (reinterpret_cast<uintptr_t>(d_stats) & 7u))) return hipErrorInvalidValue;
    if (!o.plain && (!d_table || (reinterpret_cast<uintptr_t>(d_table) & (o.esize - 1)))) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(d_out) & (o.esize - 1)) return hipErrorInvalidValue;
    const uint64_t npix = uint64_t(oh) * ow;
    if ((npix + 1023) / 1024 > 0x7FFFFFFFull) return hipErrorInvalidValue;  // (an output of 2^41 pixels: no buffer holds it)
    uint8_t* st = static_cast<uint8_t*>(d_stats);
    return c == 3 ? launch_step_c<3>(d_px, d_chains, st, d_luts, d_table, o, d_out, views, npix, step, stats, table, stream)
                  : launch_step_c<1>(d_px, d_chains, st, d_luts, d_table, o, d_out, views, npix, step, stats, table, stream);
}

}  // namespace llcomp_mi
