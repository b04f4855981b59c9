// resize_v_out_body.inc -- the body of k_resize_v_out and k_resize_v_out_bias (resize_kernels.hip), which differ in the constant BIAS
// alone: included once in each, so that the kernel without a bias is compiled from exactly the text it always had (a shared
// __device__ function changed the instruction order of some of its instantiations; the other two passes share one without that).
    using T = typename Elem<E>::T;
    const uint32_t c = C ? uint32_t(C) : c_rt;
    __shared__ uint32_t s_lut[C ? C * 64 * E : 1];
    if constexpr (C != 0) {
        for (uint32_t j = threadIdx.x; j < uint32_t(C * 64 * E); j += 256) s_lut[j] = table[j];
        __syncthreads();
    }
    const T* __restrict__ lut = reinterpret_cast<const T*>(C ? s_lut : table);
    const uint32_t f = blockIdx.y;
    const ResizeFrame& e = tab[f];
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= uint64_t(oh) * ow) return;
    const uint32_t y = uint32_t(i / ow), x = uint32_t(i - uint64_t(y) * ow), ky = e.ky;
    const int32_t* lo = wts + e.vy;
    const int32_t* q = lo + oh + y;
    const size_t stride = size_t(ow) * c;
    const uint8_t* src = mid + ((size_t(f) * mh + uint32_t(lo[y])) * ow + x) * c;
    const uint32_t xo = (e.flags & 1u) ? ow - 1 - x : x;
    T* const o = static_cast<T*>(out);
    const size_t plane = size_t(oh) * ow, px = size_t(y) * ow + xo;  // (CHW: element [f][ch][y][xo] = (f * c + ch) * plane + px)
    int32_t b = 0;
    const int32_t* fill = nullptr;
    if constexpr (BIAS) {
        b = wts[e.pad[0] + ow + y];
        fill = wts + e.pad[1];
    }
    auto start = [&](uint32_t ch) { return BIAS ? b * fill[ch] : int32_t(0); };
    auto put = [&](uint32_t ch, uint32_t v) {
        if constexpr (CHW)
            o[(size_t(f) * c + ch) * plane + px] = lut[ch * 256 + v];
        else
            o[(size_t(f) * plane + px) * c + ch] = lut[ch * 256 + v];
    };
    if constexpr (C == 4) {
        int32_t a0 = start(0), a1 = start(1), a2 = start(2), a3 = start(3);
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint32_t p = *reinterpret_cast<const uint32_t*>(src + j * stride);
            a0 += wj * int32_t(p & 0xFF);
            a1 += wj * int32_t((p >> 8) & 0xFF);
            a2 += wj * int32_t((p >> 16) & 0xFF);
            a3 += wj * int32_t(p >> 24);
        }
        const uint32_t l0 = lut[q22_round(a0)], l1 = lut[256 + q22_round(a1)], l2 = lut[512 + q22_round(a2)], l3 = lut[768 + q22_round(a3)];
        if constexpr (CHW) {
            o[size_t(f) * 4 * plane + px] = T(l0);
            o[(size_t(f) * 4 + 1) * plane + px] = T(l1);
            o[(size_t(f) * 4 + 2) * plane + px] = T(l2);
            o[(size_t(f) * 4 + 3) * plane + px] = T(l3);
        } else {
            T* d = o + (size_t(f) * plane + px) * 4;
            if constexpr (E == 1)
                *reinterpret_cast<uint32_t*>(d) = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
            else if constexpr (E == 2)
                *reinterpret_cast<uint2*>(d) = make_uint2(l0 | (l1 << 16), l2 | (l3 << 16));
            else
                *reinterpret_cast<uint4*>(d) = make_uint4(l0, l1, l2, l3);
        }
    } else if constexpr (C == 3) {
        int32_t a0 = start(0), a1 = start(1), a2 = start(2);
        for (uint32_t j = 0; j < ky; ++j) {
            const int32_t wj = q[size_t(j) * oh];
            const uint8_t* p = src + j * stride;
            a0 += wj * int32_t(p[0]);
            a1 += wj * int32_t(p[1]);
            a2 += wj * int32_t(p[2]);
        }
        put(0, q22_round(a0));
        put(1, q22_round(a1));
        put(2, q22_round(a2));
    } else if constexpr (C == 1) {
        int32_t a = start(0);
        for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride]);
        put(0, q22_round(a));
    } else {
        for (uint32_t ch = 0; ch < c; ++ch) {
            int32_t a = start(ch);
            for (uint32_t j = 0; j < ky; ++j) a += q[size_t(j) * oh] * int32_t(src[j * stride + ch]);
            put(ch, q22_round(a));
        }
    }
