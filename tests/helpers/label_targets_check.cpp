// label_targets_check.cpp -- the label targets (llcomp_amd/csrc/label_targets_rule.hpp) walked on the host under a sanitizer, workgroup
// by workgroup and thread by thread as k_label_targets<MB, K, KIND> does -- the table's samples that get workgroups, a workgroup per
// segment and plane chunk, the table, the list and the segment's values in arrays of the sizes the kernel's LDS has, the threads of
// each phase one after the other -- through a memory that checks every access: an address read lies in the maps, a 16-byte access is
// aligned and whole inside its buffer, an element access aligned to the element and inside; every output byte is written exactly once
// and nothing outside; a slot of the workgroup's arrays lies inside them.  The result is compared with
// llcomp_mi_label_targets_reference and with a value worked out pixel by pixel.  Host code only; built and run by
// tests/test_label_targets_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/label_targets_check.cpp llcomp_amd/csrc/label_targets.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "label_targets_rule.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace llcomp_mi {
void target_table_put(uint32_t n, const llcomp_mi_label_targets& t, const TargetCall& c, uint8_t* at);
}

namespace {

struct HostMem {
    uint64_t maps, bytes;
    bool bad = false;
    LabelChunk load16(uint64_t a) {
        LabelChunk c{{0, 0, 0, 0}};
        if ((a & 15) || a < maps || a + 16 > maps + bytes) return bad = true, c;
        std::memcpy(&c, reinterpret_cast<const void*>(uintptr_t(a)), 16);
        return c;
    }
    template <uint32_t N>
    uint32_t load_el(uint64_t a) {
        uint32_t v = 0;
        if ((a & (N - 1)) || a < maps || a + N > maps + bytes) return bad = true, v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);
        return v;
    }
};
struct HostSink {
    uint64_t out, bytes;
    std::vector<uint8_t> writes;  // of every output byte
    bool bad = false;
    void count(uint64_t a, uint32_t len) {
        for (uint32_t b = 0; b < len; ++b) bad |= ++writes[size_t(a - out) + b] != 1;
    }
    void store16(uint64_t a, const LabelChunk& c) {
        if ((a & 15) || a < out || a + 16 > out + bytes) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &c, 16);
        count(a, 16);
    }
    template <uint32_t ES>
    void store_el(uint64_t a, uint64_t bits) {
        if ((a & (ES - 1)) || a < out || a + ES > out + bytes) return void(bad = true);
        if (ES < 8 && (bits >> (8 * (ES & 7))) != 0) return void(bad = true);
        std::memcpy(reinterpret_cast<void*>(uintptr_t(a)), &bits, ES);
        count(a, ES);
    }
};
// an array of the workgroup's LDS
template <class T>
struct Slots {
    std::vector<T> a;
    mutable bool bad = false;
    T spare = 0;
    explicit Slots(size_t n) : a(n) {}
    T& operator[](size_t i) { return i < a.size() ? a[i] : (bad = true, spare); }
    const T& operator[](size_t i) const { return i < a.size() ? a[i] : (bad = true, spare); }
};

struct Case {
    uint32_t map_bytes, kind, dtype;
    int32_t dflt;
    uint32_t on, off;
};

// maps [n][P] of ids drawn from pool in runs, `moff` bytes past a 16-byte boundary; the output `ooff` bytes past one
int run(const Case& cs, uint32_t n, uint32_t P, uint32_t moff, uint32_t ooff, const std::vector<std::vector<uint16_t>>& lists, const std::vector<uint32_t>& planes,
        const std::vector<uint16_t>& pool, std::mt19937& rng) {
    const uint32_t MB = cs.map_bytes;
    const size_t px = size_t(n) * P;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[moff + MB * px]);  // (operator new[] aligns to 16; the maps end where the array ends)
    CHECK(reinterpret_cast<uintptr_t>(buf.get()) % 16 == 0 && moff % MB == 0);
    std::vector<uint16_t> ids_of(px);
    for (size_t i = 0; i < px;) {  // runs of drawn lengths
        const uint16_t id = pool[rng() % pool.size()];
        for (uint32_t len = 1 + rng() % 12; len && i < px; --len) ids_of[i++] = id;
    }
    for (size_t i = 0; i < px; ++i) std::memcpy(buf.get() + moff + MB * i, &ids_of[i], MB);
    std::vector<uint16_t> ids;
    std::vector<int32_t> values;
    std::vector<uint32_t> first(1, 0u), plane_first(1, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint16_t id : lists[i]) ids.push_back(id), values.push_back(int32_t(rng() % 4 == 0 ? -3 : cs.dtype == LLCOMP_MI_TARGET_U8 && cs.kind == 0 ? rng() % 256 : rng() % (planes[i] + 2)));
        first.push_back(uint32_t(ids.size()));
        plane_first.push_back(plane_first.back() + planes[i]);
    }
    if (cs.kind == LLCOMP_MI_TARGET_INDEX && cs.dtype == LLCOMP_MI_TARGET_U8)
        for (int32_t& v : values) v = v < 0 ? 255 : v;
    ids.push_back(0), values.push_back(0);  // (never NULL)
    llcomp_mi_label_targets t{};
    t.struct_size = sizeof t, t.map_bytes = MB, t.kind = cs.kind, t.dtype = cs.dtype, t.default_value = cs.dflt, t.on_bits = cs.on, t.off_bits = cs.off;
    t.ids = ids.data(), t.values = values.data(), t.first = first.data(), t.plane_first = cs.kind == LLCOMP_MI_TARGET_PLANES ? plane_first.data() : nullptr;
    TargetCall c;
    CHECK(label_targets_check_call(n, P, 1, &t, c) == LLCOMP_MI_OK);
    const uint32_t ES = c.esize, K = MB == 1 ? 256u : label16_capacity(c.longest);
    CHECK(c.longest <= K && c.out_bytes == llcomp_mi_label_targets_out_bytes(n, P, 1, &t) && ooff % ES == 0);
    CHECK(c.out_bytes == (cs.kind == LLCOMP_MI_TARGET_PLANES ? uint64_t(plane_first[n]) : uint64_t(n)) * P * ES);
    std::unique_ptr<uint8_t[]> obuf(new uint8_t[ooff + c.out_bytes]), rbuf(new uint8_t[ooff + c.out_bytes + 16]);
    std::memset(obuf.get(), 0xA5, ooff + c.out_bytes);
    std::memset(rbuf.get(), 0xA5, ooff + c.out_bytes + 16);
    CHECK(llcomp_mi_label_targets_reference(buf.get() + moff, n, P, 1, &t, rbuf.get() + ooff) == LLCOMP_MI_OK);
    for (uint32_t b = 0; b < 16; ++b) CHECK(rbuf[ooff + c.out_bytes + b] == 0xA5);
    for (uint32_t b = 0; b < ooff; ++b) CHECK(rbuf[b] == 0xA5);

    const bool planar = cs.kind == LLCOMP_MI_TARGET_PLANES;
    const TargetTable tt(n, c.n_work, c.total, planar);
    CHECK(tt.bytes <= target_table_bound(n, c.total));
    std::unique_ptr<uint8_t[]> table(new uint8_t[tt.bytes]);
    target_table_put(n, t, c, table.get());
    const uint32_t* tfirst = reinterpret_cast<const uint32_t*>(table.get() + tt.first_at);
    const uint32_t* tsamples = reinterpret_cast<const uint32_t*>(table.get() + tt.samples_at);
    const uint32_t* tplanes = planar ? reinterpret_cast<const uint32_t*>(table.get() + tt.planes_at) : nullptr;
    const int32_t* tvalues = reinterpret_cast<const int32_t*>(table.get() + tt.values_at);
    const uint16_t* tids = reinterpret_cast<const uint16_t*>(table.get() + tt.ids_at);

    const TargetGeom g = target_geom(reinterpret_cast<uintptr_t>(buf.get() + moff), reinterpret_cast<uintptr_t>(obuf.get() + ooff), n, P, 1, MB);
    const TargetParams a{cs.kind, ES, cs.dflt, cs.on, cs.off};
    const uint32_t chunks = target_plane_chunks(cs.kind, c.most_planes);
    CHECK(g.segments == (P + kTargetSegment - 1) / kTargetSegment && chunks >= 1 && chunks <= 65535);
    HostMem mem{g.maps, g.map_bytes};
    HostSink sink{g.out, c.out_bytes, std::vector<uint8_t>(size_t(c.out_bytes), 0)};
    for (uint32_t y = 0; y < c.n_work; ++y) {
        CHECK(tsamples[y] < n && (!y || tsamples[y - 1] < tsamples[y]));
        const uint32_t i = tsamples[y];
        CHECK(tfirst[i + 1] - tfirst[i] <= K && tfirst[i + 1] <= c.total && (!planar || tplanes[i + 1] > tplanes[i]));
        for (uint32_t seg = 0; seg < g.segments; ++seg)
            for (uint32_t z = 0; z < chunks; ++z) {  // one workgroup
                Slots<uint16_t> list(MB == 1 ? 0 : K), v16(planar ? kTargetSegment : 0);
                Slots<uint32_t> vals(K), v32(planar ? 0 : kTargetSegment);
                if (planar) label_targets_host_workgroup(g, a, MB, tfirst, tplanes, tvalues, tids, i, seg, z, mem, sink, list, vals, v16);
                else label_targets_host_workgroup(g, a, MB, tfirst, tplanes, tvalues, tids, i, seg, z, mem, sink, list, vals, v32);
                CHECK(!list.bad && !vals.bad && !v16.bad && !v32.bad);
            }
    }
    CHECK(!mem.bad && !sink.bad);
    for (size_t b = 0; b < size_t(c.out_bytes); ++b) CHECK(sink.writes[b] == 1);
    for (uint32_t b = 0; b < ooff; ++b) CHECK(obuf[b] == 0xA5);
    CHECK(!c.out_bytes || std::memcmp(obuf.get() + ooff, rbuf.get() + ooff, size_t(c.out_bytes)) == 0);
    // ... and pixel by pixel
    const uint8_t* o = obuf.get() + ooff;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < P; ++p) {
            int32_t v = cs.dflt;
            for (uint32_t j = first[i]; j < first[i + 1]; ++j)
                if (ids[j] == ids_of[size_t(i) * P + p]) v = values[j];
            if (!planar) {
                int64_t got = 0;
                const uint8_t* e = o + (size_t(i) * P + p) * ES;
                if (ES == 1) got = *e;
                else if (ES == 4) { int32_t x; std::memcpy(&x, e, 4); got = x; }
                else std::memcpy(&got, e, 8);
                CHECK(got == v);
            } else {
                for (uint32_t k = 0; k < planes[i]; ++k) {
                    uint32_t got = 0;
                    std::memcpy(&got, o + ((size_t(plane_first[i]) + k) * P + p) * ES, ES);
                    CHECK(got == (v >= 0 && uint32_t(v) == k ? cs.on : cs.off));
                }
            }
        }
    return 0;
}

// a strictly ascending list of `count` drawn ids below `limit`
std::vector<uint16_t> draw_list(uint32_t count, uint32_t limit, std::mt19937& rng) {
    std::vector<uint16_t> all(limit);
    for (uint32_t i = 0; i < limit; ++i) all[i] = uint16_t(i);
    std::shuffle(all.begin(), all.end(), rng);
    std::vector<uint16_t> l(all.begin(), all.begin() + count);
    std::sort(l.begin(), l.end());
    return l;
}

int check_refusals() {
    const uint16_t ids[5] = {0, 3, 9, 1, 2}, wide[5] = {0, 3, 300, 1, 2};
    const int32_t values[5] = {0, 1, 2, 3, 4}, neg[5] = {0, -1, 2, 3, 4}, big[5] = {0, 1, 2, 256, 4};
    const uint32_t first[3] = {0, 3, 5}, pf[3] = {0, 2, 6}, pf1[3] = {1, 2, 6}, pfdec[3] = {0, 4, 3}, pfbig[3] = {0, 4097, 4097}, badfirst[3] = {0, 4, 3};
    llcomp_mi_label_targets ok{};
    ok.struct_size = sizeof ok, ok.map_bytes = 2, ok.kind = LLCOMP_MI_TARGET_INDEX, ok.dtype = LLCOMP_MI_TARGET_I64, ok.default_value = -100;
    ok.ids = ids, ok.values = values, ok.first = first;
    TargetCall c;
    CHECK(label_targets_check_call(2, 5, 4, &ok, c) == LLCOMP_MI_OK && c.esize == 8 && c.n_work == 2 && c.total == 5 && c.longest == 3 && c.out_bytes == 2 * 20 * 8);
    CHECK(label_targets_check_call(2, 5, 4, nullptr, c) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets_out_bytes(2, 5, 4, nullptr) == 0);
    auto refused = [&](auto&& change) {
        llcomp_mi_label_targets t = ok;
        change(t);
        TargetCall cc;
        return label_targets_check_call(2, 5, 4, &t, cc) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets_out_bytes(2, 5, 4, &t) == 0;
    };
    CHECK(refused([](auto& t) { t.struct_size -= 1; }) && refused([](auto& t) { t.map_bytes = 0; }) && refused([](auto& t) { t.map_bytes = 3; }));
    CHECK(refused([](auto& t) { t.kind = 2; }) && refused([](auto& t) { t.dtype = 3; }) && refused([](auto& t) { t.ids = nullptr; }));
    CHECK(refused([](auto& t) { t.values = nullptr; }) && refused([](auto& t) { t.first = nullptr; }) && refused([&](auto& t) { t.first = badfirst; }));
    CHECK(refused([&](auto& t) { t.map_bytes = 1, t.ids = wide; }) && !refused([&](auto& t) { t.ids = wide; }) && !refused([](auto& t) { t.map_bytes = 1; }));
    CHECK(refused([](auto& t) { t.dtype = LLCOMP_MI_TARGET_U8; }) && !refused([](auto& t) { t.dtype = LLCOMP_MI_TARGET_U8, t.default_value = 255; }));
    CHECK(refused([&](auto& t) { t.dtype = LLCOMP_MI_TARGET_U8, t.default_value = 0, t.values = neg; }));
    CHECK(refused([&](auto& t) { t.dtype = LLCOMP_MI_TARGET_U8, t.default_value = 0, t.values = big; }) && !refused([&](auto& t) { t.values = neg; }));
    CHECK(refused([](auto& t) { t.kind = LLCOMP_MI_TARGET_PLANES, t.dtype = LLCOMP_MI_DTYPE_F16; }));  // (no plane_first)
    auto planes = [&](const uint32_t* p, uint32_t dtype, uint32_t on) {
        return [=](auto& t) { t.kind = LLCOMP_MI_TARGET_PLANES, t.dtype = dtype, t.plane_first = p, t.on_bits = on; };
    };
    CHECK(!refused(planes(pf, LLCOMP_MI_DTYPE_F16, 0x3C00)) && refused(planes(pf1, LLCOMP_MI_DTYPE_F16, 0x3C00)) && refused(planes(pfdec, LLCOMP_MI_DTYPE_F16, 0x3C00)));
    CHECK(refused(planes(pfbig, LLCOMP_MI_DTYPE_F16, 0x3C00)) && refused(planes(pf, LLCOMP_MI_DTYPE_F16, 0x10000)) && refused(planes(pf, LLCOMP_MI_DTYPE_U8, 256)));
    CHECK(!refused(planes(pf, LLCOMP_MI_DTYPE_F32, 0x3F800000)) && refused(planes(pf, 4, 1)) && !refused(planes(pf, LLCOMP_MI_DTYPE_BF16, 0x3F80)));
    llcomp_mi_label_targets huge = ok;  // 65535 samples of 2^32 - 1 pixels of 8 bytes: 2^51 bytes pass; 4096 planes each of 4 bytes are 2^62
    CHECK(label_targets_check_call(1, 65536, 65536, &huge, c) == LLCOMP_MI_BAD_ARGS);
    alignas(16) static uint16_t m[64];
    alignas(16) static uint8_t out[2 * 20 * 8 + 16];
    std::memset(out, 0x5A, sizeof out);
    CHECK(llcomp_mi_label_targets_reference(reinterpret_cast<uint8_t*>(m) + 1, 2, 5, 4, &ok, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_targets_reference(m, 2, 5, 4, &ok, out + 4) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets_reference(nullptr, 2, 5, 4, &ok, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_targets_reference(m, 2, 5, 4, &ok, nullptr) == LLCOMP_MI_BAD_ARGS && out[0] == 0x5A && out[8] == 0x5A);
    CHECK(llcomp_mi_label_targets_reference(m, 2, 5, 4, &ok, out + 8) == LLCOMP_MI_OK && out[7] == 0x5A && out[8] == 0 && out[8 + 320] == 0x5A);
    CHECK(llcomp_mi_label_targets_segment() == kTargetSegment && llcomp_mi_label_targets_max_planes() == kTargetMaxPlanes && kTargetMaxPlanes == 4096);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(1717);
    uint32_t rounds = 0;
    const uint32_t S = kTargetSegment, C = kTargetPlaneChunk;
    const uint32_t Ps[5] = {1, S - 1, S, S + 1, 2 * S + 3};
    static const Case cases[12] = {
        {1, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_U8, 255, 0, 0},        {1, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I32, -100, 0, 0},
        {1, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I64, -100, 0, 0},      {1, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_U8, -1, 1, 0},
        {1, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_F16, 1, 0x3B33, 0x2E66}, {1, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_F32, 0, 0x3F800000, 0},
        {2, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_U8, 0, 0, 0},          {2, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I32, -1, 0, 0},
        {2, LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I64, -100, 0, 0},      {2, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_U8, 0, 255, 7},
        {2, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_BF16, -1, 0x3F80, 0},  {2, LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_F32, 2, 0x3F666666, 0x3D4CCCCD}};
    // pixel counts around a segment, three samples of which the middle one has an empty list and no planes, the maps at every offset
    // of a 16-byte unit and the output at none, one element and 16 bytes less one element: the first and last units of a segment,
    // a plane and a sample are shared with their neighbours wherever P * ES is no multiple of 16
    static const uint16_t low[6] = {1, 2, 3, 200, 255, 0}, high[6] = {0x0001, 0x0101, 0x0201, 0xFF01, 0x0100, 0x0000};
    for (const Case& cs : cases)
        for (uint32_t P : Ps)
            for (uint32_t moff = 0; moff < 16; moff += cs.map_bytes) {
                const uint32_t ES = target_esize(cs.kind, cs.dtype);
                for (uint32_t ooff : {0u, ES, 16u - ES}) {
                    if (cs.map_bytes == 1) {
                        if (run(cs, 3, P, moff, ooff, {{1, 3, 255}, {}, {0, 2, 3, 200}}, {3, 0, 2}, std::vector<uint16_t>(low, low + 6), rng)) return 1;
                    } else {
                        if (run(cs, 3, P, moff, ooff, {{0x0001, 0x0101, 0xFF01}, {}, {0x0000, 0x0002, 0x0201, 0xFF00}}, {3, 0, 2}, std::vector<uint16_t>(high, high + 6), rng)) return 1;
                    }
                    ++rounds;
                }
            }
    // the capacities and their borders (1-byte maps: up to all 256 ids)
    static const uint32_t counts[6] = {1, 256, 257, 1024, 1025, 4096};
    for (uint32_t count : counts)
        for (const Case& cs : {cases[2], cases[4], cases[8], cases[10]}) {
            if (cs.map_bytes == 1 && count > 256) continue;
            std::vector<uint16_t> l = draw_list(count, cs.map_bytes == 1 ? 256 : 65536, rng), half(l.begin(), l.begin() + count / 2 + 1);
            std::vector<uint16_t> pool;
            for (uint32_t i = 0; i < count; i += 1 + count / 40) pool.push_back(l[i]);
            for (uint32_t i = 0; i < 20; ++i) pool.push_back(uint16_t(cs.map_bytes == 1 ? rng() % 256 : rng()));
            if (run(cs, 2, S + 45, 6, 16 - target_esize(cs.kind, cs.dtype), {l, half}, {5, 3}, pool, rng)) return 1;
            ++rounds;
        }
    // plane counts: one, a chunk, a chunk and one, and the most (at P <= S), next to a sample without planes
    for (uint32_t planes : {1u, C, C + 1, kTargetMaxPlanes})
        for (const Case& cs : {cases[3], cases[4], cases[10], cases[11]}) {
            const uint32_t P = planes == kTargetMaxPlanes ? 37 : S + 9;
            std::vector<uint16_t> l = draw_list(40, 256, rng);
            if (run(cs, 3, P, 2, target_esize(cs.kind, cs.dtype), {l, l, {}}, {planes, 0, planes == 1 ? 2 : planes - 1}, l, rng)) return 1;
            ++rounds;
        }
    if (check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
