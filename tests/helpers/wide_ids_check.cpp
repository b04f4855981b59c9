// wide_ids_check.cpp -- the label boxes and the label targets of the wide id maps (map_bytes 3 and 4: llcomp_amd/csrc/batch_chunk.hpp,
// label_boxes_rule.hpp, label_lists.hpp, label_targets_rule.hpp) walked on the host under a sanitizer, workgroup by workgroup and thread
// by thread as k_label_boxes32<MB, K> and k_label_targets32<MB, K, KIND> do, through a memory that checks every access: an address
// read lies in the maps, a 16-byte access is aligned and whole inside its buffer, a 4-byte pixel is read at a multiple of 4; the maps
// are never written; every pixel of a band lies in exactly one run and has the run's id; every output byte is written exactly once and
// nothing outside; a slot of the workgroup's arrays lies inside them.  The results are compared with
// llcomp_mi_label_boxes32_reference and llcomp_mi_label_targets32_reference and with values worked out pixel by pixel.  Host code
// only; built and run by tests/test_wide_id_maps_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/wide_ids_check.cpp llcomp_amd/csrc/label_boxes.cpp llcomp_amd/csrc/label_targets.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "label_boxes_rule.hpp"
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
void label32_table_put(uint32_t n, const uint32_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at);
void target32_table_put(uint32_t n, const llcomp_mi_label_targets32& t, const TargetCall& c, uint8_t* at);
}  // namespace llcomp_mi

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

// the maps of a round: n samples of px pixels of MB bytes, `moff` bytes past a 16-byte boundary, ending where their array ends
struct Maps {
    std::unique_ptr<uint8_t[]> buf, copy;
    std::vector<uint32_t> ids_of;
    uint32_t MB, moff;
    size_t bytes;
    uint8_t* at() const { return buf.get() + moff; }
    bool unwritten() const { return std::memcmp(buf.get(), copy.get(), moff + bytes) == 0; }
};
Maps draw_maps(uint32_t MB, size_t px, uint32_t moff, const std::vector<uint32_t>& pool, std::mt19937& rng) {
    Maps m;
    m.MB = MB, m.moff = moff, m.bytes = MB * px;
    m.buf.reset(new uint8_t[moff + m.bytes]);  // (operator new[] aligns to 16)
    m.copy.reset(new uint8_t[moff + m.bytes]);
    std::memset(m.buf.get(), 0xEE, moff);
    m.ids_of.resize(px);
    for (size_t i = 0; i < px;) {  // runs of drawn lengths
        const uint32_t id = pool[rng() % pool.size()];
        for (uint32_t len = 1 + rng() % 9; len && i < px; --len) m.ids_of[i++] = id;
    }
    for (size_t i = 0; i < px; ++i) std::memcpy(m.at() + MB * i, &m.ids_of[i], MB);  // (little-endian: the low MB bytes)
    std::memcpy(m.copy.get(), m.buf.get(), moff + m.bytes);
    return m;
}

// the records of a sample's list, and every pixel of the sample: in how many runs it lay
struct BoxSink {
    LabelFinder<const uint32_t*> finder;
    std::vector<llcomp_mi_label_box>* recs;  // of the sample's list
    const uint32_t* ids_of;  // of the sample
    uint32_t ow, oh;
    std::vector<uint8_t>* seen;
    bool bad = false;
    void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        if (y >= oh || x_first >= x_end || x_end > ow || length != x_end - x_first) return void(bad = true);
        for (uint32_t x = x_first; x < x_end; ++x) bad |= ids_of[size_t(y) * ow + x] != id || ++(*seen)[size_t(y) * ow + x] != 1;
        const uint32_t j = finder.find(id);
        if (j == kLabel16None) return;
        if (j >= recs->size()) return void(bad = true);
        label_box_update((*recs)[j], x_first, x_end, y, length);
    }
};

template <uint32_t MB>
int boxes_walk(const LabelGeom& g, uint32_t n, const uint32_t* tfirst, const uint32_t* tsamples, const uint32_t* tids, uint32_t n_listed, uint32_t K, const Maps& m,
               std::vector<llcomp_mi_label_box>& out) {
    HostMem mem{g.maps, g.bytes};
    for (uint32_t k = 0; k < n_listed; ++k) {
        const uint32_t i = tsamples[k];
        CHECK(i < n && (!k || tsamples[k - 1] < i));
        const uint32_t at = tfirst[i], cnt = tfirst[i + 1] - at;
        CHECK(cnt && cnt <= K);
        std::vector<llcomp_mi_label_box> recs(cnt, label_box_identity(g.ow, g.oh));
        std::vector<uint8_t> seen(size_t(g.ow) * g.oh, 0);
        for (uint32_t b = 0; b < g.bands; ++b) {  // one workgroup
            uint64_t sample, lo, hi;
            label_band<MB>(g, i, b, sample, lo, hi);
            for (uint32_t t = 0; t < kLabelThreads; ++t) {
                BoxSink sink{label_finder32(tids + at, cnt), &recs, m.ids_of.data() + size_t(i) * g.ow * g.oh, g.ow, g.oh, &seen};
                label_boxes_thread<MB>(g, sample, lo, hi, t, mem, sink);
                CHECK(!sink.bad);
            }
        }
        for (uint8_t s : seen) CHECK(s == 1);
        for (uint32_t j = 0; j < cnt; ++j) out[at + j] = recs[j];
    }
    CHECK(!mem.bad);
    return 0;
}

int run_boxes(uint32_t MB, uint32_t n, uint32_t ow, uint32_t oh, uint32_t moff, const std::vector<std::vector<uint32_t>>& lists, const std::vector<uint32_t>& pool,
              std::mt19937& rng) {
    const size_t P = size_t(ow) * oh;
    const Maps m = draw_maps(MB, n * P, moff, pool, rng);
    std::vector<uint32_t> ids, first(1, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        ids.insert(ids.end(), lists[i].begin(), lists[i].end());
        first.push_back(uint32_t(ids.size()));
    }
    const uint32_t total = first[n];
    ids.push_back(0);  // (never NULL)
    uint32_t longest = 0, n_listed = 0;
    CHECK(label_boxes32_check_call(MB, n, ow, oh, ids.data(), first.data(), &longest, &n_listed) == LLCOMP_MI_OK);
    const uint32_t K = label16_capacity(longest);
    std::vector<llcomp_mi_label_box> ref(total + 1, llcomp_mi_label_box{7, 7, 7, 7, 7}), got(total + 1, llcomp_mi_label_box{7, 7, 7, 7, 7});
    CHECK(llcomp_mi_label_boxes32_reference(m.at(), MB, n, ow, oh, ids.data(), first.data(), ref.data()) == LLCOMP_MI_OK && ref[total].count == 7);
    const Label16Table tab(n, n_listed, total, 4);
    CHECK(tab.bytes <= label32_table_bound(n, total));
    std::unique_ptr<uint8_t[]> table(new uint8_t[tab.bytes]);
    label32_table_put(n, ids.data(), first.data(), n_listed, table.get());
    const uint32_t* tfirst = reinterpret_cast<const uint32_t*>(table.get() + tab.first_at);
    const uint32_t* tsamples = reinterpret_cast<const uint32_t*>(table.get() + tab.samples_at);
    const uint32_t* tids = reinterpret_cast<const uint32_t*>(table.get() + tab.ids_at);
    const uint64_t base = reinterpret_cast<uintptr_t>(m.at());
    if (MB == 3) {
        if (boxes_walk<3>(label_geom<3>(base, n, ow, oh), n, tfirst, tsamples, tids, n_listed, K, m, got)) return 1;
    } else {
        if (boxes_walk<4>(label_geom<4>(base, n, ow, oh), n, tfirst, tsamples, tids, n_listed, K, m, got)) return 1;
    }
    CHECK(m.unwritten());
    CHECK(!total || std::memcmp(ref.data(), got.data(), total * sizeof(llcomp_mi_label_box)) == 0);
    for (uint32_t i = 0; i < n; ++i)  // ... and pixel by pixel
        for (uint32_t j = first[i]; j < first[i + 1]; ++j) {
            llcomp_mi_label_box b = label_box_identity(ow, oh);
            for (uint32_t y = 0; y < oh; ++y)
                for (uint32_t x = 0; x < ow; ++x)
                    if (m.ids_of[i * P + size_t(y) * ow + x] == ids[j]) label_box_update(b, x, x + 1, y, 1);
            CHECK(std::memcmp(&b, &ref[j], sizeof b) == 0);
        }
    return 0;
}

struct Case {
    uint32_t kind, dtype;
    int32_t dflt;
    uint32_t on, off;
};

int run_targets(uint32_t MB, const Case& cs, uint32_t n, uint32_t P, uint32_t moff, uint32_t ooff, const std::vector<std::vector<uint32_t>>& lists,
                const std::vector<uint32_t>& planes, const std::vector<uint32_t>& pool, std::mt19937& rng) {
    const size_t px = size_t(n) * P;
    const Maps m = draw_maps(MB, px, moff, pool, rng);
    std::vector<uint32_t> ids, first(1, 0u), plane_first(1, 0u);
    std::vector<int32_t> values;
    const bool planar = cs.kind == LLCOMP_MI_TARGET_PLANES, u8 = !planar && cs.dtype == LLCOMP_MI_TARGET_U8;
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t id : lists[i]) ids.push_back(id), values.push_back(int32_t(u8 ? rng() % 256 : rng() % 4 == 0 ? -3 : rng() % (planes[i] + 2)));  // (shared values)
        first.push_back(uint32_t(ids.size()));
        plane_first.push_back(plane_first.back() + planes[i]);
    }
    ids.push_back(0), values.push_back(0);  // (never NULL)
    llcomp_mi_label_targets32 t{};
    t.struct_size = sizeof t, t.map_bytes = MB, t.kind = cs.kind, t.dtype = cs.dtype, t.default_value = cs.dflt, t.on_bits = cs.on, t.off_bits = cs.off;
    t.ids = ids.data(), t.values = values.data(), t.first = first.data(), t.plane_first = planar ? plane_first.data() : nullptr;
    TargetCall c;
    CHECK(label_targets32_check_call(n, P, 1, &t, c) == LLCOMP_MI_OK);
    const uint32_t ES = c.esize, K = label16_capacity(c.longest);
    CHECK(c.out_bytes == llcomp_mi_label_targets32_out_bytes(n, P, 1, &t) && ooff % ES == 0);
    CHECK(c.out_bytes == (planar ? uint64_t(plane_first[n]) : uint64_t(n)) * P * ES);
    std::unique_ptr<uint8_t[]> obuf(new uint8_t[ooff + c.out_bytes]), rbuf(new uint8_t[ooff + c.out_bytes + 16]);
    std::memset(obuf.get(), 0xA5, ooff + c.out_bytes);
    std::memset(rbuf.get(), 0xA5, ooff + c.out_bytes + 16);
    CHECK(llcomp_mi_label_targets32_reference(m.at(), n, P, 1, &t, rbuf.get() + ooff) == LLCOMP_MI_OK);
    for (uint32_t b = 0; b < 16; ++b) CHECK(rbuf[ooff + c.out_bytes + b] == 0xA5);
    for (uint32_t b = 0; b < ooff; ++b) CHECK(rbuf[b] == 0xA5);

    const TargetTable tt(n, c.n_work, c.total, planar, 4);
    CHECK(tt.bytes <= target32_table_bound(n, c.total));
    std::unique_ptr<uint8_t[]> table(new uint8_t[tt.bytes]);
    target32_table_put(n, t, c, table.get());
    const uint32_t* tfirst = reinterpret_cast<const uint32_t*>(table.get() + tt.first_at);
    const uint32_t* tsamples = reinterpret_cast<const uint32_t*>(table.get() + tt.samples_at);
    const uint32_t* tplanes = planar ? reinterpret_cast<const uint32_t*>(table.get() + tt.planes_at) : nullptr;
    const int32_t* tvalues = reinterpret_cast<const int32_t*>(table.get() + tt.values_at);
    const uint32_t* tids = reinterpret_cast<const uint32_t*>(table.get() + tt.ids_at);

    const TargetGeom g = target_geom(reinterpret_cast<uintptr_t>(m.at()), reinterpret_cast<uintptr_t>(obuf.get() + ooff), n, P, 1, MB);
    const TargetParams a{cs.kind, ES, cs.dflt, cs.on, cs.off};
    const uint32_t chunks = target_plane_chunks(cs.kind, c.most_planes);
    HostMem mem{g.maps, g.map_bytes};
    HostSink sink{g.out, c.out_bytes, std::vector<uint8_t>(size_t(c.out_bytes), 0)};
    for (uint32_t y = 0; y < c.n_work; ++y) {
        CHECK(tsamples[y] < n && (!y || tsamples[y - 1] < tsamples[y]));
        const uint32_t i = tsamples[y];
        CHECK(tfirst[i + 1] - tfirst[i] <= K && tfirst[i + 1] <= c.total);
        for (uint32_t seg = 0; seg < g.segments; ++seg)
            for (uint32_t z = 0; z < chunks; ++z) {  // one workgroup
                Slots<uint16_t> v16(planar ? kTargetSegment : 0);
                Slots<uint32_t> list(K), vals(K), v32(planar ? 0 : kTargetSegment);
                if (planar) label_targets_host_workgroup(g, a, MB, tfirst, tplanes, tvalues, tids, i, seg, z, mem, sink, list, vals, v16);
                else label_targets_host_workgroup(g, a, MB, tfirst, tplanes, tvalues, tids, i, seg, z, mem, sink, list, vals, v32);
                CHECK(!list.bad && !vals.bad && !v16.bad && !v32.bad);
            }
    }
    CHECK(!mem.bad && !sink.bad && m.unwritten());
    for (size_t b = 0; b < size_t(c.out_bytes); ++b) CHECK(sink.writes[b] == 1);
    for (uint32_t b = 0; b < ooff; ++b) CHECK(obuf[b] == 0xA5);
    CHECK(!c.out_bytes || std::memcmp(obuf.get() + ooff, rbuf.get() + ooff, size_t(c.out_bytes)) == 0);
    const uint8_t* o = obuf.get() + ooff;  // ... and pixel by pixel
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < P; ++p) {
            int32_t v = cs.dflt;
            for (uint32_t j = first[i]; j < first[i + 1]; ++j)
                if (ids[j] == m.ids_of[size_t(i) * P + p]) v = values[j];
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

// a strictly ascending list of `count` drawn ids of MB bytes
std::vector<uint32_t> draw_list(uint32_t count, uint32_t MB, std::mt19937& rng) {
    std::vector<uint32_t> l;
    while (l.size() < count) {
        for (size_t i = l.size(); i < count; ++i) l.push_back(MB == 3 ? rng() & 0xFFFFFFu : rng());
        std::sort(l.begin(), l.end());
        l.erase(std::unique(l.begin(), l.end()), l.end());
    }
    return l;
}

int check_refusals() {
    const uint32_t ids[5] = {0, 3, 0x01000001, 1, 2}, ids3[5] = {0, 3, 0xFFFFFF, 1, 0xFFFFFF}, same[5] = {0, 3, 3, 1, 2};
    const int32_t values[5] = {0, 1, 2, 3, 4};
    const uint32_t first[3] = {0, 3, 5}, badfirst[3] = {0, 4, 3};
    alignas(16) static uint8_t m[2 * 20 * 4 + 16];
    llcomp_mi_label_box out[5];
    std::memset(out, 0x5A, sizeof out);
    const uint8_t* o = reinterpret_cast<const uint8_t*>(out);
    CHECK(llcomp_mi_label_boxes32_reference(m, 4, 2, 5, 4, ids, first, out) == LLCOMP_MI_OK && out[0].count == 20);
    CHECK(llcomp_mi_label_boxes32_reference(m + 1, 3, 2, 5, 4, ids3, first, out) == LLCOMP_MI_OK);
    std::memset(out, 0x5A, sizeof out);
    for (uint32_t mb : {0u, 1u, 2u, 5u}) CHECK(llcomp_mi_label_boxes32_reference(m, mb, 2, 5, 4, ids3, first, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes32_reference(m, 3, 2, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS);  // (an id above 0xFFFFFF)
    for (uint32_t off : {1u, 2u, 3u, 6u}) CHECK(llcomp_mi_label_boxes32_reference(m + off, 4, 2, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes32_reference(m, 4, 2, 5, 4, same, first, out) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_boxes32_reference(m, 4, 2, 5, 4, ids, badfirst, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes32_reference(nullptr, 4, 2, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_boxes32_reference(m, 4, 2, 5, 4, ids, first, nullptr) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes32_reference(m, 4, 0, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_boxes32_reference(m, 4, 2, 0, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS);
    for (size_t b = 0; b < sizeof out; ++b) CHECK(o[b] == 0x5A);

    llcomp_mi_label_targets32 ok{};
    ok.struct_size = sizeof ok, ok.map_bytes = 4, ok.kind = LLCOMP_MI_TARGET_INDEX, ok.dtype = LLCOMP_MI_TARGET_I64, ok.default_value = -100;
    ok.ids = ids, ok.values = values, ok.first = first;
    TargetCall c;
    CHECK(label_targets32_check_call(2, 5, 4, &ok, c) == LLCOMP_MI_OK && c.esize == 8 && c.n_work == 2 && c.total == 5 && c.longest == 3 && c.out_bytes == 2 * 20 * 8);
    auto refused = [&](auto&& change) {
        llcomp_mi_label_targets32 t = ok;
        change(t);
        TargetCall cc;
        return label_targets32_check_call(2, 5, 4, &t, cc) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets32_out_bytes(2, 5, 4, &t) == 0;
    };
    CHECK(refused([](auto& t) { t.struct_size -= 1; }) && refused([](auto& t) { t.map_bytes = 0; }) && refused([](auto& t) { t.map_bytes = 1; }));
    CHECK(refused([](auto& t) { t.map_bytes = 2; }) && refused([](auto& t) { t.map_bytes = 5; }) && refused([](auto& t) { t.map_bytes = 3; }));
    CHECK(!refused([&](auto& t) { t.map_bytes = 3, t.ids = ids3; }) && refused([&](auto& t) { t.ids = same; }) && refused([](auto& t) { t.kind = 2; }));
    CHECK(refused([](auto& t) { t.ids = nullptr; }) && refused([](auto& t) { t.values = nullptr; }) && refused([&](auto& t) { t.first = badfirst; }));
    llcomp_mi_label_targets narrow{};  // the 16-bit struct goes on refusing the wide widths
    const uint16_t ids16[5] = {0, 3, 9, 1, 2};
    narrow.struct_size = sizeof narrow, narrow.map_bytes = 2, narrow.kind = LLCOMP_MI_TARGET_INDEX, narrow.dtype = LLCOMP_MI_TARGET_I64;
    narrow.ids = ids16, narrow.values = values, narrow.first = first;
    CHECK(label_targets_check_call(2, 5, 4, &narrow, c) == LLCOMP_MI_OK);
    narrow.map_bytes = 3;
    CHECK(label_targets_check_call(2, 5, 4, &narrow, c) == LLCOMP_MI_BAD_ARGS);
    narrow.map_bytes = 4;
    CHECK(label_targets_check_call(2, 5, 4, &narrow, c) == LLCOMP_MI_BAD_ARGS);
    alignas(16) static uint8_t tout[2 * 20 * 8 + 16];
    std::memset(tout, 0x5A, sizeof tout);
    CHECK(llcomp_mi_label_targets32_reference(m + 2, 2, 5, 4, &ok, tout) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets32_reference(m, 2, 5, 4, &ok, tout + 4) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_targets32_reference(nullptr, 2, 5, 4, &ok, tout) == LLCOMP_MI_BAD_ARGS && llcomp_mi_label_targets32_reference(m, 2, 5, 4, &ok, nullptr) == LLCOMP_MI_BAD_ARGS);
    for (uint8_t b : tout) CHECK(b == 0x5A);
    CHECK(llcomp_mi_label_targets32_reference(m, 2, 5, 4, &ok, tout + 8) == LLCOMP_MI_OK && tout[7] == 0x5A && tout[8] == 0 && tout[8 + 320] == 0x5A);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(2323);
    uint32_t rounds = 0;
    // ids that differ only in byte 2 or byte 3, the ends of the range
    const std::vector<uint32_t> pool3 = {0x000001, 0x010001, 0xFF0001, 0x000000, 0xFFFFFF, 0x00FF00, 0x123456};
    const std::vector<uint32_t> pool4 = {0x000001, 0x010001, 0xFF0001, 0x01000001, 0x00000000, 0xFFFFFFFF, 0x00FFFFFF, 0x80000000};
    const std::vector<std::vector<uint32_t>> lists3 = {{0x000001, 0x010001, 0xFFFFFF}, {}, {0x000000, 0x000002, 0xFF0001, 0xFFFFFF}};
    const std::vector<std::vector<uint32_t>> lists4 = {{0x000001, 0x01000001, 0xFFFFFFFF}, {}, {0x00000000, 0x010001, 0x00FFFFFF, 0x80000000, 0xFFFFFFFF}};
    // the boxes: widths around the pixels of a unit, heights around a band, three samples of which the middle one has an empty list,
    // the maps at every byte offset (4-byte maps: every multiple of 4), ending where their array ends
    const uint32_t B = kLabelBoxRows, ows[8] = {1, 5, 6, 7, 11, 16, 17, 33}, ohs[5] = {1, B - 1, B, B + 1, 2 * B + 3};
    for (uint32_t MB : {3u, 4u})
        for (uint32_t ow : ows)
            for (uint32_t oh : ohs)
                for (uint32_t moff = 0; moff < 16; moff += MB == 3 ? 1 : 4) {
                    if (run_boxes(MB, 3, ow, oh, moff, MB == 3 ? lists3 : lists4, MB == 3 ? pool3 : pool4, rng)) return 1;
                    ++rounds;
                }
    // the capacities and their borders
    for (uint32_t MB : {3u, 4u})
        for (uint32_t count : {1u, 256u, 257u, 1024u, 1025u, 4096u}) {
            std::vector<uint32_t> l = draw_list(count, MB, rng), half(l.begin(), l.begin() + count / 2 + 1), pool;
            if (MB == 4 && l.back() != 0xFFFFFFFFu) l.push_back(0xFFFFFFFFu), l.erase(l.begin());  // (the id the finder starts from, listed last)
            for (uint32_t i = 0; i < l.size(); i += 1 + count / 40) pool.push_back(l[i]);
            pool.push_back(l.back());
            for (uint32_t i = 0; i < 20; ++i) pool.push_back(MB == 3 ? rng() & 0xFFFFFFu : rng());
            if (run_boxes(MB, 2, 37, B + 2, MB == 3 ? 7 : 12, {l, half}, pool, rng)) return 1;
            if (run_targets(MB, Case{LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I64, -100, 0, 0}, 2, kTargetSegment + 45, MB == 3 ? 5 : 8, 8, {l, half}, {0, 0}, pool, rng)) return 1;
            rounds += 2;
        }
    // the targets: pixel counts around a segment, the same three samples, the maps at the same offsets, the output at none, one
    // element and 16 bytes less one element
    const uint32_t S = kTargetSegment, Ps[5] = {1, S - 1, S, S + 1, 2 * S + 5};
    static const Case cases[7] = {{LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_U8, 255, 0, 0},         {LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I32, -1, 0, 0},
                                  {LLCOMP_MI_TARGET_INDEX, LLCOMP_MI_TARGET_I64, -100, 0, 0},       {LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_U8, -1, 1, 0},
                                  {LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_F16, 1, 0x3B33, 0x2E66}, {LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_BF16, -1, 0x3F80, 0},
                                  {LLCOMP_MI_TARGET_PLANES, LLCOMP_MI_DTYPE_F32, 2, 0x3F666666, 0x3D4CCCCD}};
    for (uint32_t MB : {3u, 4u})
        for (const Case& cs : cases)
            for (uint32_t P : Ps)
                for (uint32_t moff = 0; moff < 16; moff += MB == 3 ? 1 : 4) {
                    const uint32_t ES = target_esize(cs.kind, cs.dtype), ooffs[3] = {0u, ES, 16u - ES};
                    if (run_targets(MB, cs, 3, P, moff, ooffs[moff % 3], MB == 3 ? lists3 : lists4, {3, 0, 2}, MB == 3 ? pool3 : pool4, rng)) return 1;
                    ++rounds;
                }
    if (check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
