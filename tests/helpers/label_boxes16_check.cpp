// label_boxes16_check.cpp -- the label boxes of both calls (llcomp_amd/csrc/label_boxes_rule.hpp, label_lists.hpp) walked on the host
// under a sanitizer, workgroup by workgroup and thread by thread as k_label_boxes16<K> and k_label_boxes do -- for the listed call the
// table's listed samples, a workgroup per band, the list and the records of the band in arrays of the capacity K the call would launch,
// for the dense call 256 records per band; label_boxes_thread for each of the 256 threads, then the merge of the records that have a
// pixel -- through a memory that checks every access: an address read lies in the maps, a 16-byte access is aligned and inside the
// batch, a pixel's one aligned to the pixel; a record merged lies inside the call's records, a list slot inside the capacity.  The
// result is compared with llcomp_mi_label_boxes16_reference or llcomp_mi_label_boxes_reference and with a count pixel by pixel.  Host
// code only; built and run by tests/test_label_boxes16_sanitizers.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/label_boxes16_check.cpp llcomp_amd/csrc/label_boxes.cpp
// Prints "ok <rounds>".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "label_boxes_rule.hpp"
#include "label_lists.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

namespace llcomp_mi {
void label16_table_put(uint32_t n, const uint16_t* ids, const uint32_t* first, uint32_t n_listed, uint8_t* at);
}

namespace {

struct HostMem {
    uint64_t maps, bytes;
    uint32_t mb;  // the map's bytes per pixel
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
        if (N != mb || (a & (N - 1)) || a < maps || a + N > maps + bytes) return bad = true, v;
        std::memcpy(&v, reinterpret_cast<const void*>(uintptr_t(a)), N);
        return v;
    }
};
// the dense call's finder: the id is the slot, of 256
struct Identity {
    uint32_t count;
    uint32_t find(uint32_t id) const { return id; }
};
// the workgroup's arrays of K slots
template <class Finder>
struct WgSink {
    Finder finder;
    std::vector<llcomp_mi_label_box>& recs;
    bool bad = false;
    void run(uint32_t id, uint32_t x_first, uint32_t x_end, uint32_t y, uint32_t length) {
        const uint32_t j = finder.find(id);
        if (j == kLabel16None) return;
        if (j >= recs.size() || j >= finder.count || !length || x_first >= x_end) return void(bad = true);
        label_box_update(recs[j], x_first, x_end, y, length);
    }
};
// One workgroup: band b of sample i with cnt records, which are out[0 .. cnt) of the call's
template <uint32_t MB, class Finder>
bool workgroup(const LabelGeom& g, uint32_t i, uint32_t b, const Finder& finder, uint32_t cnt, HostMem& mem, llcomp_mi_label_box* out) {
    std::vector<llcomp_mi_label_box> recs(cnt, label_box_identity(g.ow, g.oh));
    uint64_t sample, lo, hi;
    label_band<MB>(g, i, b, sample, lo, hi);
    for (uint32_t tid = 0; tid < kLabelThreads; ++tid) {
        WgSink<Finder> sink{finder, recs};
        label_boxes_thread<MB>(g, sample, lo, hi, tid, mem, sink);
        if (sink.bad) return false;
    }
    for (uint32_t j = 0; j < cnt; ++j) {
        if (!recs[j].count) continue;
        llcomp_mi_label_box& o = out[j];
        o.count += recs[j].count;
        o.x0 = std::min(o.x0, recs[j].x0), o.y0 = std::min(o.y0, recs[j].y0), o.x1 = std::max(o.x1, recs[j].x1), o.y1 = std::max(o.y1, recs[j].y1);
    }
    return true;
}

// the dense call on n byte maps at byte offset `off`
int run8(uint32_t n, uint32_t ow, uint32_t oh, uint32_t off, std::mt19937& rng) {
    const size_t px = size_t(n) * ow * oh;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[off + px]);  // (operator new[] aligns to 16; the batch ends where the array ends)
    CHECK(reinterpret_cast<uintptr_t>(buf.get()) % 16 == 0);
    uint8_t* maps = buf.get() + off;
    for (size_t i = 0; i < px;) {  // runs of drawn lengths
        const uint8_t id = rng() % 4 ? uint8_t(rng() % 6) : uint8_t(rng());
        for (uint32_t len = 1 + rng() % 12; len && i < px; --len) maps[i++] = id;
    }
    CHECK(label_boxes_check_call(n, ow, oh) == LLCOMP_MI_OK);
    const uint32_t total = n * kLabelIds;
    std::vector<llcomp_mi_label_box> ref(total + 1, llcomp_mi_label_box{9, 9, 9, 9, 9}), out(total);
    CHECK(llcomp_mi_label_boxes_reference(maps, n, ow, oh, ref.data()) == LLCOMP_MI_OK && ref[total].count == 9);
    for (uint32_t r = 0; r < total; ++r) out[r] = label_box_identity(ow, oh);  // k_label_boxes_init
    const LabelGeom g = label_geom<1>(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    CHECK(g.bytes == px);
    HostMem mem{g.maps, g.bytes, 1};
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < g.bands; ++b) CHECK(workgroup<1>(g, i, b, Identity{kLabelIds}, kLabelIds, mem, out.data() + size_t(i) * kLabelIds));
    CHECK(!mem.bad);
    CHECK(std::memcmp(out.data(), ref.data(), total * sizeof(llcomp_mi_label_box)) == 0);
    // ... and pixel by pixel
    std::vector<llcomp_mi_label_box> w(total, label_box_identity(ow, oh));
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t y = 0; y < oh; ++y)
            for (uint32_t x = 0; x < ow; ++x) label_box_update(w[size_t(i) * kLabelIds + maps[(size_t(i) * oh + y) * ow + x]], x, x + 1, y, 1);
    CHECK(std::memcmp(w.data(), out.data(), total * sizeof(llcomp_mi_label_box)) == 0);
    return 0;
}

int run(uint32_t n, uint32_t ow, uint32_t oh, uint32_t off, const std::vector<std::vector<uint16_t>>& lists, const std::vector<uint16_t>& pool,
        std::mt19937& rng) {
    const size_t px = size_t(n) * ow * oh;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[off + 2 * px]);  // (operator new[] aligns to 16; the batch ends where the array ends)
    CHECK(reinterpret_cast<uintptr_t>(buf.get()) % 16 == 0 && off % 2 == 0);
    uint16_t* maps = reinterpret_cast<uint16_t*>(buf.get() + off);
    for (size_t i = 0; i < px;) {  // runs of drawn lengths
        const uint16_t id = pool[rng() % pool.size()];
        for (uint32_t len = 1 + rng() % 12; len && i < px; --len) maps[i++] = id;
    }
    std::vector<uint16_t> ids;
    std::vector<uint32_t> first(1, 0u);
    for (const auto& l : lists) ids.insert(ids.end(), l.begin(), l.end()), first.push_back(uint32_t(ids.size()));
    ids.push_back(0);  // (never NULL)
    uint32_t longest = 0, n_listed = 0;
    CHECK(label_boxes16_check_call(n, ow, oh, ids.data(), first.data(), &longest, &n_listed) == LLCOMP_MI_OK);
    const uint32_t total = first[n], K = label16_capacity(longest);
    CHECK(longest <= K && K <= kLabel16MaxIds && K * kLabel16IdBytes <= 160 * 1024);
    std::vector<llcomp_mi_label_box> ref(total + 1, llcomp_mi_label_box{9, 9, 9, 9, 9}), out(total);
    CHECK(llcomp_mi_label_boxes16_reference(maps, n, ow, oh, ids.data(), first.data(), ref.data()) == LLCOMP_MI_OK && ref[total].count == 9);

    const Label16Table t(n, n_listed, total);
    CHECK(t.bytes <= label16_table_bound(n, total));
    std::unique_ptr<uint8_t[]> table(new uint8_t[t.bytes]);
    label16_table_put(n, ids.data(), first.data(), n_listed, table.get());
    std::vector<uint32_t> tfirst(n + 1), tsamples(n_listed);
    std::vector<uint16_t> tids(total);
    std::memcpy(tfirst.data(), table.get() + t.first_at, 4 * (n + 1));
    if (n_listed) std::memcpy(tsamples.data(), table.get() + t.samples_at, 4 * n_listed);
    if (total) std::memcpy(tids.data(), table.get() + t.ids_at, 2 * total);

    for (uint32_t r = 0; r < total; ++r) out[r] = label_box_identity(ow, oh);  // k_label_boxes16_init
    const LabelGeom g = label_geom<2>(reinterpret_cast<uintptr_t>(maps), n, ow, oh);
    HostMem mem{g.maps, g.bytes, 2};
    for (uint32_t z = 0; z < n_listed; ++z)
        for (uint32_t b = 0; b < g.bands; ++b) {  // one workgroup
            CHECK(tsamples[z] < n && (!z || tsamples[z - 1] < tsamples[z]));
            const uint32_t i = tsamples[z], at = tfirst[i], cnt = tfirst[i + 1] - at;
            CHECK(cnt && cnt <= K && at + cnt <= total);
            std::vector<uint16_t> list(tids.begin() + at, tids.begin() + at + cnt);
            CHECK(workgroup<2>(g, i, b, LabelFinder<const uint16_t*>{list.data(), cnt}, cnt, mem, out.data() + at));
        }
    CHECK(!mem.bad);
    CHECK(!total || std::memcmp(out.data(), ref.data(), total * sizeof(llcomp_mi_label_box)) == 0);
    // ... and pixel by pixel
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = first[i]; j < first[i + 1]; ++j) {
            llcomp_mi_label_box w = label_box_identity(ow, oh);
            for (uint32_t y = 0; y < oh; ++y)
                for (uint32_t x = 0; x < ow; ++x)
                    if (maps[(size_t(i) * oh + y) * ow + x] == ids[j]) label_box_update(w, x, x + 1, y, 1);
            CHECK(std::memcmp(&w, &out[j], sizeof w) == 0);
        }
    return 0;
}

// a strictly ascending list of `count` drawn ids, and a pool of ids for the map: some listed, some not
std::vector<uint16_t> draw_list(uint32_t count, std::mt19937& rng) {
    std::vector<uint16_t> all(65536);
    for (uint32_t i = 0; i < 65536; ++i) all[i] = uint16_t(i);
    std::shuffle(all.begin(), all.end(), rng);
    std::vector<uint16_t> l(all.begin(), all.begin() + count);
    std::sort(l.begin(), l.end());
    return l;
}

int check_refusals() {
    const uint16_t ids[5] = {0, 3, 9, 1, 2}, eq[5] = {0, 3, 3, 1, 2}, desc[5] = {0, 3, 9, 2, 1};
    const uint32_t first[3] = {0, 3, 5}, f1[3] = {1, 3, 5}, dec[3] = {0, 4, 3}, longf[3] = {0, 4097, 4097};
    std::vector<uint16_t> longl(4097);
    for (uint32_t i = 0; i < 4097; ++i) longl[i] = uint16_t(i);
    uint32_t longest = 77, listed = 77;
    CHECK(label_boxes16_check_call(2, 5, 4, ids, first, &longest, &listed) == LLCOMP_MI_OK && longest == 3 && listed == 2);
    CHECK(label_boxes16_check_call(2, 5, 4, nullptr, first) == LLCOMP_MI_BAD_ARGS && label_boxes16_check_call(2, 5, 4, ids, nullptr) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(2, 5, 4, ids, f1) == LLCOMP_MI_BAD_ARGS && label_boxes16_check_call(2, 5, 4, ids, dec) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(2, 5, 4, eq, first) == LLCOMP_MI_BAD_ARGS && label_boxes16_check_call(2, 5, 4, desc, first) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(2, 5, 4, longl.data(), longf) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(0, 5, 4, ids, first) == LLCOMP_MI_BAD_ARGS && label_boxes16_check_call(65536, 5, 4, ids, first) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(2, 0, 4, ids, first) == LLCOMP_MI_BAD_ARGS && label_boxes16_check_call(2, 5, 0, ids, first) == LLCOMP_MI_BAD_ARGS);
    CHECK(label_boxes16_check_call(1, 65536, 65536, ids, first) == LLCOMP_MI_BAD_ARGS);
    std::vector<uint32_t> big(258);
    for (uint32_t i = 0; i < 258; ++i) big[i] = i * 4096;  // 257 lists of 4096: above 2^20 in all, refused before an id is read
    CHECK(label_boxes16_check_call(257, 1, 1, ids, big.data()) == LLCOMP_MI_BAD_ARGS);
    alignas(16) static uint16_t m[64];
    llcomp_mi_label_box out[5];
    std::memset(out, 0x5A, sizeof out);
    CHECK(llcomp_mi_label_boxes16_reference(reinterpret_cast<uint8_t*>(m) + 1, 2, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes16_reference(nullptr, 2, 5, 4, ids, first, out) == LLCOMP_MI_BAD_ARGS);
    CHECK(llcomp_mi_label_boxes16_reference(m, 2, 5, 4, ids, first, nullptr) == LLCOMP_MI_BAD_ARGS && out[0].count == 0x5A5A5A5Au);
    CHECK(label16_capacity(0) == 256 && label16_capacity(256) == 256 && label16_capacity(257) == 1024 && label16_capacity(1024) == 1024);
    CHECK(label16_capacity(1025) == 4096 && label16_capacity(4096) == 4096 && llcomp_mi_label_boxes16_max_ids() == 4096);
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(16016);
    uint32_t rounds = 0;
    const uint32_t B = kLabelBoxRows;
    // widths around a unit's 8 pixels by heights around a band, the maps at every even byte offset: the band's first and last units are
    // shared with the neighbouring band and sample wherever 2 * ow * rows is no multiple of 16
    static const uint32_t ows[7] = {1, 7, 8, 9, 17, 33, 130};
    const uint32_t ohs[5] = {1, B - 1, B, B + 1, 2 * B + 3};
    static const uint16_t high[6] = {0x0001, 0x0101, 0x0201, 0xFF01, 0x0100, 0x0000};
    for (uint32_t ow : ows)
        for (uint32_t oh : ohs)
            for (uint32_t off = 0; off < 16; off += 2, ++rounds) {
                std::vector<uint16_t> pool(high, high + 6);
                std::vector<std::vector<uint16_t>> lists{{0x0001, 0x0101, 0xFF01}, {}, {0x0000, 0x0002, 0x0201, 0xFF00}};
                if (run(3, ow, oh, off, lists, pool, rng)) return 1;
            }
    // the three capacities and their borders
    static const uint32_t counts[7] = {1, 256, 257, 1024, 1025, 4095, 4096};
    for (uint32_t count : counts)
        for (uint32_t off : {0u, 6u}) {
            std::vector<uint16_t> l = draw_list(count, rng), half(l.begin(), l.begin() + count / 2 + 1);
            std::vector<uint16_t> pool;
            for (uint32_t i = 0; i < count; i += 1 + count / 40) pool.push_back(l[i]);
            for (uint32_t i = 0; i < 20; ++i) pool.push_back(uint16_t(rng()));
            if (run(2, 45, B + 3, off, {l, half}, pool, rng)) return 1;
            ++rounds;
        }
    // the dense call: the same widths by the same heights, the byte maps at every byte offset
    for (uint32_t ow : ows)
        for (uint32_t oh : ohs)
            for (uint32_t off = 0; off < 16; ++off, ++rounds)
                if (run8(3, ow, oh, off, rng)) return 1;
    if (check_refusals()) return 1;
    std::printf("ok %u\n", rounds);
    return 0;
}
