// host_result_check.cpp -- the plain-C++ pieces every host call goes through, under a sanitizer: covered_span (container.hpp) against a
// brute-force sum over seeded slice tables, for every tile box of five shapes and with the payload cut short; HostOut and
// with_overflow_retry (host_result.hpp).  Host code only; built and run by tests/test_host_result.py:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I llcomp_amd/csrc
//       tests/helpers/host_result_check.cpp llcomp_amd/csrc/container.cpp
// Prints "ok <boxes>".
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "container.hpp"
#include "host_result.hpp"

using namespace llcomp_mi;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

namespace {

// the span of `box` in a copy of the container's first `len` bytes, held in a heap buffer of exactly that size (a read past it is seen)
int span_of(const std::vector<uint8_t>& whole, size_t len, const uint32_t box[4], PayloadSpan& s) {
    std::vector<uint8_t> cut(whole.begin(), whole.begin() + long(len));
    llcomp_mi_info info;
    CHECK(llcomp_mi_probe(cut.data(), cut.size(), &info) == LLCOMP_MI_OK);
    s = covered_span(info, cut.data(), cut.size(), box);
    return 0;
}

int check_shape_spans(uint32_t w, uint32_t h, uint32_t c, uint32_t tw, uint32_t th, uint32_t planar, std::mt19937& rng, uint64_t& boxes) {
    Geometry g;
    CHECK(make_geometry(g, 1, w, h, c, tw, th, planar));
    const uint32_t n = g.slices_per_frame, planes = planar ? c : 1u;
    const size_t head = LLCOMP_MI_SLICED_HEADER_BYTES + 4 * size_t(n);
    std::vector<uint32_t> lens(n);
    uint64_t payload = 0;
    for (uint32_t i = 0; i < n; ++i) payload += lens[i] = rng() % 4 == 0 ? 0 : rng() % 41;  // (empty slices among them)
    std::vector<uint8_t> whole(head + payload, 0xA5);
    write_sliced_header(whole.data(), g);
    for (uint32_t i = 0; i < n; ++i) put_u32le(whole.data() + LLCOMP_MI_SLICED_HEADER_BYTES + 4 * size_t(i), lens[i]);
    for (uint32_t ty0 = 0; ty0 < g.nty; ++ty0)
        for (uint32_t ty1 = ty0 + 1; ty1 <= g.nty; ++ty1)
            for (uint32_t tx0 = 0; tx0 < g.ntx; ++tx0)
                for (uint32_t tx1 = tx0 + 1; tx1 <= g.ntx; ++tx1) {
                    const uint32_t box[4] = {tx0, ty0, tx1, ty1};
                    // brute force: the first and the last covered slice by testing every slice's tile, then the sums in front of them
                    uint32_t first = n, last = 0;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint32_t tile = i / planes, ty = tile / g.ntx, tx = tile % g.ntx;
                        if (tx < tx0 || tx >= tx1 || ty < ty0 || ty >= ty1) continue;
                        if (first == n) first = i;
                        last = i;
                    }
                    CHECK(first < n);
                    uint64_t begin = 0, end = 0;
                    for (uint32_t i = 0; i <= last; ++i) {
                        if (i < first) begin += lens[i];
                        end += lens[i];
                    }
                    PayloadSpan s;
                    if (span_of(whole, whole.size(), box, s)) return 1;
                    CHECK(s.begin == begin && s.end == end);
                    // the payload cut short: at the span's end, inside it, and before its first byte -- both ends clamp
                    if (span_of(whole, head + end, box, s)) return 1;
                    CHECK(s.begin == begin && s.end == end);
                    if (end > begin) {
                        const uint64_t mid = begin + (end - begin) / 2;
                        if (span_of(whole, head + mid, box, s)) return 1;
                        CHECK(s.begin == begin && s.end == mid);
                    }
                    if (begin > 0) {
                        if (span_of(whole, head + begin - 1, box, s)) return 1;
                        CHECK(s.begin == begin - 1 && s.end == begin - 1);
                    }
                    if (span_of(whole, head, box, s)) return 1;
                    CHECK(s.begin == 0 && s.end == 0);
                    ++boxes;
                }
    return 0;
}

int check_legacy_span() {
    std::vector<uint8_t> s(6 + 37, 0x5A);
    write_legacy_header(s.data(), 19, 13, 3);
    const uint32_t box[4] = {0, 0, 1, 1};
    PayloadSpan p;
    if (span_of(s, s.size(), box, p)) return 1;
    CHECK(p.begin == 0 && p.end == 37);
    if (span_of(s, 6, box, p)) return 1;
    CHECK(p.begin == 0 && p.end == 0);
    return 0;
}

int check_host_out() {
    const size_t n = 29;
    {  // a caller's buffer of exactly n bytes
        std::vector<uint8_t> buf(n, 0xEE);
        uint8_t* alloc = nullptr;
        uint8_t* dst = nullptr;
        size_t len = 7;
        HostOut o(buf.data(), n, &alloc, &len);
        CHECK(o.take(n, dst) == LLCOMP_MI_OK && dst == buf.data() && len == n);
        std::memset(dst, 1, n);
        o.commit();
        CHECK(alloc == nullptr);  // nothing was allocated: nothing is published
    }
    {  // ... of n - 1 bytes: OVERFLOW, the size reported, nothing written (the byte behind the capacity neither)
        std::vector<uint8_t> buf(n, 0xEE);
        uint8_t* dst = nullptr;
        size_t len = 7;
        HostOut o(buf.data(), n - 1, nullptr, &len);
        CHECK(o.take(n, dst) == LLCOMP_MI_OUTPUT_OVERFLOW && dst == nullptr && len == n);
        for (uint8_t b : buf) CHECK(b == 0xEE);
    }
    {  // n = 0: into a caller's buffer without capacity, and allocated (one byte is still a buffer the caller can free)
        uint8_t one = 0xEE;
        uint8_t* dst = nullptr;
        size_t len = 7;
        HostOut o(&one, 0, nullptr, &len);
        CHECK(o.take(0, dst) == LLCOMP_MI_OK && dst == &one && len == 0 && one == 0xEE);
        uint8_t* alloc = nullptr;
        uint8_t* dst2 = nullptr;
        HostOut a(nullptr, 0, &alloc, nullptr);  // (no length wanted: the decodes report a shape)
        CHECK(a.take(0, dst2) == LLCOMP_MI_OK && dst2 != nullptr);
        dst2[0] = 3;
        a.commit();
        CHECK(alloc == dst2);
        std::free(alloc);
    }
    {  // an allocation, committed: n + 1 bytes that now belong to the caller
        uint8_t* alloc = nullptr;
        uint8_t* dst = nullptr;
        size_t len = 0;
        {
            HostOut o(nullptr, 0, &alloc, &len);
            CHECK(o.take(n, dst) == LLCOMP_MI_OK && dst != nullptr && len == n && alloc == nullptr);
            std::memset(dst, 2, n + 1);
            o.commit();
        }
        CHECK(alloc == dst && alloc[n] == 2);
        std::free(alloc);
    }
    {  // an allocation abandoned without commit: freed by the destructor (LeakSanitizer is the assertion), nothing published
        uint8_t* alloc = nullptr;
        uint8_t* dst = nullptr;
        size_t len = 0;
        {
            HostOut o(nullptr, 0, &alloc, &len);
            CHECK(o.take(n, dst) == LLCOMP_MI_OK && dst != nullptr);
            dst[0] = 4;
        }
        CHECK(alloc == nullptr && len == n);
    }
    return 0;
}

int check_retry() {
    std::vector<uint64_t> caps;
    std::vector<int> script;
    auto attempt = [&](uint64_t cap) {
        caps.push_back(cap);
        return script[caps.size() - 1];
    };
    script = {LLCOMP_MI_OK};  // success at first: one call
    CHECK(with_overflow_retry(10, 50, attempt) == LLCOMP_MI_OK && caps == std::vector<uint64_t>({10}));
    caps.clear();
    script = {LLCOMP_MI_OUTPUT_OVERFLOW, LLCOMP_MI_OK};  // overflow, then success at max_cap
    CHECK(with_overflow_retry(10, 50, attempt) == LLCOMP_MI_OK && caps == std::vector<uint64_t>({10, 50}));
    caps.clear();
    script = {LLCOMP_MI_OUTPUT_OVERFLOW, LLCOMP_MI_OUTPUT_OVERFLOW, LLCOMP_MI_OK};  // overflow twice: no third call
    CHECK(with_overflow_retry(10, 50, attempt) == LLCOMP_MI_OUTPUT_OVERFLOW && caps == std::vector<uint64_t>({10, 50}));
    caps.clear();
    script = {LLCOMP_MI_OUTPUT_OVERFLOW, LLCOMP_MI_OK};  // first_cap == max_cap: there is nothing to grow to
    CHECK(with_overflow_retry(50, 50, attempt) == LLCOMP_MI_OUTPUT_OVERFLOW && caps == std::vector<uint64_t>({50}));
    caps.clear();
    script = {LLCOMP_MI_BAD_EXPONENT, LLCOMP_MI_OK};  // another status is passed through at once
    CHECK(with_overflow_retry(10, 50, attempt) == LLCOMP_MI_BAD_EXPONENT && caps == std::vector<uint64_t>({10}));
    caps.clear();
    script = {LLCOMP_MI_OUTPUT_OVERFLOW, LLCOMP_MI_NOMEM};  // the second attempt's status is the call's
    CHECK(with_overflow_retry(10, 50, attempt) == LLCOMP_MI_NOMEM && caps == std::vector<uint64_t>({10, 50}));
    return 0;
}

}  // namespace

int main() {
    std::mt19937 rng(20261018);
    uint64_t boxes = 0;
    const uint32_t shapes[][6] = {{19, 13, 3, 8, 4, 1}, {100, 44, 3, 32, 16, 0}, {300, 12, 3, 64, 1, 1}, {16, 16, 1, 16, 16, 0}, {1, 1, 1, 1, 1, 0}};
    for (const auto& s : shapes)
        if (check_shape_spans(s[0], s[1], s[2], s[3], s[4], s[5], rng, boxes)) return 1;
    if (check_legacy_span() || check_host_out() || check_retry()) return 1;
    std::printf("ok %llu\n", static_cast<unsigned long long>(boxes));
    return 0;
}
