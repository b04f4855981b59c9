// host_result.hpp -- how a host call hands its result to the caller, and how it sizes a buffer whose need only the GPU knows.
// Plain C++ (no HIP): hostapi.hip, multidev.hip and container.cpp share it, tests/helpers/host_result_check.cpp runs it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/llcomp_mi.h"

namespace llcomp_mi {

// The result of a call that writes into the caller's buffer (`out`, `out_cap` bytes) or, when out == nullptr, into a malloc'ed one that
// the caller receives through *out_alloc and frees.  out_len may be null (the decodes report a shape instead of a length).
class HostOut {
public:
    HostOut(uint8_t* out, size_t out_cap, uint8_t** out_alloc, size_t* out_len) : out_(out), cap_(out_cap), alloc_(out_alloc), len_(out_len) {}
    ~HostOut() { std::free(fresh_); }  // an allocation that was never committed
    HostOut(const HostOut&) = delete;
    HostOut& operator=(const HostOut&) = delete;

    // n bytes of result: *out_len = n in every case (an OUTPUT_OVERFLOW tells the caller what it takes; nothing is written then), and
    // dst = the caller's buffer or a fresh allocation of n + 1 bytes
    int take(size_t n, uint8_t*& dst) {
        if (len_) *len_ = n;
        if (out_) {
            if (n > cap_) return LLCOMP_MI_OUTPUT_OVERFLOW;
            dst = out_;
            return LLCOMP_MI_OK;
        }
        std::free(fresh_);
        fresh_ = static_cast<uint8_t*>(std::malloc(n + 1));
        if (!fresh_) return LLCOMP_MI_NOMEM;
        dst = fresh_;
        return LLCOMP_MI_OK;
    }
    // the result is complete: an allocation now belongs to the caller
    void commit() {
        if (!fresh_ || !alloc_) return;
        *alloc_ = fresh_;
        fresh_ = nullptr;
    }

private:
    uint8_t* out_;
    size_t cap_;
    uint8_t** alloc_;
    size_t* len_;
    uint8_t* fresh_ = nullptr;
};

// attempt(cap) runs with room for `cap` and returns a status.  It runs at first_cap; if that overflows and the proven bound max_cap is
// larger, once more at max_cap.  The status of the last run comes back.
template <typename Attempt>
int with_overflow_retry(uint64_t first_cap, uint64_t max_cap, Attempt attempt) {
    int rc = attempt(first_cap);
    if (rc == LLCOMP_MI_OUTPUT_OVERFLOW && first_cap < max_cap) rc = attempt(max_cap);
    return rc;
}

}  // namespace llcomp_mi
