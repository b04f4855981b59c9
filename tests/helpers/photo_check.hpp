// photo_check.hpp -- what the stand-alone checks of the photometric chains share (photo_plan_check.cpp, photo_area_check.cpp,
// photo_sharp_check.cpp): the CHECK macro and the chains on the heap.  Each program keeps its own generator of ops and its own rounds,
// so its seeds, the order of its draws and the count it prints stay its own.
#pragma once
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "../../include/llcomp_mi.h"

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

// Chains on the heap, exactly n of them: a read past the last one is the sanitizer's to report.  Every byte is 0xEE first (what lies
// behind a chain's ops is never read as an op); a chain draws its length, unless all are empty, and then its ops from op(rng).
template <class Op>
std::unique_ptr<llcomp_mi_photo_chain[]> heap_chains(uint32_t n, std::mt19937& rng, Op&& op, bool all_empty = false) {
    std::unique_ptr<llcomp_mi_photo_chain[]> ch(new llcomp_mi_photo_chain[n]);
    for (uint32_t i = 0; i < n; ++i) {
        std::memset(&ch[i], 0xEE, sizeof ch[i]);
        ch[i].n_ops = all_empty ? 0 : rng() % (LLCOMP_MI_PHOTO_MAX_OPS + 1);
        for (uint32_t k = 0; k < ch[i].n_ops; ++k) ch[i].ops[k] = op(rng);
    }
    return ch;
}
