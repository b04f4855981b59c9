// slice_kernels.hip -- the serial part of the llcomp coding path on gfx950: binarisation, the adaptive 128-state
// binary models and the 16-bit carry-propagating range coder (llcomp.hpp:33-127, 166-247, 283-293, 439-449,
// 486-530), one LANE per slice, 1..64 independent slices per wavefront, all lanes in lockstep per coding phase.
//
// What shapes the code (measured with rocprofv3 SQ counters, profiles/):
//   * the kernels are instruction-issue bound, so the cost of a bin is its INSTRUCTION COUNT (and which of them are
//     4-cycle operations): the coded bit is kept in VCC so that selects are 2-cycle v_cndmask_e32, the decoder refills
//     from a 64-bit register window inside one exec-masked region and tops the window up once per sample, the
//     encoder renormalises in 6 instructions with eager carry propagation, its output bytes go to a per-lane LDS
//     staging area that is filled linearly and flushed 16 bytes at a time;
//   * the model table lives in LDS as 8-byte entries {next0, P, address of next0's entry | next1, P, address of next1's
//     entry} (absolute LDS addresses, added while the table is copied in): the 8 entries of a context are requested
//     together when the context is known; a run of bins on one slot walks from entry to entry with one right shift by a
//     constant per bin and no base to add, and the encoder (whose bins are known in advance) requests a successor before
//     it codes the bin that leads there;
//   * 1-row slices (tile_h == 1) can only ever reach 3 contexts (llcomp.hpp:417-429 with h == 0: hash =
//     605*quant5(L-l)), so their 24 state bytes stay in LDS and the kernel touches no state memory in HBM at all;
//     taller slices keep a private 63 KB table (u64 per context) in HBM, fetched one context per sample -- or in
//     LDS when a wavefront carries a single slice (LDSTAB);
//   * for the 1-row-slice kernels (the headline path) the per-sample coding is hand-written gfx950 assembly
//     (enc_rows_asm.hpp, dec_rows_asm.hpp: nested lane sets, outcomes taken in place, carry-out loop exits); the C++
//     below states the same algorithm, serves every other kernel family and the decoder's checked replay, and is what
//     the blocks are A/B-tested against (LLMI_ASM_ENC / LLMI_ASM_DEC = 0).
#include <algorithm>
#include <type_traits>

#include "device_common.hpp"
#include "kernels.hpp"

// The encoder's sample of the 1-row-slice kernels as one hand-written block (enc_rows_asm.hpp); 0 = hipcc's code everywhere.
#ifndef LLMI_ASM_ENC
#define LLMI_ASM_ENC 1
#endif
#if LLMI_ASM_ENC
#include "enc_rows_asm.hpp"
#endif
// The decoder's fast path of a sample of the 1-row-slice kernels as one hand-written block (dec_rows_asm.hpp); 0 = hipcc's code.
#ifndef LLMI_ASM_DEC
#define LLMI_ASM_DEC 1
#endif
#if LLMI_ASM_DEC
#include "dec_rows_asm.hpp"
#endif

namespace llcomp_mi {

namespace {

// ---- diagnostic build only (make probe: -DLLMI_CLOCK_PROBE, a separate library that is never shipped or benchmarked) -----
// In-kernel shader clock of the two slice kernels, the way /opt/skills/guides/MI355X_MICROARCH.md prescribes: every
// wavefront stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) when it starts coding and when it is done; the
// quotient of the differences x 100 MHz is the clock it ran at.  The stamps go to a buffer of their own that no kernel
// reads; no output depends on them.  The product build contains none of this.
#ifdef LLMI_CLOCK_PROBE
constexpr uint32_t kProbeSlots = 1u << 15;
__device__ unsigned long long g_probe[2][kProbeSlots][2];  // [kernel: 0 encode / 1 decode][block & mask][shader ticks, 100 MHz ticks]
struct ProbeStamp {
    unsigned long long t, r;
    __device__ __forceinline__ void start() {
        t = __builtin_amdgcn_s_memtime();
        r = __builtin_amdgcn_s_memrealtime();
    }
    __device__ __forceinline__ void stop(int kernel) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            g_probe[kernel][blockIdx.x & (kProbeSlots - 1)][0] = t1 - t;
            g_probe[kernel][blockIdx.x & (kProbeSlots - 1)][1] = r1 - r;
        }
    }
};
#define LLMI_PROBE_START() ProbeStamp probe_stamp; probe_stamp.start()
#define LLMI_PROBE_STOP(kernel) probe_stamp.stop(kernel)
// Where a sample of the 2-D decoder spends its shader cycles: [block & mask][context arithmetic, bank fetch (issue -> data),
// decoding, write-back + neighbour rotation]; every stamp drains the wavefront's LDS / scalar-memory queue (s_memtime is a
// scalar-memory read), so the four parts are serialised -- a decomposition of the chain, not of the undisturbed kernel.
__device__ unsigned long long g_probe_parts[kProbeSlots][4];
struct PartClock {
    unsigned long long acc[4] = {0, 0, 0, 0}, last;
    __device__ __forceinline__ void start() { last = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void lap(int part) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[part] += now - last;
        last = now;
    }
    __device__ __forceinline__ void flush() {
        if (threadIdx.x == 0)
            for (int k = 0; k < 4; ++k) g_probe_parts[blockIdx.x & (kProbeSlots - 1)][k] = acc[k];
    }
};
#define LLMI_PARTS_DECL() PartClock part_clock
#define LLMI_PARTS_START() part_clock.start()
#define LLMI_PARTS_LAP(part) part_clock.lap(part)
#define LLMI_PARTS_FLUSH() part_clock.flush()
#else
#define LLMI_PROBE_START() do {} while (0)
#define LLMI_PROBE_STOP(kernel) do {} while (0)
#define LLMI_PARTS_DECL() do {} while (0)
#define LLMI_PARTS_START() do {} while (0)
#define LLMI_PARTS_LAP(part) do {} while (0)
#define LLMI_PARTS_FLUSH() do {} while (0)
#endif

// ---- model table ------------------------------------------------------------------------------------------------
// entry = entry_lo | entry_hi << 32 (tables.hpp), always moved as ONE 64-bit LDS access
using entry_t = unsigned long long;
struct EntryTable {
    entry_t v[128];
};
constexpr EntryTable make_entries() {
    EntryTable t{};
    for (uint32_t s = 0; s < 128; ++s) t.v[s] = entry_t(entry_lo(s)) | (entry_t(entry_hi(s)) << 32);
    return t;
}
__constant__ EntryTable c_entries = make_entries();

// The copy in LDS carries ABSOLUTE LDS byte addresses in the offset fields of its entries (tables.hpp has them relative to
// the table): the table's own LDS address is added to both while it is copied in.  Walking from entry to entry is then a
// right shift and a load with no base to add -- whether the table sits at a fixed address the compiler knows (static LDS) or
// in the dynamic block, where it only knows a symbol (and would add it with a 4-cycle SDWA add per access).
using lds_u8_ptr = __attribute__((address_space(3))) uint8_t*;
using lds_entry_ptr = const __attribute__((address_space(3))) unsigned long long*;
__device__ __forceinline__ uint32_t lds_address(const void* p) { return uint32_t(uintptr_t((lds_u8_ptr) reinterpret_cast<const uint8_t*>(p))); }
__device__ __forceinline__ void load_table(entry_t* tab) {
    const unsigned long long rebase = (unsigned long long)lds_address(tab) * 0x0001000000010000ull;
    for (uint32_t i = threadIdx.x; i < 128; i += blockDim.x) tab[i] = c_entries.v[i] + rebase;
    __syncthreads();
}
// the entry at an absolute LDS address taken from a half-entry / a wide row bank
__device__ __forceinline__ entry_t lds_entry(uint32_t address) { return *reinterpret_cast<lds_entry_ptr>(uintptr_t(address)); }

// s_waitcnt vmcnt(0) as an instruction hipcc's own wait-count pass sees (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt and
// lgkmcnt left at their maxima): everything the wavefront has sent to vector memory is done afterwards, and the compiler knows it.
__device__ __forceinline__ void drain_vector_memory() { __builtin_amdgcn_s_waitcnt(0x0F70); }

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 0xFF; }
__device__ __forceinline__ uint32_t consume_here(uint32_t v);
template <int SLOT>
__device__ __forceinline__ uint32_t slot_state(const uint32_t* bank) {
    return byte_of(bank[SLOT >> 2], SLOT & 3);
}
template <int SLOT>
__device__ __forceinline__ void set_slot_state(uint32_t* bank, uint32_t ns) {
    constexpr int W = SLOT >> 2, SH = (SLOT & 3) * 8;
    bank[W] = (bank[W] & ~(0xFFu << SH)) | (ns << SH);
}
// The 8 state bytes of the context being coded (slot k = byte k).  For 1-row slices they live in LDS ([context][lane]):
// a new state is then ONE byte store and the words below are a read-only copy; otherwise the words are updated and
// written back by the caller.
struct Bank {
    uint32_t w[4];  // (w[2], w[3]: only the decoder's wide row banks, below)
    uint8_t* lds;
};
// Row banks in LDS: [context][word 0 / 1][lane] dwords, so that the 64 lanes of a byte store (or of a word read) sit in 64
// consecutive dwords -- conflict-free.  (As [context][lane] 8-byte entries every byte store of a new state was a 2-way
// bank conflict: 28 of the ~150 LDS cycles of a sample.)  State byte k of a lane: word k / 4, 256 bytes further on.
constexpr uint32_t kRowBankWords = 3 * 2 * 64;
[[maybe_unused]] __device__ __forceinline__ constexpr uint32_t rowbank_byte(int slot) { return uint32_t(slot >> 2) * 256u + uint32_t(slot & 3); }
// The DECODER's row banks are wide: 16 bits per slot, holding the TABLE OFFSET of the slot's state (8 * state, what the upper
// half of a half-entry carries anyway) instead of the state byte -- [context][word 0..3][lane] dwords, slot k in half k & 1 of
// word k / 2.  The address of a slot's entry is then a mask or a right shift by a constant (2-cycle operations) where the
// byte form needs an SDWA shift (4 cycles), eight times per sample; a new state is one 16-bit store straight out of the
// half-entry's upper half.  (4 KB of LDS per wavefront with the table: fits eight wavefronts per SIMD.  The encoder's
// staging area leaves no room for the same there.)
constexpr uint32_t kWideBankWords = 3 * 4 * 64;
__device__ __forceinline__ constexpr uint32_t widebank_byte(int slot) { return uint32_t(slot >> 1) * 256u + uint32_t(slot & 1) * 2u; }
template <int SLOT>
__device__ __forceinline__ uint32_t wide_offset(const uint32_t (&w)[4]) {
    return (SLOT & 1) ? (w[SLOT >> 1] >> 16) : (w[SLOT >> 1] & 0xFFFFu);
}
template <int SLOT, bool INLDS>
__device__ __forceinline__ void put_state(Bank& b, uint32_t ns) {  // ns: new state in byte 0
    if constexpr (INLDS) b.lds[rowbank_byte(SLOT)] = uint8_t(ns);
    else set_slot_state<SLOT>(b.w, ns & 0xFF);
}
// successor state / successor probability of entry e for the coded bit
__device__ __forceinline__ uint32_t prob_of(entry_t e) { return byte_of(uint32_t(e), 1); }
// half of the entry that belongs to the coded bit: byte0 = successor state, upper half = byte offset of its entry
__device__ __forceinline__ uint32_t successor(entry_t e, bool bit) { return bit ? uint32_t(e >> 32) : uint32_t(e); }

// State tables in HBM (2-D tiles with several slices per wavefront) are NOT cleared per call: that was 6 GB of memset per
// direction for 16 frames at 64x64 tiles, beside kernels that are bound by their own HBM traffic.  A state byte uses
// 7 bits (128 states), so the eight spare top bits of a bank carry the GENERATION of the call that wrote it: a bank whose
// tag is not this call's generation is stale and reads as eight zero states -- exactly what a cleared table holds.  The
// host clears the table for real once per 255 calls (generation 0 = cleared memory, never a call's tag).
// The 8 entries of one context.  `all` = request slots 1..7 together with slot 0 (worth it when most residuals
// are non-zero); otherwise they are requested after the zero flag turned out 0.
struct Entries {
    entry_t e0, e1, e2, e3, e4, e5, e6, e7;
    template <int SLOT>
    __device__ __forceinline__ entry_t get() const {
        if constexpr (SLOT == 0) return e0;
        else if constexpr (SLOT == 1) return e1;
        else if constexpr (SLOT == 2) return e2;
        else if constexpr (SLOT == 3) return e3;
        else if constexpr (SLOT == 4) return e4;
        else if constexpr (SLOT == 5) return e5;
        else if constexpr (SLOT == 6) return e6;
        else return e7;
    }
};
__device__ __forceinline__ void fetch_slot0(Entries& E, const uint32_t* bank, const entry_t* tab) {
    E.e0 = tab[slot_state<0>(bank)];
}
__device__ __forceinline__ void fetch_rest(Entries& E, const uint32_t* bank, const entry_t* tab) {
    E.e1 = tab[slot_state<1>(bank)];
    E.e2 = tab[slot_state<2>(bank)];
    E.e3 = tab[slot_state<3>(bank)];
    E.e4 = tab[slot_state<4>(bank)];
    E.e5 = tab[slot_state<5>(bank)];
    E.e6 = tab[slot_state<6>(bank)];
    E.e7 = tab[slot_state<7>(bank)];
}

// the entry of the successor that half-entry `nx` names: its LDS address sits in the upper half (load_table)
__device__ __forceinline__ entry_t entry_at(const entry_t*, uint32_t nx) { return lds_entry(nx >> 16); }

// Event counters (llcomp_mi_codec_get_counters; kernels.hpp kCtr*): a lane counts in a register, the wavefront adds the sum of its
// active lanes with ONE atomic -- and only when some lane has something to report (replays and carry-backs are rare).  Convergent
// v_readlane sum over the lanes that are active here, as for the group sums below.
__device__ __forceinline__ void publish_count(unsigned long long* counters, uint32_t which, uint32_t mine) {
    if (!counters) return;
    unsigned long long live = __ballot(mine != 0);
    if (live == 0) return;
    unsigned long long sum = 0;
    const unsigned long long all = __ballot(1);
    while (live) {
        const int lane = __builtin_ctzll(live);
        sum += uint32_t(__builtin_amdgcn_readlane(mine, lane));
        live &= live - 1;
    }
    if (threadIdx.x == uint32_t(__builtin_ctzll(all))) atomicAdd(counters + which, sum);
}

// How the sample loops of a 1-row-slice kernel form L - l, the difference behind the context (llcomp.hpp:417-429 with h == 0).  The
// model is fixed per launch, so it is a template flag of the kernels (SMALL): no loop carries a mask for it.
constexpr int kModelSmall = 0;  // LargeModel = false -- and the first samples of a slice, which have no L: no difference, context 0
constexpr int kModelLarge = 1;  // the difference as it is
constexpr std::integral_constant<int, kModelSmall> no_model{};

// ================================================ ENCODER ========================================================
// Range encoder of one lane (llcomp.hpp:33-89).  Output bytes are staged in a per-lane 32-byte LDS area and leave for
// HBM as aligned 16-byte stores.
//
// Carries.  The reference holds one byte back (outstanding_byte) plus a count of undecided 0xFF bytes behind it
// (outstanding_count) and writes them once it knows whether a carry reaches them (llcomp.hpp:40-57).  That is long
// addition done lazily; the bytes it finally emits are those of the exact sum.  Here the same sum is formed eagerly:
// only ONE byte is held back, an undecided 0xFF is emitted like any other byte, and in the rare event that a carry
// arrives while the held byte is 0xFF (about one renormalisation in a thousand) the carry is propagated into the bytes
// already written -- in the LDS staging area or, behind the last flush, in this lane's own units in HBM.  The common path of a
// renormalisation is then seven instructions with a single test.  (The reference's `outstanding_byte + 1` cannot
// overflow a byte: low < 0x1FE00 always, so a byte 0xFF is never held when low >= 0x10000 produced it.)
// `pos` starts at -1: the reference emits nothing for its first renormalisation (outstanding_byte == -1); here a dummy
// byte goes to position -1 instead, which is the same thing without the special case.
struct RangeEnc {
    uint32_t low;     // bits 0..15: the reference's low; bits 16..23: the byte held back (its outstanding_byte), so a
                      // carry out of the low 16 bits lands in the held byte by itself; bit 24: that byte overflowed
    uint32_t range;
    uint32_t wp;      // LDS byte address the next output byte goes to (this lane's staging area, below)
    uint32_t base;    // LDS byte address of this lane's staging area; bytes produced so far = flushed + (wp - base)
    uint8_t* area;    // the same as a pointer (into the block's __shared__ array: the compiler emits LDS accesses)
    int32_t flushed;  // bytes already stored to HBM (multiple of 16)
    uint8_t* out;     // this lane's first 16-byte unit in the stream lane order array
    uint8_t* gout;    // WAVE-UNIFORM: first unit of the lane group (all lanes of a wavefront belong to one group) ...
    uint32_t oofs;    // ... and the byte offset from there of the unit the next flush stores: one scalar-base store and one
    uint32_t ostep;   //     2-cycle add per flush instead of 64-bit address arithmetic (ostep = 16 << lane_shift, a vector value)
    int32_t cap;
    uint32_t shift;   // lane_shift
    uint32_t carries; // event counter: carries that went on into bytes already stored to HBM (kCtrEncCarryBacks)
};
// Staging area: 32 bytes per lane, filled LINEARLY -- the renormalisation stores its byte at `wp` and adds one, no index
// arithmetic (round 2 kept a ring and paid a v_and_or per renormalisation, which the wavefront executes for every bin
// because some lane renormalises in nearly every bin).  The reference's "no byte on the first renormalisation" is a dummy byte
// at position -1, i.e. the last byte of the neighbouring lane's area (16 bytes of padding in front of lane 0).
// Two flush policies, both once per sample and in front of its coding:
//   * every sample (enc_flush16 under `wp >= base + 16`): a lane enters a sample with at most 15 bytes, a sample adds at most
//     kSampleBytesMax, so 28 of the 32 bytes are ever used -- the 2-D, snapshot and table-in-HBM families;
//   * in batches (enc_flush_batched, the 1-row-slice kernels): the wavefront enters the flush region only when SOME lane holds at
//     least kFlushAt bytes, and every lane with a whole unit then stores one.  INVARIANT: a lane enters a sample with at most
//     kFlushAt - 1 bytes (below the threshold, or at most kStageFill - 16 behind its flush) and leaves it with at most
//     kStageFill = kFlushAt - 1 + kSampleBytesMax.  kStageFill stops ONE short of kStageBytes: the area's last byte is where the
//     next lane's dummy byte lands, whenever that lane renormalises first -- a flat row does so many samples after a noisy
//     neighbour has filled its area, so the byte can never hold output.  (kFlushAt = 20 would use all 32.)
constexpr int kStageBytes = 32;
constexpr int kStagePad = 16;
constexpr int kSampleBytesMax = 13;  // bytes one sample can add: one per bin at the most (putSymbol<true,4,6,7> on 8-bit planes)
constexpr int kFlushAt = 19;
constexpr int kStageFill = kFlushAt - 1 + kSampleBytesMax;
static_assert(kStageFill <= kStageBytes - 1, "the staging area's last byte belongs to the next lane's dummy byte");
static_assert(kStageFill - 16 <= kFlushAt - 1 && kFlushAt >= 16, "one unit per lane and flush event must be enough");
__device__ __forceinline__ int32_t enc_pos(const RangeEnc& e) { return e.flushed + int32_t(e.wp - e.base); }
// stream lane order: unit u of this lane is (u << lane_shift) units further on
__device__ __forceinline__ uint8_t* unit_byte(RangeEnc& e, uint32_t k) {
    return e.out + ((size_t(k >> 4) << (e.shift + 4)) + (k & 15));
}
// the first 16 staged bytes -> HBM, the rest moves down
__device__ __forceinline__ void enc_flush16(RangeEnc& e) {
    uint32_t* a = reinterpret_cast<uint32_t*>(e.area);
    uint4 v, rest;
    v.x = a[0]; v.y = a[1]; v.z = a[2]; v.w = a[3];
    rest.x = a[4]; rest.y = a[5]; rest.z = a[6]; rest.w = a[7];
    // `flushed` is a multiple of 16: its unit starts (flushed << lane_shift) bytes after the lane's first unit
    if (e.flushed + 16 <= e.cap) *reinterpret_cast<uint4*>(e.gout + e.oofs) = v;
    e.oofs += e.ostep;
    a[0] = rest.x; a[1] = rest.y; a[2] = rest.z; a[3] = rest.w;
    e.flushed += 16;
    e.wp -= 16;
}
// The batched policy (see the staging area): one compare and one wave-uniform branch per sample outside the region.
__device__ __forceinline__ void enc_flush_batched(RangeEnc& e) {
    if (__builtin_amdgcn_ballot_w64(e.wp >= e.base + uint32_t(kFlushAt)) != 0) {
        uint32_t w = e.wp + uint32_t(kFlushAt - 16);
        asm volatile("" : "+v"(w));  // (pinned inside the region: hipcc otherwise folds both tests into one exec mask, two compares a sample)
        if (w >= e.base + uint32_t(kFlushAt)) enc_flush16(e);
    }
}
// rare: +1 into the bytes before position `pos` (the byte at `pos` itself just wrapped from 0xFF to 0x00)
__device__ __forceinline__ void enc_carry_back(RangeEnc& e) {
    for (int32_t k = enc_pos(e) - 1; k >= 0; --k) {
        uint32_t v;
        if (k >= e.flushed) {
            uint8_t& r = e.area[k - e.flushed];
            v = r;
            r = uint8_t(v + 1);
        } else if (k < e.cap) {
            uint8_t* g = unit_byte(e, uint32_t(k));
            if (k == e.flushed - 1) ++e.carries;  // the carry leaves the staging area
            v = *g;
            *g = uint8_t(v + 1);
        } else {
            break;  // beyond the scratch capacity: the slice is reported as overflowed anyway
        }
        if (v != 0xFF) break;
    }
}
// Renormalisation (body of the reference's `while (range < 0x100)`: one step always suffices because range >= 7 after
// put() and == 0xFF in finish()).  One exec-masked region for the lanes that renormalise: a store and four instructions.
// The held byte is stored straight out of bits 16..23 of `low` (ds_write_b8_d16_hi), then the 16 low bits move up by 8:
// the old bits 8..15 become the new held byte.
__device__ __forceinline__ void enc_renorm(RangeEnc& e) {
    if (e.range < 0x100) {
        asm volatile("ds_write_b8_d16_hi %0, %1" : : "v"(e.wp), "v"(e.low) : "memory");
        // held was 0xFF and a carry arrived: rare, so the test is a wave-uniform branch (no exec bookkeeping when no
        // lane needs it)
        const bool wrapped = e.low > 0xFFFFFFu;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(wrapped) != 0, 0)) {
            if (wrapped) enc_carry_back(e);
        }
        ++e.wp;
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
            : "=v"(e.low) : "v"(8u), "v"(e.low));  // (low & 0xFFFF) << 8
        e.range <<= 8;
    }
}
// `m` = all ones when the coded bit is 1, zero when it is 0 (llcomp.hpp:60-73)
__device__ __forceinline__ void enc_core(RangeEnc& e, uint32_t P, uint32_t m) {
    const uint32_t r1 = __umul24(e.range, P) >> 8;
    const uint32_t r0 = e.range - r1;
    e.low += r0 & m;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(e.range) : "v"(m), "v"(r1), "v"(r0));  // m ? r1 : r0 (see successor_m)
    enc_renorm(e);
}
__device__ __forceinline__ uint32_t successor_m(entry_t e, uint32_t m) {  // successor() on a mask: ONE v_bfi_b32
    uint32_t r;  // (hipcc splits the bit-select into not/and/and/or when both halves are live: four ops instead of one)
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(uint32_t(e >> 32)), "v"(uint32_t(e)));
    return r;
}
// One bin of a run on one slot (unary tail, mantissa tail): codes the top bit of `bits`, shifts `bits` left and returns
// the half of entry `cur` that belongs to the coded bit.  The shift is an add with carry-out, so the bit arrives in VCC
// and the three selects are 2-cycle v_cndmask_e32 (a mask in a VGPR costs a 4-cycle v_bfi per select).
__device__ __forceinline__ uint32_t enc_step_msb(RangeEnc& e, uint32_t& bits, entry_t cur) {
    uint32_t off, r1;  // off: table offset (state * 8) of the successor
    unsigned long long saved_exec;
    // Every lane takes the bit-0 outcome (range -= r1, successor = low half of the entry); the lanes whose bit is 1
    // then patch it up under exec = VCC: low += r0, range = r1, successor = high half.  Eight vector instructions; the
    // two scalar ones ride along for free (the kernels are bound by VALU issue).
    asm("v_add_co_u32_e32 %[bits], vcc, %[bits], %[bits]\n\t"
        "v_mul_u32_u24_sdwa %[r1], %[lo], %[range] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_lshrrev_b32_e32 %[r1], 8, %[r1]\n\t"
        "v_sub_u32_e32 %[range], %[range], %[r1]\n\t"
        "v_lshrrev_b32_e32 %[off], 16, %[lo]\n\t"
        "s_and_saveexec_b64 %[save], vcc\n\t"
        "v_add_u32_e32 %[low], %[low], %[range]\n\t"
        "v_mov_b32_e32 %[range], %[r1]\n\t"
        "v_lshrrev_b32_e32 %[off], 16, %[hi]\n\t"
        "s_mov_b64 exec, %[save]"
        : [bits] "+v"(bits), [range] "+v"(e.range), [low] "+v"(e.low), [off] "=&v"(off), [r1] "=&v"(r1), [save] "=&s"(saved_exec)
        : [lo] "v"(uint32_t(cur)), [hi] "v"(uint32_t(cur >> 32))  // byte 1 of lo = probability of this state
        : "vcc");
    enc_renorm(e);
    return off;
}
// a slot that is coded at most once per sample; the bit as a mask (all ones / zero) ...
template <int SLOT, bool INLDS>
__device__ __forceinline__ void enc_once_m(RangeEnc& e, Bank& bank, const Entries& E, uint32_t m) {
    enc_core(e, prob_of(E.get<SLOT>()), m);
    put_state<SLOT, INLDS>(bank, successor_m(E.get<SLOT>(), m));
}
// ... or as a condition.  With the states in LDS every lane first takes the bit-0 outcome (range -= r1, successor =
// low half of the entry, stored straight away); the lanes whose bit is 1 then patch up inside one exec-masked region:
// low += r0, range = r1, store the other successor.  Five vector instructions instead of seven selects and adds.
template <int SLOT, bool INLDS>
__device__ __forceinline__ void enc_once(RangeEnc& e, Bank& bank, const Entries& E, bool bit) {
    const entry_t en = E.get<SLOT>();
    const uint32_t r1 = __umul24(e.range, prob_of(en)) >> 8;
    if constexpr (INLDS) {
        e.range -= r1;
        put_state<SLOT, true>(bank, uint32_t(en));
        if (bit) {
            asm volatile("" : "+v"(e.low));  // (keeps hipcc from turning this region back into selects)
            e.low += e.range;
            e.range = r1;
            put_state<SLOT, true>(bank, uint32_t(en >> 32));
        }
        enc_renorm(e);
    } else {
        const uint32_t r0 = e.range - r1;
        e.low += bit ? r0 : 0u;
        e.range = bit ? r1 : r0;
        const uint32_t ns = successor(en, bit);
        enc_renorm(e);
        put_state<SLOT, INLDS>(bank, ns);
    }
}

// putSymbol<true,4,6,7> (llcomp.hpp:166-206).  All lanes walk the phases together, so the slot of every bin is a
// compile-time constant.
template <bool ALL, bool INLDS>
__device__ __forceinline__ void enc_residual(RangeEnc& e, Bank& bank, const entry_t* tab, int res) {
    Entries E;
    fetch_slot0(E, bank.w, tab);
    if (ALL) fetch_rest(E, bank.w, tab);
    enc_once<0, INLDS>(e, bank, E, res == 0);
    if (res != 0) {
        if (!ALL) fetch_rest(E, bank.w, tab);
        const uint32_t a = uint32_t(res < 0 ? -res : res);
        const int ex = 31 - __clz(int(a));
        enc_once<1, INLDS>(e, bank, E, ex > 0);
        if (ex > 0) {
            enc_once<2, INLDS>(e, bank, E, ex > 1);
            if (ex > 1) {
                enc_once<3, INLDS>(e, bank, E, ex > 2);
                if (ex > 2) {
                    // Unary tail on slot 4: (ex - 3) ones, then a zero.  The lanes that stay in the loop are exactly
                    // the lanes that code a 1, so the loop's own exec mask does the selecting (see the decoder): every
                    // lane takes the bit-0 outcome (range -= r1), a lane whose run is over leaves, the others add r0
                    // to low, take r1 as the range, renormalise and move on to the high half's successor.  The
                    // iteration index is wave-uniform: "is this bin a one" is a single compare.
                    entry_t cur = E.e4;
                    const uint32_t ones = uint32_t(ex - 3);
                    uint32_t r1 = __umul24(e.range, prob_of(cur)) >> 8;
                    e.range -= r1;
                    for (uint32_t i = 0; i < ones; ++i) {  // (rotated: one compare per bin)
                        // the successor on a 1 is known before this bin is coded: its entry is requested first and has
                        // the whole renormalisation to arrive (the state chain does not depend on low / range)
                        cur = entry_at(tab, uint32_t(cur >> 32));
                        e.low += e.range;
                        e.range = r1;
                        enc_renorm(e);
                        r1 = __umul24(e.range, prob_of(cur)) >> 8;
                        e.range -= r1;
                    }
                    enc_renorm(e);
                    put_state<4, INLDS>(bank, uint32_t(cur));
                }
            }
            enc_once_m<5, INLDS>(e, bank, E, uint32_t(__builtin_amdgcn_sbfe(int(a), uint32_t(ex - 1), 1u)));
            if (ex > 1) {  // mantissa tail on slot 6, MSB first
                entry_t cur = E.e6;
                uint32_t nx;
                // remaining mantissa bits left-aligned, followed by a sentinel 1: the loop needs no counter
                uint32_t bits = ((a << 1) | 1u) << (32 - ex);
                do {
                    nx = enc_step_msb(e, bits, cur);  // successor's LDS address
                    cur = lds_entry(nx);
                } while (bits != 0x80000000u);
                put_state<6, INLDS>(bank, (nx - lds_address(tab)) >> 3);
            }
        }
        enc_once<7, INLDS>(e, bank, E, res < 0);
    }
}

template <bool BATCHED>
__device__ __forceinline__ void enc_finish_and_count(RangeEnc& e, int32_t& n_bytes) {  // llcomp.hpp:75-81
    // the batched policy leaves up to kStageFill bytes behind the last sample: room for the two bytes below
    if constexpr (BATCHED) {
        if (e.wp >= e.base + 16) enc_flush16(e);
    }
    e.range = 0xFF; e.low += 0xFF; enc_renorm(e);
    e.range = 0xFF; enc_renorm(e);
    n_bytes = enc_pos(e);
    while (int32_t(e.wp - e.base) > 0) enc_flush16(e);  // tail: whole 16-byte groups, the slack is scratch
}

// Lane-per-slice encoder.  ROWS: every slice is one row high (its three contexts' states live in LDS).  `lpw` = slices per
// wavefront (1..64).
// LDSTAB: one slice per wavefront (a lone whole-image stream, a handful of big tiles) -- its 63 KB state table fits in
// LDS, which takes the HBM round trip of every context fetch off the serial chain.
extern __shared__ __attribute__((aligned(32))) unsigned char dyn_lds[];
// LDS of the 1-row-slice encoder with the hand-written sample: everything sits in the dynamic block, which starts at LDS
// address 0 when a kernel has no static LDS -- the block addresses the model table with offsets relative to 0 (the kernel
// checks that and refuses to run otherwise).
constexpr uint32_t kRowsEncTabOff = 0, kRowsEncStageOff = 1024, kRowsEncBankOff = 1024 + 16 + 32 * 64;
constexpr uint32_t kRowsEncLdsBytes = kRowsEncBankOff + 3 * 64 * 8;
// rare: a carry that the block could not finish inside the staging area goes on into the bytes already stored to HBM
// (`out`: the lane's first unit, RangeEnc::out -- a parameter, so that a sample loop which can form it on the spot need not hold the
// pointer in a register pair for the whole slice)
[[maybe_unused]] __device__ __forceinline__ void enc_carry_back_flushed(RangeEnc& e, uint8_t* out) {
    if (e.flushed > 0 && e.flushed - 1 < e.cap) ++e.carries;
    for (int32_t k = e.flushed - 1; k >= 0; --k) {
        if (k >= e.cap) break;  // beyond the scratch capacity: the slice is reported as overflowed anyway
        uint8_t* g = out + ((size_t(uint32_t(k) >> 4) << (e.shift + 4)) + (uint32_t(k) & 15));  // unit_byte()
        const uint32_t v = *g;
        *g = uint8_t(v + 1);
        if (v != 0xFF) break;
    }
}
template <bool LDSTAB>
__device__ __forceinline__ void clear_lds_states() {
    if constexpr (LDSTAB) {
        unsigned long long* t = reinterpret_cast<unsigned long long*>(dyn_lds);
        for (uint32_t i = threadIdx.x; i < uint32_t(kContexts); i += blockDim.x) t[i] = 0;
    }
}
// SNAP: slices of several rows whose states were replayed ahead of the coder (snapshot_kernels.hip): `sym` is then the array of
// folded residuals (i16) and `states` the array of state banks as they stand BEFORE each sample (u64), both in stream order
// and in the piece layout [lane group][piece][lane][32 bytes] -- the kernel reads them front to back and touches no table.
// SEG (SNAP only; slices above 4096 samples, whose snapshot pass runs chunk after chunk): the launch codes samples [seg_first,
// seg_first + 4096) of every slice and parks the lane's coder -- low, range, the staged bytes, the count of flushed ones -- in a
// 64-byte record per slice (`seg_state`) for the launch that codes the next segment, so that the coding of chunk c runs while the
// pass prepares chunk c + 1 on another stream (codec.hip).  The last segment of a slice finishes its stream as ever.
// (the 1-row-slice kernels are held to the registers of eight wavefronts per SIMD: they are bound by instruction issue and live on
// the other wavefronts' instructions while one waits)
// SMALL (ROWS with SYM = uint8_t only, where the kernel forms the contexts itself): LargeModel = false.
template <int NCH, bool ROWS, typename SYM, bool LDSTAB = false, bool SNAP = false, bool SEG = false, bool SMALL = false>
__global__ __launch_bounds__(64, ROWS ? 8 : 1) void k_encode_slices(const Geometry g, const uint32_t lpw,
                                                      const SYM* __restrict__ sym, uint64_t* __restrict__ states,
                                                      uint8_t* __restrict__ scratch, uint32_t* __restrict__ slice_len,
                                                      uint64_t* __restrict__ group_sum, uint32_t* status, const uint64_t gpat,
                                                      unsigned long long* __restrict__ counters, const uint32_t seg_first = 0,
                                                      uint32_t* __restrict__ seg_state = nullptr) {
    static_assert(!(SNAP && (ROWS || LDSTAB)) && (SNAP || !SEG), "one kernel family at a time");
    static_assert(!SMALL || (ROWS && sizeof(SYM) == 1), "the model is a template flag only where the kernel forms the contexts");
    constexpr bool ASM = (ROWS || SNAP) && LLMI_ASM_ENC != 0;
    entry_t* tab;
    uint8_t* stage;
    uint32_t* rowbank;
    if constexpr (ASM) {
        static_assert(kStagePad == 16 && kStageBytes == 32, "kRowsEncBankOff");
#ifdef LLMI_TEST_LDS_OFFSET  // guard build only (make guards): static LDS in front of the dynamic block -- the check below must fire
        __shared__ uint32_t s_displace[4];
        if (threadIdx.x < 4) reinterpret_cast<volatile uint32_t*>(s_displace)[threadIdx.x] = gpat != 0;
#endif
        tab = reinterpret_cast<entry_t*>(dyn_lds + kRowsEncTabOff);
        stage = dyn_lds + kRowsEncStageOff;
        rowbank = reinterpret_cast<uint32_t*>(dyn_lds + kRowsEncBankOff);
        if (uint32_t(uintptr_t((lds_u8_ptr)dyn_lds)) != 0) {  // (folds away: the address is a link-time constant)
            if (threadIdx.x == 0) atomicOr(status, kStInternal);
            return;
        }
    } else {
        __shared__ entry_t s_tab[128];
        __shared__ __attribute__((aligned(32))) uint8_t s_stage[kStagePad + kStageBytes * 64];
        __shared__ uint32_t s_rowbank[ROWS ? kRowBankWords : 1];  // (SNAP without the hand-written block keeps its bank in registers)
        tab = s_tab;
        stage = s_stage;
        rowbank = s_rowbank;
    }
    clear_lds_states<LDSTAB>();
    load_table(tab);
    const uint32_t id = blockIdx.x * lpw + threadIdx.x;
    if (threadIdx.x >= lpw || id >= g.n_slices) return;
    const SliceRect r = slice_rect(g, id);
    RangeEnc e;
    e.low = 0; e.range = 0xFF00;  // llcomp.hpp:35 (held byte: see RangeEnc)
    e.flushed = 0;
    e.area = stage + kStagePad + threadIdx.x * kStageBytes;
    e.base = uint32_t(uintptr_t((lds_u8_ptr)stage)) + kStagePad + threadIdx.x * kStageBytes;
    e.wp = e.base - 1;  // position -1: the dummy byte of the first renormalisation (see the staging area)
    e.out = scratch + ((((size_t(id >> g.lane_shift) * (g.slice_cap >> 4)) << g.lane_shift) + (id & ((1u << g.lane_shift) - 1))) << 4);
    e.gout = scratch + (((size_t(__builtin_amdgcn_readfirstlane(id >> g.lane_shift)) * (g.slice_cap >> 4)) << g.lane_shift) << 4);
    e.oofs = (id & ((1u << g.lane_shift) - 1)) << 4;
    e.ostep = 16u << g.lane_shift;
    asm volatile("" : "+v"(e.ostep));
    e.cap = int32_t(g.slice_cap);
    e.shift = g.lane_shift;
    e.carries = 0;
    const uint32_t n_row = r.sw * (NCH ? uint32_t(NCH) : g.nch);  // samples per slice row (NCH == 0: any channel count)
    // symbols in lane order: sample k of this slice is p0[k * GW]; the lanes of a group read one contiguous piece
    const SYM* p0 = sym + lane_order_index(g, id, 0);
    const size_t GW = size_t(1) << g.lane_shift;  // distance between consecutive samples of this slice
    const uint32_t total = n_row * r.sh;
    bool hot = false;  // wave-uniform: most lanes had a non-zero residual last time
    LLMI_PROBE_START();

    if constexpr (SNAP) {
        // One bank and one residual per sample, front to back.  The sample index is wave-uniform (lock-step), so the piece
        // address is a scalar base plus the lane's fixed offset.
        const uint32_t cap = snapshot_cap(g);
        const uint32_t grp = __builtin_amdgcn_readfirstlane(id >> g.lane_shift);
        const char* const gres = reinterpret_cast<const char*>(sym) + ((size_t(grp) * cap * 2) << g.lane_shift);
        const char* const gbank = reinterpret_cast<const char*>(states) + ((size_t(grp) * cap * 8) << g.lane_shift);
        const uint32_t row = 32u << g.lane_shift;
        uint32_t lofs = (id & ((1u << g.lane_shift) - 1)) * 32u;
        asm volatile("" : "+v"(lofs));
        auto load_res = [&](uint32_t i) -> int {
            i = min(i, cap - 1);
            return *reinterpret_cast<const int16_t*>(gres + size_t(i >> 4) * row + ((i & 15u) << 1) + lofs);
        };
        auto load_bank = [&](uint32_t i) -> uint2 {
            i = min(i, cap - 1);
            return *reinterpret_cast<const uint2*>(gbank + size_t(i >> 3) * (2 * row) + ((i & 7u) << 3) + 2 * lofs);  // 64-byte pieces
        };
        uint32_t i = 0, end = total;
        [[maybe_unused]] uint32_t* const rec = SEG ? seg_state + size_t(id) * 16 : nullptr;  // this slice's parked coder (64 bytes)
        if constexpr (SEG) {
            if (seg_first >= total) return;  // this slice ended in an earlier segment (its length is written)
            i = seg_first;
            end = min(total, seg_first + kSnapMaxSamples);
            if (seg_first) {  // take the coder up where the previous segment's launch left it
                const uint4 a = *reinterpret_cast<const uint4*>(rec), b = *reinterpret_cast<const uint4*>(rec + 4);
                const uint4 s0 = *reinterpret_cast<const uint4*>(rec + 8), s1 = *reinterpret_cast<const uint4*>(rec + 12);
                e.low = a.x; e.range = a.y; e.wp = e.base + a.z; e.flushed = int32_t(a.w);
                e.carries = b.x; hot = b.y != 0;
                e.oofs += (uint32_t(e.flushed) >> 4) * e.ostep;
                uint32_t* const st = reinterpret_cast<uint32_t*>(e.area);
                st[0] = s0.x; st[1] = s0.y; st[2] = s0.z; st[3] = s0.w; st[4] = s1.x; st[5] = s1.y; st[6] = s1.z; st[7] = s1.w;
            }
        }
#if LLMI_ASM_ENC
        // the hand-written sample in its snapshot form (enc_sample_asm.inc, LL_SNAP): the bank arrives in two registers and no
        // state is written back anywhere
        EncRowsExtra xs{0u, 0u, 0u};
        unsigned long long low_range = e.low | ((unsigned long long)e.range << 32);
#endif
        auto code = [&](int res, uint2 bk) {
#if LLMI_ASM_ENC
            enc_snap_sample_asm(low_range, e.wp, xs, bk.x, bk.y, res, e.base);
            if (__builtin_expect(xs.any_pend != 0, 0)) {
                xs.any_pend = 0;
                if (xs.pend) enc_carry_back_flushed(e, e.out);
                xs.pend = 0;
            }
#else
            Bank bank{{bk.x, bk.y}, nullptr};
            if (hot) enc_residual<true, false>(e, bank, tab, res); else enc_residual<false, false>(e, bank, tab, res);
            hot = __builtin_amdgcn_readfirstlane(2 * __popcll(__ballot(res != 0)) >= __popcll(__ballot(true)));
#endif
        };
        // A wavefront that runs alone on its SIMD (a few thousand slices of 4096 samples do not fill the GPU) codes a sample
        // in well under a microsecond, an HBM round trip under load takes two: bank and residual are requested FOUR samples
        // ahead, through four register slots that the 4x unrolled bulk loop rotates statically.  The bulk runs under a scalar
        // counter when all slices of the wavefront are equally long; what is left takes the loop with the per-lane test.
        const uint32_t todo = end - i, todo0 = __builtin_amdgcn_readfirstlane(todo);
        const bool same = __builtin_amdgcn_ballot_w64(todo != todo0) == 0;
        const uint32_t n_bulk = i + (same ? todo0 & ~3u : 0);  // (i is wave-uniform: 0, or the segment's first sample)
        int r0 = load_res(i), r1 = load_res(i + 1), r2 = load_res(i + 2), r3 = load_res(i + 3);
        uint2 b0 = load_bank(i), b1 = load_bank(i + 1), b2 = load_bank(i + 2), b3 = load_bank(i + 3);
#define LLMI_SNAP_SAMPLE(R, B, AHEAD)                          \
        {                                                          \
            const int rc = int(consume_here(uint32_t(R)));        \
            uint2 bc = B;                                          \
            bc.x = consume_here(bc.x);                             \
            R = load_res(i + AHEAD);                               \
            B = load_bank(i + AHEAD);                              \
            if (e.wp >= e.base + 16) enc_flush16(e);               \
            code(rc, bc);                                          \
        }
        for (; i < n_bulk; i += 4) {
            LLMI_SNAP_SAMPLE(r0, b0, 4)
            LLMI_SNAP_SAMPLE(r1, b1, 5)
            LLMI_SNAP_SAMPLE(r2, b2, 6)
            LLMI_SNAP_SAMPLE(r3, b3, 7)
        }
        for (; i < end; ++i) {  // (slot 0 always holds sample i here: the slots move down by one)
            LLMI_SNAP_SAMPLE(r0, b0, 4)
            {
                const int tr = r0;
                const uint2 tb = b0;
                r0 = r1; r1 = r2; r2 = r3; r3 = tr;
                b0 = b1; b1 = b2; b2 = b3; b3 = tb;
            }
        }
#undef LLMI_SNAP_SAMPLE
#if LLMI_ASM_ENC
        e.low = uint32_t(low_range);
        e.range = uint32_t(low_range >> 32);
#endif
        if constexpr (SEG) {
            if (end < total) {  // the slice goes on: park the coder for the next segment's launch
                const uint32_t* const st = reinterpret_cast<const uint32_t*>(e.area);
                *reinterpret_cast<uint4*>(rec) = make_uint4(e.low, e.range, e.wp - e.base, uint32_t(e.flushed));
                *reinterpret_cast<uint4*>(rec + 4) = make_uint4(e.carries, hot ? 1u : 0u, 0u, 0u);
                *reinterpret_cast<uint4*>(rec + 8) = make_uint4(st[0], st[1], st[2], st[3]);
                *reinterpret_cast<uint4*>(rec + 12) = make_uint4(st[4], st[5], st[6], st[7]);
                return;
            }
        }
    } else if constexpr (ROWS) {
        // contexts 0 / 605 / 1210 only: their state bytes sit in LDS, [context][lane] (a read + a write per sample
        // instead of selecting among / writing back to three register pairs: twelve v_cndmask)
        for (uint32_t k = 0; k < 6; ++k) rowbank[k * 64 + threadIdx.x] = 0;
        // PX (SYM = uint8_t, planar 1-row slices: rows_encoder_reads_pixels): `sym` is the caller's pixel batch and the lane runs stage A
        // itself -- it reads its own pixels (tile base + k*C), keeps its plane's l and L in registers and forms the context's byte offset
        // and the folded residual exactly as k_model_rows_fwd + the 16-bit symbol below do.  Otherwise symbols in lane order.
        // Either way the input comes through a wave-uniform base and a running 32-bit byte offset per lane: one global_load with a
        // scalar base and one 2-cycle add per sample, no 64-bit address arithmetic.
        constexpr bool PX = sizeof(SYM) == 1;
        const char* gsym;
        uint32_t sofs, sstep;
        [[maybe_unused]] uint32_t n_dword = total;  // PX: samples 0 .. n_dword-1 are read as dwords, the rest byte by byte (rows_px_dwords)
        [[maybe_unused]] uint32_t xm = 0, coef = 0, my = 0;
        [[maybe_unused]] int pl = 128, pL = 128;  // PX: l and L of the lane's plane (llcomp.hpp:417-419: 128 at the slice start; see xm)
        if constexpr (PX) {
            // tile_h == 1: the tiles of a batch lie back to back in raster order, so lane 0's tile starts lowest and the wavefront's
            // tiles span (64 / C + 2) tiles at most (< 2^31 bytes: rows_encoder_reads_pixels)
            const uint32_t C = g.c;
            const unsigned long long tbase = ((unsigned long long)(r.frame) * g.h + r.y0) * g.w * C + (unsigned long long)(r.x0) * C;
            // (readfirstlane returns an int: both halves through uint32_t, or a low word at or past 2^31 would sign-extend)
            const unsigned long long wbase = (unsigned long long)uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(tbase))) |
                                             ((unsigned long long)uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(tbase >> 32))) << 32);
            gsym = reinterpret_cast<const char*>(sym) + wbase;
            sofs = uint32_t(tbase - wbase);
            sstep = C;
            const unsigned long long total_bytes = (unsigned long long)(g.frames) * g.h * g.w * C;
            n_dword = rows_px_dwords(tbase, total, C, total_bytes);
            // the plane from the pixel's dword d (llcomp.hpp:396-414), without a branch and without extracting a byte: two byte dot
            // products (v_dot4_u32_u8).  With G' = 255 - G in byte 1 of d ^ 0xFF00 every term is non-negative:
            //   plane 0: R - G + 255 = (1,1,0,0) . (d ^ 0xFF00)      plane 2: B - G + 255 = (0,1,1,0) . (d ^ 0xFF00)
            //   plane 1: G + (t & my), t = (R + B - 2G) / 4 truncated, R + B - 2G = (1,2,1,0) . (d ^ 0xFF00) - 510
            //   plane 3 and C < 3: the own byte.
            // t & my goes in as the second product's accumulator.  Planes 0 and 2 are carried 255 too high, l and L with them from
            // their start value on: the coder only ever sees v - l and L - l.
            const bool diff = C >= 3 && (r.ch == 0 || r.ch == 2);
            xm = diff ? 0xFF00u : 0u;
            coef = diff ? (r.ch == 0 ? 0x0101u : 0x010100u) : 1u << (8 * r.ch);
            my = C >= 3 && r.ch == 1 ? ~0u : 0u;
            pl = pL = 128 + int(xm >> 8);
            asm volatile("" : "+v"(xm), "+v"(coef), "+v"(my));
        } else {
            const uint32_t grp = __builtin_amdgcn_readfirstlane(id >> g.lane_shift);
            gsym = reinterpret_cast<const char*>(sym + ((size_t(grp) * g.slice_samples) << g.lane_shift));
            sofs = (id & ((1u << g.lane_shift) - 1)) * uint32_t(sizeof(SYM));
            sstep = uint32_t(sizeof(SYM)) << g.lane_shift;
        }
        asm volatile("" : "+v"(sstep));  // (a vector value: a VALU add with a scalar operand costs twice as much)
        auto load_sym = [&](uint32_t ofs) -> uint32_t {
            if constexpr (PX) {
                uint32_t w;
                __builtin_memcpy(&w, gsym + ofs, 4);  // (pixels start at any byte offset: an unaligned dword load)
                return w;
            } else {
                return *reinterpret_cast<const SYM*>(gsym + ofs);
            }
        };
        // sample k with a per-lane test (the prologue and the loop with the tests): PX, the samples whose dword would leave the caller's
        // buffer -- at most three pixels at the very end of the batch, geometry.hpp -- read their C bytes alone
        auto load_at = [&](uint32_t ofs, uint32_t k) -> uint32_t {
            if constexpr (PX) {
                if (k >= n_dword) {
                    const uint8_t* p = reinterpret_cast<const uint8_t*>(gsym + ofs);
                    uint32_t w = p[0];
                    if (g.c > 1) w |= uint32_t(p[1]) << 8;
                    if (g.c > 2) w |= uint32_t(p[2]) << 16;
                    if (g.c > 3) w |= uint32_t(p[3]) << 24;
                    return w;
                }
            }
            return load_sym(ofs);
        };
        uint32_t s0 = load_at(sofs, 0);
        sofs += sstep;
        uint32_t s1 = total > 1 ? load_at(sofs, 1) : 0;
        sofs += sstep;
        uint32_t bank_base = uint32_t(uintptr_t((lds_u8_ptr) reinterpret_cast<uint8_t*>(rowbank))) + threadIdx.x * 4;
        asm volatile("" : "+v"(bank_base));
#if LLMI_ASM_ENC
        EncRowsExtra xs{0u, 0u, 0u};
        unsigned long long low_range = e.low | ((unsigned long long)e.range << 32);  // (one register pair: enc_rows_asm.hpp)
#endif
        // What the coding needs of a loaded symbol, formed BEFORE the load of the sample two ahead is issued (the asm pins the order):
        // the symbol's register is free by then and the load can take it.  PX: the value of the lane's plane (stage A of
        // k_model_rows_fwd for one sample); otherwise the symbol itself.
        auto front = [&](uint32_t sy) -> uint32_t {
            uint32_t t = sy;
            if constexpr (PX) {
                const int sum = int(__builtin_amdgcn_udot4(sy ^ 0xFF00u, 0x010201u, uint32_t(-510), false));
                int neg = sum >> 31;
                asm volatile("" : "+v"(neg));  // (2-cycle forms only: ashr, and, add, ashr -- not a bit-field extract)
                const int q = (sum + (neg & 3)) >> 2;  // truncating division, llcomp.hpp:402
                t = __builtin_amdgcn_udot4(sy ^ xm, coef, uint32_t(q & int(my)), false);
            }
            asm volatile("" : "+v"(t) : : "memory");
            return t;
        };
        // The context of a sample needs no symbol: PX, it hangs on pl and pL alone.  Formed in front of front(), it is the last reader
        // of pL -- the value front() forms can then take pL's register, and pl / pL swap roles from sample to sample.  MODEL (PX only):
        // how L - l is formed -- kModelSmall for the slice's first two samples ("no L at x <= 1", llcomp.hpp:417-419) and under
        // LargeModel = false.
        struct Ctx {
            uint32_t bofs;  // |quant5(L - l)| * 512: byte offset of the context's row bank
            int sg;         // hash = 605*quant5(L - l) < 0: the residual is folded (llcomp.hpp:433-436)
        };
        auto context = [&](auto model) -> Ctx {
            constexpr int MODEL = decltype(model)::value;
            Ctx c{0u, 0};
            if constexpr (PX && MODEL != kModelSmall) {
                const int dq = pL - pl;
                c.sg = dq >> 31;
                asm volatile("" : "+v"(c.sg));  // (or hipcc forms |d| with v_sub + v_max_i32, a 4-cycle form)
                const uint32_t aq = uint32_t((dq ^ c.sg) - c.sg);
                // |quant5| * 512 = 512 * ([aq >= 1] + [aq >= 4]); planes lie in [-255, 255], so aq <= 510 and bit 9 of aq + 511
                // (aq + 508) says aq >= 1 (aq >= 4)
                c.bofs = ((aq + 511u) & 0x200u) + ((aq + 508u) & 0x200u);
                asm volatile("" : "+v"(c.bofs));
            }
            return c;
        };
        // one sample: context -> row bank, residual -> bins
        auto code = [&](uint32_t sy, Ctx c, auto model) {
            constexpr int MODEL = decltype(model)::value;
            uint32_t bofs = c.bofs;
            int res;
            if constexpr (PX) {
                const int v = int(sy);
                res = MODEL == kModelSmall ? v - pl : ((v - pl) ^ c.sg) - c.sg;
                pL = pl;
                pl = v;
            } else if constexpr (sizeof(SYM) == 2) {  // fused stage A: |quant5| in bits 12..13, residual in bits 0..11
                bofs = (sy >> 3) & 0x600u;
                res = int(sy << 20) >> 20;
            } else {
                bofs = (((sy & 0xFFFF) * 109u) >> 7) & 0x600u;  // 0 / 605 / 1210 -> 0 / 1 / 2
                res = int(sy) >> 16;
            }
#if LLMI_ASM_ENC
            enc_rows_sample_asm(low_range, e.wp, xs, bank_base + bofs, res, e.base);
            if (__builtin_expect(xs.any_pend != 0, 0)) {
                xs.any_pend = 0;
                // (all lanes of the wavefront belong to one lane group: the lane's first unit from the group's)
                if (xs.pend) enc_carry_back_flushed(e, e.gout + (size_t(id & ((1u << g.lane_shift) - 1)) << 4));
                xs.pend = 0;
            }
#else
            uint32_t* bp = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(rowbank) + threadIdx.x * 4 + bofs);
            Bank bank{{bp[0], bp[64]}, reinterpret_cast<uint8_t*>(bp)};  // new states: byte stores
            if (hot) enc_residual<true, true>(e, bank, tab, res); else enc_residual<false, true>(e, bank, tab, res);
            hot = __builtin_amdgcn_readfirstlane(2 * __popcll(__ballot(res != 0)) >= __popcll(__ballot(true)));
#endif
        };
        // Memory operations of one wave retire in order and s_waitcnt counts loads and stores together, so the order
        // inside a sample is: consume what was requested two samples ago (long back, no stall) -> issue the next prefetch
        // -> issue the stores of the previous sample's output.  Nothing is ever waited for right after it was issued.
        // The slice's first two samples are coded in front of the loops, with their per-lane tests: they have no L, and no loop
        // carries a test for them.  When all slices of the wavefront have the same length (all but those with the ragged last
        // tile column), the bulk then runs under a scalar loop counter with no per-lane tests, two samples per turn: the prefetch
        // distance is two, so the load for sample i + 2 goes into the register sample i has just left and pl / pL swap roles --
        // nothing is copied at the back edge.  An odd sample, the last two samples (PX: rows_px_tail(C) -- the bulk loads no sample
        // that may need byte reads: 5 for C = 1, 3 for C = 2 and 3, 2 for C = 4), and ragged wavefronts, take the loop with the tests.
        const uint32_t total0 = __builtin_amdgcn_readfirstlane(total);
        const bool same = __builtin_amdgcn_ballot_w64(total != total0) == 0;
        const uint32_t tail = PX ? rows_px_tail(g.c) : 2u;
        const uint32_t n_bulk = same && total0 > tail ? total0 - tail : 0;
        auto sample_tested = [&](uint32_t i, auto model) {
            s0 = consume_here(s0);
            const Ctx c0 = context(model);
            const uint32_t t0 = front(s0);
            const uint32_t s2 = i + 2 < total ? load_at(sofs, i + 2) : 0;
            sofs += sstep;
            enc_flush_batched(e);  // (LDS addresses: no wrap-around, wp >= base - 1)
            code(t0, c0, model);
            s0 = s1;
            s1 = s2;
        };
        auto bulk = [&](uint32_t& i, auto model) {
            for (; i + 1 < n_bulk; i += 2) {
                s0 = consume_here(s0);  // loaded two samples ago
                const Ctx c0 = context(model);
                const uint32_t t0 = front(s0);
                s0 = load_sym(sofs);
                sofs += sstep;
                enc_flush_batched(e);
                code(t0, c0, model);
                s1 = consume_here(s1);
                const Ctx c1 = context(model);
                const uint32_t t1 = front(s1);
                s1 = load_sym(sofs);
                sofs += sstep;
                enc_flush_batched(e);
                code(t1, c1, model);
            }
            for (; i < total; ++i) sample_tested(i, model);
        };
        sample_tested(0, no_model);  // (a slice has at least one sample)
        if (total > 1) sample_tested(1, no_model);
#if LLMI_ASM_ENC
        // (behind a per-lane test hipcc holds the block's wave-uniform flags in vector registers: back to scalars)
        xs.hot = __builtin_amdgcn_readfirstlane(xs.hot);
        xs.any_pend = 0;
#endif
        uint32_t i = 2;
        bulk(i, std::integral_constant<int, SMALL ? kModelSmall : kModelLarge>{});
#if LLMI_ASM_ENC
        e.low = uint32_t(low_range);
        e.range = uint32_t(low_range >> 32);
#endif
    } else {
        // Everything the coder needs is known up front: the symbol two samples ahead and the state bank one sample
        // ahead are in flight while a sample is coded (forwarded when consecutive samples share a context).
        // state tables of a lane group in HBM: [context][lane], so that lanes which are in the same context at the same
        // time (smooth content: most of them) share cache lines; LDSTAB: this slice's own table in LDS
        uint64_t* banks;
        uint32_t bsh;  // log2 of the distance between consecutive contexts, in entries
        if constexpr (LDSTAB) {
            banks = reinterpret_cast<uint64_t*>(dyn_lds);
            bsh = 0;
        } else {
            banks = states + ((size_t(id >> g.lane_shift) * kContexts) << g.lane_shift) + (id & ((1u << g.lane_shift) - 1));
            bsh = g.lane_shift;
        }
        uint32_t fk = 0;
        auto fetch = [&]() -> uint32_t { return p0[size_t(fk++) * GW]; };
        uint32_t s0 = fetch();
        uint32_t s1 = total > 1 ? fetch() : 0;
        // (LDSTAB: the table was cleared in LDS by this kernel, gpat == 0 and every tag is 0: both helpers are identities)
        uint64_t b0 = bank_fresh<LDSTAB>(banks[size_t(s0 & 0xFFFF) << bsh], gpat);
        for (uint32_t i = 0; i < total; ++i) {
            const uint32_t s2 = i + 2 < total ? fetch() : 0;
            const uint32_t ctx0 = s0 & 0xFFFF, ctx1 = s1 & 0xFFFF;
            const int res = int(s0) >> 16;
            // The next sample's bank is REQUESTED here and looked at only behind this sample's coding (its tag test right here
            // put a wait for the load -- and for everything sent before it -- in front of the coding: one memory round trip per
            // sample in the serial chain, as in the decoder before round 5).
            uint64_t raw1 = (i + 1 < total) ? banks[size_t(ctx1) << bsh] : 0;
            Bank bank{{uint32_t(b0), uint32_t(b0 >> 32)}, nullptr};
            if (hot) enc_residual<true, false>(e, bank, tab, res); else enc_residual<false, false>(e, bank, tab, res);
            hot = __builtin_amdgcn_readfirstlane(2 * __popcll(__ballot(res != 0)) >= __popcll(__ballot(true)));
            b0 = uint64_t(bank.w[0]) | (uint64_t(bank.w[1]) << 32);
            // one drain per sample, in front of this sample's stores: what it waits for was sent a whole sample ago
            if constexpr (!LDSTAB) drain_vector_memory();
            uint64_t b1 = bank_fresh<LDSTAB>(raw1, gpat);
            banks[size_t(ctx0) << bsh] = bank_tagged<LDSTAB>(b0, gpat);
            if (ctx1 == ctx0) b1 = b0;  // the prefetched copy is stale: forward
            b0 = b1;
            if (e.wp >= e.base + 16) enc_flush16(e);
            s0 = s1;
            s1 = s2;
        }
    }
    int32_t n_bytes = enc_pos(e);  // (before the tail flush moves wp)
    enc_finish_and_count<ROWS>(e, n_bytes);
    LLMI_PROBE_STOP(0);
    if (n_bytes > e.cap) {
        atomicOr(status, kStOverflow);
        n_bytes = e.cap;
    }
    slice_len[id] = uint32_t(n_bytes);
    publish_count(counters, kCtrEncCarryBacks, e.carries);
    // When a wavefront holds exactly one lane group (the normal case) it leaves the group's byte count behind: the
    // global scan then runs over one value per group instead of one per slice.  The sum is formed with v_readlane over
    // the lanes that are active HERE (a convergent operation with a defined result per lane: no shared-memory hand-off
    // between lanes whose order would rest on how the compiler lays out the reconverged paths above).
    if (group_sum) {
        unsigned long long live = __ballot(1), sum = 0;
        while (live) {
            const int lane = __builtin_ctzll(live);
            sum += uint32_t(__builtin_amdgcn_readlane(n_bytes, lane));
            live &= live - 1;
        }
        if (threadIdx.x == 0) group_sum[blockIdx.x] = sum;
    }
}

// ================================================ DECODER ========================================================
// new state of a slot from the half-entry that belongs to the decoded bit (byte 0 = state, upper half = table offset)
template <int SLOT, bool INLDS>
__device__ __forceinline__ void dec_put_state(Bank& b, uint32_t half) {
    if constexpr (INLDS) *reinterpret_cast<uint16_t*>(b.lds + widebank_byte(SLOT)) = uint16_t(half >> 16);
    else set_slot_state<SLOT>(b.w, half & 0xFF);
}
template <int SLOT, bool INLDS>
__device__ __forceinline__ entry_t dec_entry(const Bank& b, const entry_t* tab) {
    if constexpr (INLDS) return lds_entry(wide_offset<SLOT>(b.w));
    else return tab[slot_state<SLOT>(b.w)];
}
template <bool INLDS>
__device__ __forceinline__ void dec_fetch_slot0(Entries& E, const Bank& b, const entry_t* tab) { E.e0 = dec_entry<0, INLDS>(b, tab); }
template <bool INLDS>
__device__ __forceinline__ void dec_fetch_rest(Entries& E, const Bank& b, const entry_t* tab) {
    E.e1 = dec_entry<1, INLDS>(b, tab);
    E.e2 = dec_entry<2, INLDS>(b, tab);
    E.e3 = dec_entry<3, INLDS>(b, tab);
    E.e4 = dec_entry<4, INLDS>(b, tab);
    E.e5 = dec_entry<5, INLDS>(b, tab);
    E.e6 = dec_entry<6, INLDS>(b, tab);
    E.e7 = dec_entry<7, INLDS>(b, tab);
}
// Range decoder of one lane (llcomp.hpp:91-127).  The stream is consumed through a 64-bit register window (next byte
// = window & 0xFF) that is topped up with aligned dword loads, one dword prefetched ahead; bytes past the end of the
// slice read as 0 (llcomp.hpp:475-479).  The fill level is not counted: a SENTINEL 1 bit sits right above the valid
// bytes (bit 8 * valid), so consuming a byte is just the shift, "at most 3 bytes left" is `high dword == 0`, and
// "consumed more than there was" is `window == 0` (the sentinel itself was shifted out).
struct RangeDec {
    uint32_t low, range;
    unsigned long long win; // window, LSB first (next byte = win & 0xFF), sentinel bit above the valid bytes
    uint32_t nxt;           // prefetched dword that follows the window
    // The staged streams are in DWORD lane order, [group][dword k][lane]: dword k of this lane sits `k * step` bytes
    // behind its first one, so the prefetch walks a running byte offset -- one 2-cycle add and one clamp per dword
    // (16-byte units as on the encoder's side cost five 4-cycle operations of address arithmetic per top-up).
    const char* gbase;      // WAVE-UNIFORM: first dword of this lane group in the staged array
    uint32_t ofs;           // byte offset from there of the next dword to prefetch (lane * 4 + k * step)
    uint32_t step;          // 4 << lane_shift (a vector value: an add with a scalar operand costs twice as much)
    uint32_t ofs_end;       // offset of the first dword AFTER the stream; the stager guarantees it (and every byte past the
                            // end of the stream inside the last dword) reads zero, as llcomp.hpp:475-479 wants
    uint32_t replays;       // event counter: samples that went through rollback + checked replay (kCtrDecReplays)
};
__device__ __forceinline__ bool window_low(const RangeDec& d) { return uint32_t(d.win >> 32) == 0; }  // <= 3 bytes
// issues the load of dword k.  UNCONDITIONAL (index clamped to the zero dword behind the stream) so that its result
// lands directly in the loop-carried register -- a conditional load ends in a register copy and hipcc waits vmcnt(0)
// for that copy right after the issue; 32-bit offset from a wave-uniform base = one global_load with an SGPR base.
__device__ __forceinline__ void dec_prefetch(RangeDec& d) {
    d.nxt = *reinterpret_cast<const uint32_t*>(d.gbase + min(d.ofs, d.ofs_end));
    d.ofs += d.step;
}
// Pins the point where a value that was loaded earlier is consumed: the compiler's s_waitcnt for it lands HERE (the
// load was issued a whole sample ago, so it has long returned) and no later load may be hoisted above it -- otherwise
// hipcc issues the next prefetch first and then waits vmcnt(0) for both.
__device__ __forceinline__ uint32_t consume_here(uint32_t v) {
    asm volatile("" : "+v"(v) : : "memory");
    return v;
}
__device__ __forceinline__ void dec_append(RangeDec& d) {  // requires window_low(d) and win != 0
    const uint32_t ready = consume_here(d.nxt);
    // the sentinel (bit sh = 0, 8, 16 or 24 of the low dword) is replaced by the new dword with a sentinel above it
    const uint32_t sh = 31u - uint32_t(__builtin_clz(uint32_t(d.win)));
    const uint32_t rest = uint32_t(d.win) ^ (1u << sh);  // (the high dword is zero here)
    d.win = ((0x100000000ull | ready) << sh) | rest;
    dec_prefetch(d);
}
// The checked replay's top-up (rare): the dword it requests is waited for at once, so that no request of the replay is still
// in flight when the sample is done -- the sample loops can then rely on "nothing pending behind the last drain" (2-D decoder).
__device__ __forceinline__ void dec_append_drained(RangeDec& d) {
    dec_append(d);
    drain_vector_memory();
}
__device__ __forceinline__ void dec_open(RangeDec& d, const uint32_t* group, uint32_t lane, uint32_t shift, uint32_t len) {
    d.gbase = reinterpret_cast<const char*>(group);
    d.ofs = lane * 4;
    d.step = 4u << shift;
    asm volatile("" : "+v"(d.step));
    d.ofs_end = lane * 4 + ((len + 3) >> 2) * d.step;
    dec_prefetch(d);
    const uint32_t first = d.nxt;
    dec_prefetch(d);
    const unsigned long long both = first | ((unsigned long long)d.nxt << 32);
    dec_prefetch(d);
    d.range = 0xFF00;  // llcomp.hpp:93-96: low = first two bytes
    d.low = ((first & 0xFF) << 8) | ((first >> 8) & 0xFF);
    d.win = (both >> 16) | (1ull << 48);  // six bytes left
    d.replays = 0;
}
// CHECKED == false is the fast path: it never looks at the fill level of the window.  The kernel tops the window up to
// >= 4 bytes before every sample and afterwards looks at it once: an empty window (the sentinel is gone) means the
// sample consumed more bytes than the window held (possible, a sample can take up to 13 bytes, but rare); the coder
// state is then rolled back and the sample is decoded again with CHECKED == true, which refills inside the step.
// window >>= 8 as ONE 64-bit shift (hipcc splits it into v_perm + v_lshr)
__device__ __forceinline__ unsigned long long window_next(unsigned long long w) {
    unsigned long long r;
    asm("v_lshrrev_b64 %0, 8, %1" : "=v"(r) : "v"(w));
    return r;
}
// Refill inside ONE exec-masked region with constant shift amounts (llcomp.hpp:115-120).
__device__ __forceinline__ void dec_refill(RangeDec& d) {
    if (d.range < 0x100) {
        d.range <<= 8;
        d.low = (d.low << 8) | (uint32_t(d.win) & 0xFF);  // low < range < 0x100 here
        d.win = window_next(d.win);
    }
}
template <bool CHECKED>
__device__ __forceinline__ bool dec_core(RangeDec& d, uint32_t P) {  // llcomp.hpp:98-121, branch-free refill
    if (CHECKED && d.win <= 1) dec_append_drained(d);  // no byte left
    const uint32_t r1 = __umul24(d.range, P) >> 8;
    const uint32_t r0 = d.range - r1;
    uint32_t diff;
    const bool under = __builtin_usub_overflow(d.low, r0, &diff);  // one v_sub_co: difference and the decision
    const bool bit = !under;
    d.low = under ? d.low : diff;
    d.range = under ? r0 : r1;
    // Refill inside ONE exec-masked region with constant shift amounts.  (Measured on gfx950, tools/ubench: shifts by a
    // register, v_cndmask with an SGPR mask, v_perm, v_alignbit, v_cmp all take 4 cycles per wavefront, plain
    // add/sub/and/or/mov and shifts by a constant take 2; the branch-free form of this block cost eight 4-cycle ops.)
    dec_refill(d);
    return bit;
}
// dec_core for a run of bins on one slot whose bits are gathered in `w` (inverted: see dec_residual): the borrow of the
// subtraction stays in VCC for all three selects (2-cycle v_cndmask_e32) and is shifted into `w` by an add-with-carry.
// Returns the half of entry `cur` that belongs to the decoded bit.
template <bool CHECKED>
__device__ __forceinline__ uint32_t dec_step_acc(RangeDec& d, uint32_t P, entry_t cur, uint32_t& w) {
    if (CHECKED && d.win <= 1) dec_append_drained(d);  // no byte left
    const uint32_t r1 = __umul24(d.range, P) >> 8;
    const uint32_t r0 = d.range - r1;
    uint32_t diff, nx;
    asm("v_sub_co_u32_e32 %[diff], vcc, %[low], %[r0]\n\t"
        "s_nop 1\n\t"
        "v_cndmask_b32_e32 %[range], %[r1], %[r0], vcc\n\t"   // borrow: bit 0, range = r0, low stays
        "v_cndmask_b32_e32 %[low], %[diff], %[low], vcc\n\t"
        "v_cndmask_b32_e32 %[nx], %[hi], %[lo], vcc\n\t"
        "v_addc_co_u32_e32 %[w], vcc, %[w], %[w], vcc"
        : [diff] "=&v"(diff), [range] "=&v"(d.range), [low] "+v"(d.low), [nx] "=&v"(nx), [w] "+v"(w)
        : [r0] "v"(r0), [r1] "v"(r1), [lo] "v"(uint32_t(cur)), [hi] "v"(uint32_t(cur >> 32))
        : "vcc");
    if (d.range < 0x100) {  // refill: see dec_core
        d.range <<= 8;
        d.low = (d.low << 8) | (uint32_t(d.win) & 0xFF);
        d.win = window_next(d.win);
    }
    return nx;
}
// A slot that is decoded at most once per sample: selects on the borrow in VCC.  (Round 2 let every lane take the bit-0
// outcome and the lanes with a 1 patch up inside an exec-masked region -- two vector instructions fewer, but three scalar
// ones and an LDS store more, and scalar work is not free: 1 % slower, DESIGN.md section 4.  The ENCODER keeps its regions:
// there the select form makes hipcc spill an entry to scratch, +14 %.)
template <int SLOT, bool CHECKED, bool INLDS>
__device__ __forceinline__ bool dec_once(RangeDec& d, Bank& bank, const Entries& E) {
    const entry_t en = E.get<SLOT>();
    const bool bit = dec_core<CHECKED>(d, prob_of(en));
    dec_put_state<SLOT, INLDS>(bank, successor(en, bit));
    return bit;
}
// getSymbol<true,4,6,7> (llcomp.hpp:219-247).  Returns false on "Invalid exponent".  Arithmetic modulo 2^32.
template <bool ALL, bool CHECKED, bool INLDS>
__device__ __forceinline__ bool dec_residual(RangeDec& d, Bank& bank, const entry_t* tab, uint32_t& out) {
    Entries E;
    dec_fetch_slot0<INLDS>(E, bank, tab);
    if (ALL) dec_fetch_rest<INLDS>(E, bank, tab);
    if (dec_once<0, CHECKED, INLDS>(d, bank, E)) {
        out = 0;
        return true;
    }
    if (!ALL) dec_fetch_rest<INLDS>(E, bank, tab);
    int ex = 0;
    bool ok = true;
    if (dec_once<1, CHECKED, INLDS>(d, bank, E)) {
        ex = 1;
        if (dec_once<2, CHECKED, INLDS>(d, bank, E)) {
            ex = 2;
            if (dec_once<3, CHECKED, INLDS>(d, bank, E)) {
                // Unary tail on slot 4.  The lanes that stay in the loop are exactly the lanes that decoded a 1, so the
                // loop's own exec mask does the selecting: every lane takes the bit-0 outcome (range = r0, low stays,
                // successor = low half of the entry), a lane that decodes a 0 leaves, the others patch up (low = diff,
                // range = r1), refill and move on to the high half's successor.  The refill of the closing bin
                // happens once, behind the loop.
                entry_t cur = E.e4;
                int n = 0;  // bins of the unary tail: n - 1 ones and the closing zero
                for (;;) {
                    if (CHECKED && d.win <= 1) dec_append_drained(d);
                    const uint32_t r1 = __umul24(d.range, prob_of(cur)) >> 8;
                    d.range -= r1;
                    ++n;
                    asm volatile("" : "+v"(n));  // (a per-lane counter: hipcc counts in a scalar and copies it out, a 4-cycle v_mov per bin)
                    uint32_t diff;
                    if (__builtin_usub_overflow(d.low, d.range, &diff)) break;
                    d.low = diff;
                    d.range = r1;
                    if (CHECKED && n > 29) break;  // exponent would exceed 31
                    cur = entry_at(tab, uint32_t(cur >> 32));  // requested before the refill, needed by the next bin
                    dec_refill(d);
                }
                dec_refill(d);
                ex = 2 + n;
                // fast path: no per-step limit -- the run ends by itself once the window holds only zeros; a run
                // longer than 31 is "Invalid exponent" (llcomp.hpp:230-235) and is confirmed by the checked replay
                if (ex > 31) ok = false;
                const uint32_t nx = uint32_t(cur);
                dec_put_state<4, INLDS>(bank, nx);
            }
        }
    }
    if (!ok) return false;
    // The mantissa is gathered with INVERTED bits below its leading one (w), because the decision of a bin is the borrow
    // of a subtraction and the decoded bit is its complement: w = 2w + borrow is one add-with-carry (dec_step_acc).
    uint32_t w = 1;
    const uint32_t ones = (1u << ex) - 1;
    if (ex > 0) {
        w += w + uint32_t(!dec_once<5, CHECKED, INLDS>(d, bank, E));
        if (ex > 1) {
            entry_t cur = E.e6;
            uint32_t nx;
            // w has ex + 1 significant bits when the mantissa is complete.  `limit` is hidden from the optimiser, which
            // would otherwise turn `w < limit` into a shift by a register + compare (two 4-cycle ops per step).
            uint32_t limit = ones + 1;
            asm volatile("" : "+v"(limit));
            do {
                nx = dec_step_acc<CHECKED>(d, prob_of(cur), cur, w);
                cur = entry_at(tab, nx);
            } while (w < limit);
            dec_put_state<6, INLDS>(bank, nx);
        }
    }
    uint32_t v = w ^ ones;
    if (dec_once<7, CHECKED, INLDS>(d, bank, E)) v = 0u - v;
    out = v;
    return true;
}

// One sample: fast path first, checked replay when the window ran dry (or the fast path saw nonsense because of it).
// `hot` (wave-uniform, in / out): most lanes had a non-zero residual last time -- the entries of slots 1..7 are requested up front.
// SET (the hand-written block only): which of its two fixed low : copy register pairs the sample leaves its `low` in; consecutive
// samples alternate, so the low a sample reads is never in the pair it writes.
template <bool INLDS, int SET = 0>
__device__ __forceinline__ bool dec_sample(RangeDec& d, Bank& bank, const entry_t* tab, uint32_t& hot, bool replay_always,
                                           uint32_t& v) {
#if LLMI_ASM_DEC
    if constexpr (INLDS) {
        // The fast path of the 1-row-slice kernels is one hand-written block (dec_rows_asm.hpp).  It reads low, range, the window and
        // the bank words and writes none of them: the coder's state behind the sample arrives in registers of its own, so what the
        // block read IS the rollback snapshot -- nothing is copied per sample, and the registers of two consecutive samples simply
        // swap roles (the bulk loops below code two samples per turn for that).  low arrives as the high half of a pair whose low
        // half is what the sample left of its private copy of the window's next three bytes.
        uint32_t range;
        unsigned long long low_left, win;
        dec_rows_sample_asm<SET>(d.low, d.range, d.win, low_left, range, win, bank.w[0], bank.w[1], bank.w[2], bank.w[3], lds_address(bank.lds),
                                 hot, v);
        // left == 0: more than three bytes wanted, or an invalid exponent -- replayed, and the verdict is formed there
        if (__builtin_expect(uint32_t(low_left) == 0 || replay_always, 0)) {
            ++d.replays;
            // the fast path has already stored new states: put the old ones back
            reinterpret_cast<uint32_t*>(bank.lds)[0] = bank.w[0];
            reinterpret_cast<uint32_t*>(bank.lds)[64] = bank.w[1];
            reinterpret_cast<uint32_t*>(bank.lds)[128] = bank.w[2];
            reinterpret_cast<uint32_t*>(bank.lds)[192] = bank.w[3];
            // The replay starts from the untouched inputs, IN the registers of the block's outputs (the copy is written out, or
            // hipcc replays in place and has the fast path of every sample copy its results back instead).
            dec_rows_replay_inputs<SET>(d.low, d.range, d.win, low_left, range, win);
            d.low = uint32_t(low_left >> 32);
            d.range = range;
            d.win = win;
            return dec_residual<false, true, true>(d, bank, tab, v);
        }
        d.low = uint32_t(low_left >> 32);
        d.range = range;
        d.win = win;
        return true;
    } else
#endif
    {
        const uint32_t s_low = d.low, s_range = d.range, s_b0 = bank.w[0], s_b1 = bank.w[1], s_b2 = bank.w[2], s_b3 = bank.w[3];
        const unsigned long long s_win = d.win;
        bool ok = hot ? dec_residual<true, false, INLDS>(d, bank, tab, v) : dec_residual<false, false, INLDS>(d, bank, tab, v);
        hot = 2 * __popcll(__ballot(v != 0)) >= __popcll(__ballot(true));  // (ballots are wave-uniform: scalar arithmetic)
        // (a sample that ran out of window bytes shows by an empty window)
        if (__builtin_expect(!ok || d.win == 0 || replay_always, 0)) {
            ++d.replays;
            d.low = s_low; d.range = s_range; d.win = s_win;
            bank.w[0] = s_b0; bank.w[1] = s_b1;
            if constexpr (INLDS) {  // the fast path has already stored new states: put the old ones back
                bank.w[2] = s_b2; bank.w[3] = s_b3;
                reinterpret_cast<uint32_t*>(bank.lds)[0] = s_b0;
                reinterpret_cast<uint32_t*>(bank.lds)[64] = s_b1;
                reinterpret_cast<uint32_t*>(bank.lds)[128] = s_b2;
                reinterpret_cast<uint32_t*>(bank.lds)[192] = s_b3;
            }
            ok = dec_residual<false, true, INLDS>(d, bank, tab, v);
        }
        return ok;
    }
}

// CACHE (2-D slices with their tables in HBM): log2 of the entries of a per-lane, direct-mapped, write-back cache of state
// banks in the dynamic LDS block -- banks u64 [entry][lane], then tags u8 [entry][lane] (tag = context >> CACHE, 0xFF = empty;
// entry = context & (2^CACHE - 1)).  A hit costs two LDS reads and one LDS write instead of a 64-byte line fill and a 32-byte
// sector write in HBM; a miss fills, and writes the victim back behind the sample.  Nothing is flushed at the end: the table is
// per call (generation tags), whatever stays in LDS is not needed again.  32 entries = 18 KB per wavefront = eight wavefronts per
// CU; 64 entries (four per CU) were measured slower whenever a launch has more than 1024 wavefronts and 1-3 % faster below
// (profiles/r05_bank_cache_ab.txt).  0 = no cache.  The entry count is geometry.hpp's kBankCacheLog2 (one constant for the flag, the
// launcher and the kernel).
constexpr uint32_t bank_cache_lds_bytes(int log2_entries) { return log2_entries ? (64u * 9u) << log2_entries : 0u; }
// SMALL (ROWS only): LargeModel = false; the other families read the model from the geometry.
template <int NCH, bool ROWS, bool LDSTAB = false, int CACHE = 0, bool SMALL = false>
__global__ __launch_bounds__(64, ROWS && NCH == 1 ? 8 : 1) void k_decode_slices(const Geometry g, const uint32_t lpw_and_flags,
                                                      const uint8_t* __restrict__ units,
                                                      const uint32_t* __restrict__ slice_len,
                                                      uint64_t* __restrict__ states, int16_t* __restrict__ rec,
                                                      uint32_t* status, const uint64_t gpat,
                                                      unsigned long long* __restrict__ counters) {
    __shared__ entry_t tab[128];  // (entries carry absolute LDS addresses, load_table: the hand-written loop needs no base)
    __shared__ uint32_t rowbank[ROWS ? kWideBankWords : 1];
    // quant11 / quant5 as byte tables over the clamped difference (llcomp.hpp:297-341 has them as tables too): five look-ups that
    // fly together instead of five compare chains of ~17 dependent instructions each in front of every sample's bank fetch
    __shared__ int8_t quant_lut[ROWS ? 1 : 512];
    if constexpr (!ROWS) {
        for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
            quant_lut[i] = int8_t(quant11(int(i) - 128));
            quant_lut[256 + i] = int8_t(quant5(int(i) - 128));
        }
    }
    static_assert(CACHE == 0 || (!ROWS && !LDSTAB && NCH != 0), "the bank cache belongs to the 2-D kernels with tables in HBM");
    static_assert(!SMALL || ROWS, "the model is a template flag of the 1-row-slice kernels only");
    // tags are bytes holding context >> CACHE, 0xFF = empty: no real tag may reach 0xFF
    static_assert(CACHE == 0 || ((kContexts - 1) >> CACHE) < 0xFF, "bank cache: a context's tag would alias the empty marker");
    // the wavefront's misses / look-ups since the last bypass check (CACHE): lanes add theirs, every lane reads the sums
    __shared__ uint32_t wave_sums[CACHE != 0 ? 2 : 1];
    clear_lds_states<LDSTAB>();
    if constexpr (CACHE != 0) {  // every entry empty
        uint32_t* tg = reinterpret_cast<uint32_t*>(dyn_lds + (512u << CACHE));
        for (uint32_t i = threadIdx.x; i < (16u << CACHE); i += blockDim.x) tg[i] = 0xFFFFFFFFu;
        if (threadIdx.x < 2) wave_sums[threadIdx.x] = 0;
    }
    load_table(tab);
    const uint32_t lpw = lpw_and_flags & 0xFF;
    const bool replay_always = (lpw_and_flags >> 8) & 1;  // test hook: send every sample through the checked replay too
    [[maybe_unused]] const bool small_model = (g.flags & kGeoSmallModel) != 0;
    const uint32_t id = blockIdx.x * lpw + threadIdx.x;
    if (threadIdx.x >= lpw || id >= g.n_slices) return;
    const SliceRect r = slice_rect(g, id);
    RangeDec d;
    // streams come staged in dword lane order (RangeDec); lengths beyond the payload were clipped (and reported) by the stager.
    // All lanes of a wavefront belong to one lane group (lanes_per_wave divides the group width): its base is uniform.
    const uint32_t len = min(slice_len[id], g.slice_cap - 16);
    const uint32_t grp = __builtin_amdgcn_readfirstlane(id >> g.lane_shift);
    const uint32_t lane_in_group = id & ((1u << g.lane_shift) - 1);
    dec_open(d, reinterpret_cast<const uint32_t*>(units) + ((size_t(grp) * (g.slice_cap >> 2)) << g.lane_shift), lane_in_group,
             g.lane_shift, len);

    // reconstructed samples in lane order: sample k of this slice is p0[k * GW]
    int16_t* p0 = rec + lane_order_index(g, id, 0);
    const ptrdiff_t GW = ptrdiff_t(1) << g.lane_shift;  // distance between consecutive samples of this slice
    // the same through a wave-uniform base + 32-bit element offset (one store instruction, no 64-bit address math)
    int16_t* const gbase = rec + ((size_t(grp) * g.slice_samples) << g.lane_shift);
    uint32_t hot = 0;  // wave-uniform: most lanes had a non-zero residual last time (dec_sample)
    LLMI_PROBE_START();

    if constexpr (ROWS) {
        // one-row slice (llcomp.hpp:494-509 with h == 0): l = left (128 at the start), everything above = l, so
        // hash = 605*quant5(L - l), prediction = l.  The three banks sit in LDS ([context][lane], see the encoder); no
        // state memory in HBM.
        for (uint32_t k = 0; k < 12; ++k) rowbank[k * 64 + threadIdx.x] = lds_address(tab) * 0x00010001u;  // state 0 in every slot
        int l[NCH], L[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) l[k] = L[k] = 128;
        // The previous sample is stored only AFTER the window top-up of the next one, so the top-up never waits for a
        // store that was issued a moment ago (see the encoder).  The very first sample has nothing to store.
        // Per-sample bookkeeping in 2-cycle operations only (add / sub / and / xor / right shifts; tools/ubench/valu_rate3:
        // compares, selects on a scalar mask, min / max, LEFT shifts and everything with a scalar operand cost 4):
        //   * the context index |quant5(L - l)| = [|d| >= 1] + [|d| >= 4] goes straight into the byte offset of its row
        //     bank (1024 bytes per context): bit 31 of |d| + (2^31 - t) says |d| >= t, shifted down to bit 10;
        //   * "no L at x <= 1" (llcomp.hpp:496) without a select: L starts equal to l, and behind the slice's first pixel L takes
        //     the decoded value instead of the old l, so L - l is 0 at x = 0 and x = 1 by itself.  The first pixel is coded in
        //     front of the loops (START), so that no loop carries a mask for it;
        //   * the sign fold is (v ^ s) - s with s = (L - l) >> 31.  LargeModel = false (SMALL) has no difference at all: context 0,
        //     no fold;
        //   * the store goes through ONE running 32-bit byte offset from the wave-uniform base: the delayed store of the sample
        //     before uses it, then it moves on.
        int held_val = 0;
        uint32_t store_ofs = lane_in_group * 2, step_ofs = 2u << g.lane_shift;
        asm volatile("" : "+v"(step_ofs));  // (a vector value: an add with a scalar operand costs twice as much)
        uint8_t* const bank0 = reinterpret_cast<uint8_t*>(rowbank) + threadIdx.x * 4;
        // "Invalid exponent" (llcomp.hpp:230-235) does not leave the loop: the lane notes it and decodes on (whatever it
        // reads stays inside its own stream and slice, and the call reports the error) -- so the loop has no per-lane exit,
        // and when all slices of the wavefront are equally wide it runs under a scalar counter with no per-lane tests at all.
        bool bad = false;
        auto pixel = [&](auto model, auto start, auto set) {
            constexpr int MODEL = decltype(model)::value;
            constexpr bool START = decltype(start)::value;
            constexpr int SET = decltype(set)::value;  // the register pair the pixel's first sample leaves `low` in (dec_sample)
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                if (window_low(d)) dec_append(d);
                if (!(START && k == 0)) {
                    asm volatile("global_store_short %0, %1, %2" : : "v"(store_ofs), "v"(held_val), "s"(gbase) : "memory");
                    store_ofs += step_ofs;
                }
                const int lv = l[k];  // x == 0: 128
                uint32_t sg = 0, bofs = 0;
                if constexpr (MODEL != kModelSmall) {
                    const int dq = L[k] - lv;
                    sg = uint32_t(dq >> 31);  // hash = 605*quant5(L-l) < 0: the residual was folded
                    asm volatile("" : "+v"(sg));  // (or hipcc forms |d| with v_max and the offset with v_and_or: 4-cycle operations)
                    const uint32_t aq = (uint32_t(dq) ^ sg) - sg;
                    uint32_t o1 = ((aq + 0x7FFFFFFFu) >> 21) & 0x400u, o2 = ((aq + 0x7FFFFFFCu) >> 21) & 0x400u;
                    asm volatile("" : "+v"(o1), "+v"(o2));
                    bofs = o1 + o2;  // |quant5(L - l)| * 1024
                }
                uint32_t* bp = reinterpret_cast<uint32_t*>(bank0 + bofs);
                Bank bank{{bp[0], bp[64], bp[128], bp[192]}, reinterpret_cast<uint8_t*>(bp)};
                uint32_t v = 0;
                // (k is a constant once the loop is unrolled: the samples of a pixel alternate between the block's two pairs)
                const bool ok = ((SET + k) & 1) ? dec_sample<true, 1>(d, bank, tab, hot, replay_always, v)
                                                : dec_sample<true, 0>(d, bank, tab, hot, replay_always, v);
                if (!ok) bad = true;
                if constexpr (MODEL != kModelSmall) v = (v ^ sg) - sg;
                const int val = int(int16_t(uint32_t(lv) + v));
                held_val = val;
                L[k] = START ? val : lv;
                l[k] = val;
            }
        };
        // Two pixels per turn of the bulk loop: the coder's state, l / L and the bank words of consecutive samples alternate between
        // two sets of registers (a sample reads one and leaves the other), so nothing is copied at the back edge.  An odd pixel is
        // left to the loop with the per-lane tests, as are ragged wavefronts.
        const uint32_t sw0 = __builtin_amdgcn_readfirstlane(r.sw);
        const uint32_t n_bulk = __builtin_amdgcn_ballot_w64(r.sw != sw0) == 0 ? sw0 : 0;
        uint32_t x = 1;
        constexpr std::integral_constant<int, 0> set0{};
        constexpr std::integral_constant<int, 1> set1{};
        pixel(no_model, std::true_type{}, set0);  // (a slice has at least one pixel; L == l here: no difference under either model)
        constexpr std::integral_constant<int, SMALL ? kModelSmall : kModelLarge> model{};
        if constexpr (NCH == 1) {
            for (; x + 1 < n_bulk; x += 2) {
                pixel(model, std::false_type{}, set1);
                pixel(model, std::false_type{}, set0);
            }
        } else {  // (interleaved channels: a pixel is several samples already)
            for (; x < n_bulk; ++x) pixel(model, std::false_type{}, set0);
        }
        for (; x < r.sw; ++x) pixel(model, std::false_type{}, set1);
        if (bad) atomicOr(status, kStBadExponent);
        asm volatile("global_store_short %0, %1, %2" : : "v"(store_ofs), "v"(held_val), "s"(gbase) : "memory");
        publish_count(counters, kCtrDecReplays, d.replays);
    } else {
        // Neighbours of the row above rotate through registers (tl <- t <- tr); the two values the NEXT pixel needs
        // from memory (top-right, top-top) are loaded while the current one decodes.
        uint64_t* banks;  // [context][lane] per lane group, see the encoder
        uint32_t bsh;
        if constexpr (LDSTAB) {
            banks = reinterpret_cast<uint64_t*>(dyn_lds);
            bsh = 0;
        } else {
            banks = states + ((size_t(id >> g.lane_shift) * kContexts) << g.lane_shift) + (id & ((1u << g.lane_shift) - 1));
            bsh = g.lane_shift;
        }
        if constexpr (NCH == 0) {
            // Any channel count (c > 4, channels interleaved): the plain form -- all six neighbours are read back from the
            // lane-order array this lane has written itself.  Format completeness, not speed.
            const uint32_t nch = g.nch;
            const ptrdiff_t px_step = ptrdiff_t(nch) * GW, up = ptrdiff_t(r.sw) * px_step;
            for (uint32_t y = 0; y < r.sh; ++y) {
                for (uint32_t x = 0; x < r.sw; ++x) {
                    for (uint32_t k = 0; k < nch; ++k) {
                        int16_t* q = p0 + ptrdiff_t(y) * up + ptrdiff_t(x) * px_step + ptrdiff_t(k) * GW;
                        if (window_low(d)) dec_append(d);
                        const Hood n = apply_borders(x > 0 ? q[-px_step] : 0, x > 1 ? q[-2 * px_step] : 0, y > 0 ? q[-up] : 0,
                                                     (y > 0 && x > 0) ? q[-up - px_step] : 0, (y > 0 && x + 1 < r.sw) ? q[-up + px_step] : 0,
                                                     y > 1 ? q[-2 * up] : 0, x, y, r.sw);
                        int ctx = context_hash(n, small_model);
                        const bool neg = ctx < 0;
                        if (neg) ctx = -ctx;
                        const uint64_t b64 = bank_fresh<LDSTAB>(banks[size_t(ctx) << bsh], gpat);
                        Bank bank{{uint32_t(b64), uint32_t(b64 >> 32)}, nullptr};
                        uint32_t v;
                        if (!dec_sample<false>(d, bank, tab, hot, replay_always, v)) {
                            atomicOr(status, kStBadExponent);
                            return;
                        }
                                banks[size_t(ctx) << bsh] = bank_tagged<LDSTAB>(uint64_t(bank.w[0]) | (uint64_t(bank.w[1]) << 32), gpat);
                        if (neg) v = 0u - v;
                        *q = int16_t(uint32_t(predict(n)) + v);
                    }
                }
            }
            publish_count(counters, kCtrDecReplays, d.replays);
        } else {
        const ptrdiff_t up = ptrdiff_t(r.sw) * NCH * GW;  // one slice row back, in lane-order elements
        uint32_t held_ctx = ~0u;   // context of the previous sample; its updated bank is still in registers
        uint64_t held_bank = 0;
        [[maybe_unused]] uint64_t wb_bank = 0;       // CACHE: the victim of this sample's miss, written back behind the decoding
        [[maybe_unused]] uint64_t* wb_ptr = nullptr;
        // CACHE: every four rows from row 8 on the wavefront looks at the hit rate of the last four; content whose contexts do not
        // come back soon enough (a dithered gradient: 1600 contexts in a 64x64 slice, 4 % hits behind the first rows) pays for the
        // cache path without saving a transaction -- the entries are written back once and the rest of the slices runs on the plain
        // path (profiles/r05_bank_cache_ab.txt).  Every lane counts ITS misses and look-ups (the lanes of a ragged wavefront leave a
        // row at different x, so a count kept "per wavefront" inside the sample loop is not one); at the check the lanes add them up
        // in LDS and all read the same two sums: the decision is wave-uniform by construction.  The same per-lane totals feed the
        // event counters at the end (kCtrCache*); the host takes the cache away from a codec whose wavefronts all give it up
        // (codec.hip: the plain kernel holds no LDS for it).
        [[maybe_unused]] bool use_cache = CACHE != 0;
        [[maybe_unused]] uint32_t my_miss = 0, my_lookups = 0, my_wb = 0, miss_mark = 0, look_mark = 0;
        LLMI_PARTS_DECL();
        LLMI_PARTS_START();
        for (uint32_t y = 0; y < r.sh; ++y) {
            if constexpr (CACHE != 0) {
                const uint32_t yu = __builtin_amdgcn_readfirstlane(y);
                if (use_cache && yu >= 4 && (yu & 3) == 0) {  // (the counts start over at row 4: the first rows hit more than the rest)
                    __hip_atomic_fetch_add(&wave_sums[0], my_miss - miss_mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&wave_sums[1], my_lookups - look_mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    miss_mark = my_miss;
                    look_mark = my_lookups;
                    // (one wavefront per block: its LDS operations execute in program order, the adds of all lanes before the loads)
                    const uint32_t n_miss = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&wave_sums[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    const uint32_t n_seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&wave_sums[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    __hip_atomic_store(&wave_sums[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(&wave_sums[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (yu >= 8 && n_miss * 8 > n_seen * 7) {  // fewer than 1 hit in 8 over the last four rows
                        const uint64_t* c_banks = reinterpret_cast<const uint64_t*>(dyn_lds) + threadIdx.x;
                        const uint8_t* c_tags = dyn_lds + (512u << CACHE) + threadIdx.x;
#pragma unroll 1
                        for (uint32_t e = 0; e < (1u << CACHE); ++e) {
                            const uint32_t tg = c_tags[e * 64];
                            if (tg != 0xFFu) banks[size_t((tg << CACHE) | e) << bsh] = bank_tagged<false>(c_banks[e * 64], gpat);
                        }
                        use_cache = false;
                        held_ctx = ~0u;
                    }
                }
                if (use_cache) my_lookups += r.sw * NCH;  // (this row's; a lane that leaves on a bad exponent loses a row of them)
            }
            int16_t* row = p0 + ptrdiff_t(y) * up;
            int l[NCH], L[NCH], t[NCH], tl[NCH], tr[NCH], T[NCH];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                l[k] = L[k] = tl[k] = 0;
                t[k] = y > 0 ? row[k * GW - up] : 0;
                tr[k] = (y > 0 && r.sw > 1) ? row[(k + NCH) * GW - up] : 0;
                T[k] = y > 1 ? row[k * GW - 2 * up] : 0;
            }
            // The row's first neighbours are waited for HERE, once per row.  Their first use is inside the sample loop, and a
            // wait that hipcc places there runs for every sample -- as vmcnt(0), behind the stores of the sample before.
            drain_vector_memory();
            for (uint32_t x = 0; x < r.sw; ++x) {
                int16_t* q = row + ptrdiff_t(x) * NCH * GW;
                int tr_n[NCH], T_n[NCH];
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    tr_n[k] = (y > 0 && x + 2 < r.sw) ? q[(k + 2 * NCH) * GW - up] : 0;
                    T_n[k] = (y > 1 && x + 1 < r.sw) ? q[(k + NCH) * GW - 2 * up] : 0;
                }
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    if (window_low(d)) dec_append(d);
                    const Hood n = apply_borders(l[k], L[k], t[k], tl[k], tr[k], T[k], x, y, r.sw);
                    int ctx = context_hash_lut(n, quant_lut, small_model);
                    const bool neg = ctx < 0;  // llcomp.hpp:511-515
                    if (neg) ctx = -ctx;
                    // The bank just updated stays in registers next to its write-through copy in the table.  On smooth content
                    // most samples stay in the context of their predecessor, and when EVERY lane of the wavefront does, the
                    // table read -- the one memory round trip that hangs on the sample just decoded -- is skipped.  The test
                    // is wave-uniform: lanes never diverge here, and rough content pays one compare.
                    uint64_t* c_bank = nullptr;
#ifdef LLMI_CLOCK_PROBE
                    asm volatile("" : "+v"(ctx));
                    LLMI_PARTS_LAP(0);
#endif
                    if (CACHE != 0 && use_cache) {
                        // bank and tag of the context's cache entry are requested together; on a miss the victim goes back to
                        // the table (one sector write) and the context's bank is fetched (one line fill)
                        const uint32_t entry = uint32_t(ctx) & ((1u << CACHE) - 1), want = uint32_t(ctx) >> CACHE;
                        c_bank = reinterpret_cast<uint64_t*>(dyn_lds) + entry * 64 + threadIdx.x;
                        uint8_t* c_tag = dyn_lds + (512u << CACHE) + entry * 64 + threadIdx.x;
                        const uint32_t have = *c_tag;
                        held_bank = *c_bank;
                        if (have != want) {
                            ++my_miss;
                            // (the victim leaves only behind this sample's decoding: a store issued here would sit in the
                            // queue in front of the fill, and the fill's data come back in order behind it)
                            if (have != 0xFFu) {
                                ++my_wb;
                                wb_bank = bank_tagged<false>(held_bank, gpat);
                                wb_ptr = banks + (size_t((have << CACHE) | entry) << bsh);
                            }
                            held_bank = bank_fresh<false>(banks[size_t(ctx) << bsh], gpat);
                            *c_tag = uint8_t(want);
                        }
                    } else {
                    if (__builtin_amdgcn_ballot_w64(uint32_t(ctx) != held_ctx) != 0) held_bank = bank_fresh<LDSTAB>(banks[size_t(ctx) << bsh], gpat);
                    held_ctx = uint32_t(ctx);
                    }
#ifdef LLMI_CLOCK_PROBE
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(held_bank) : : "memory");
                    LLMI_PARTS_LAP(1);
#endif
                    // ONE drain of the vector-memory queue per sample, where the bank is needed anyway: the neighbours requested for
                    // the next sample, the stream dword requested by the top-up and the stores of the sample before are then all
                    // known to be done, on every path (also when the table read was skipped) -- so hipcc needs no wait of its own at
                    // the head of the next sample, where it would stand in front of the context arithmetic as vmcnt(0) right behind
                    // this sample's stores and the neighbour loads just issued: a second memory round trip per sample, serialised
                    // with the bank fetch (45 % of a sample's 11 000 cycles at 16 frames, profiles/r05_dec2d_parts.jsonl).
                    drain_vector_memory();
                    Bank bank{{uint32_t(held_bank), uint32_t(held_bank >> 32)}, nullptr};
                    uint32_t v;
                    const bool ok = dec_sample<false>(d, bank, tab, hot, replay_always, v);
                    if (!ok) {
                        atomicOr(status, kStBadExponent);
                        return;  // this lane's slice is unusable; the whole call reports the error
                    }
#ifdef LLMI_CLOCK_PROBE
                    asm volatile("" : "+v"(v), "+v"(bank.w[0]), "+v"(bank.w[1]));
                    LLMI_PARTS_LAP(2);
#endif
                    held_bank = uint64_t(bank.w[0]) | (uint64_t(bank.w[1]) << 32);
                    if (CACHE != 0 && use_cache) {
                        *c_bank = held_bank;
                        if (wb_ptr) {
                            *wb_ptr = wb_bank;
                            wb_ptr = nullptr;
                        }
                    } else banks[size_t(ctx) << bsh] = bank_tagged<LDSTAB>(held_bank, gpat);
                    if (neg) v = 0u - v;
                    const int val = int(int16_t(uint32_t(predict(n)) + v));
                    q[k * GW] = int16_t(val);
                    L[k] = l[k];
                    l[k] = val;
                    tl[k] = t[k];
                    t[k] = tr[k];
                    tr[k] = tr_n[k];
                    T[k] = T_n[k];
#ifdef LLMI_CLOCK_PROBE
                    asm volatile("" : "+v"(l[k]), "+v"(t[k]));
                    LLMI_PARTS_LAP(3);
#endif
                }
            }
        }
        LLMI_PARTS_FLUSH();
        if constexpr (CACHE != 0) {  // event counters of the cached decoder: one atomic each per wavefront
            publish_count(counters, kCtrCacheLookups, my_lookups);
            publish_count(counters, kCtrCacheMisses, my_miss);
            publish_count(counters, kCtrCacheWritebacks, my_wb);
            const unsigned long long live = __ballot(1), gave_up = __ballot(!use_cache);
            if (counters && threadIdx.x == uint32_t(__builtin_ctzll(live))) {
                atomicAdd(counters + kCtrDecCachedWaves, 1ull);
                if (gave_up) atomicAdd(counters + kCtrDecBypassedWaves, 1ull);
            }
        }
        publish_count(counters, kCtrDecReplays, d.replays);
        }
    }
    LLMI_PROBE_STOP(1);
}

}  // namespace

#ifdef LLMI_CLOCK_PROBE
// diagnostic library only: copies the stamps out (u64[2][slots][2]) and clears them; returns the slot count
extern "C" uint32_t llcomp_mi_probe_read(unsigned long long* out) {
    if (out) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_probe), sizeof(g_probe));
        static unsigned long long zeros[2][kProbeSlots][2];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_probe), zeros, sizeof(g_probe));
    }
    return kProbeSlots;
}
// the 2-D decoder's per-sample parts (u64[slots][4] shader cycles summed over a wavefront's samples)
extern "C" void llcomp_mi_probe_read_parts(unsigned long long* out) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_probe_parts), sizeof(g_probe_parts));
}
#endif

// (channels per slice, 1-row slices, state table in LDS) -> template instance
#define LLMI_DISPATCH_SLICE(nch, rows, lds, ...)                                                             \
    switch (((nch) > 4 ? 0 : (nch)) * 4 + ((rows) ? 2 : 0) + ((lds) ? 1 : 0)) {                               \
        case 0: { constexpr int C = 0; constexpr bool R = false; constexpr bool T = false; __VA_ARGS__; } break;    \
        case 1: { constexpr int C = 0; constexpr bool R = false; constexpr bool T = true; __VA_ARGS__; } break;     \
        case 4: { constexpr int C = 1; constexpr bool R = false; constexpr bool T = false; __VA_ARGS__; } break;    \
        case 5: { constexpr int C = 1; constexpr bool R = false; constexpr bool T = true; __VA_ARGS__; } break;     \
        case 6: { constexpr int C = 1; constexpr bool R = true; constexpr bool T = false; __VA_ARGS__; } break;     \
        case 8: { constexpr int C = 2; constexpr bool R = false; constexpr bool T = false; __VA_ARGS__; } break;    \
        case 9: { constexpr int C = 2; constexpr bool R = false; constexpr bool T = true; __VA_ARGS__; } break;     \
        case 10: { constexpr int C = 2; constexpr bool R = true; constexpr bool T = false; __VA_ARGS__; } break;    \
        case 12: { constexpr int C = 3; constexpr bool R = false; constexpr bool T = false; __VA_ARGS__; } break;   \
        case 13: { constexpr int C = 3; constexpr bool R = false; constexpr bool T = true; __VA_ARGS__; } break;    \
        case 14: { constexpr int C = 3; constexpr bool R = true; constexpr bool T = false; __VA_ARGS__; } break;    \
        case 16: { constexpr int C = 4; constexpr bool R = false; constexpr bool T = false; __VA_ARGS__; } break;   \
        case 17: { constexpr int C = 4; constexpr bool R = false; constexpr bool T = true; __VA_ARGS__; } break;    \
        case 18: { constexpr int C = 4; constexpr bool R = true; constexpr bool T = false; __VA_ARGS__; } break;    \
        default: return hipErrorInvalidValue;                                                               \
    }

// Kernel family of a geometry (fixed in make_geometry, geometry.hpp): 1-row slices keep their three contexts in LDS,
// a launch with one slice per wavefront keeps that slice's whole table in LDS, everything else needs tables in HBM.
bool rows_mode(const Geometry& g) { return (g.flags & kGeoRows) != 0; }
static bool states_in_lds(const Geometry& g) { return (g.flags & kGeoLdsTable) != 0; }
bool slices_need_state_tables(const Geometry& g) { return !rows_mode(g) && !states_in_lds(g); }

constexpr size_t kLdsTableBytes = size_t(kContexts) * 8;
template <typename K>
hipError_t allow_big_lds(K kernel) {  // more than the default 64 KB of LDS per block (static + dynamic)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(kLdsTableBytes));
}

// (not when the coder runs in segments -- slices above 4096 samples through the snapshot pass: a lane whose slice ended in an earlier
// segment is not there when the last one adds up)
static bool coder_in_segments(const Geometry& g) { return (g.flags & kGeoSnapshot) != 0 && snapshot_chunks(g) > 1; }
bool encoder_writes_group_sums(const Geometry& g) { return g.lpw == (1u << g.lane_shift) && !coder_in_segments(g); }

// One segment (4096 samples of every slice) of the snapshot coder: launch_snapshot has prepared banks and residuals of that chunk.
hipError_t launch_encode_segment(const Geometry& g, const void* d_res, uint64_t* d_banks, uint8_t* d_scratch, uint32_t* d_slice_len,
                                 uint32_t* d_status, unsigned long long* d_counters, uint32_t seg_first, uint32_t* d_seg_state,
                                 hipStream_t stream) {
    if (!coder_in_segments(g) || !d_seg_state) return hipErrorInvalidValue;
    const uint32_t blocks = (g.n_slices + g.lpw - 1) / g.lpw;
    k_encode_slices<0, false, uint32_t, false, true, true><<<dim3(blocks), dim3(64), LLMI_ASM_ENC ? kRowsEncLdsBytes : 0, stream>>>(
        g, g.lpw, static_cast<const uint32_t*>(d_res), d_banks, d_scratch, d_slice_len, nullptr, d_status, 0, d_counters, seg_first, d_seg_state);
    return hipGetLastError();
}

// generation (1..255) -> the tag bits of a bank: bit i of the generation in the top bit of state byte i; 0 for tables in LDS
uint64_t state_generation_tag(uint32_t generation) {
    uint64_t t = 0;
    for (int i = 0; i < 8; ++i) t |= uint64_t((generation >> i) & 1u) << (8 * i + 7);
    return t;
}

hipError_t launch_encode_slices(const Geometry& g, const void* d_sym, uint64_t* d_states, uint32_t generation, uint8_t* d_scratch,
                                uint32_t* d_slice_len, uint64_t* d_group_off, uint32_t* d_status, unsigned long long* d_counters,
                                hipStream_t stream) {
    const uint64_t gpat = slices_need_state_tables(g) ? state_generation_tag(generation) : 0;
    const uint32_t lpw = g.lpw;
    const uint32_t blocks = (g.n_slices + lpw - 1) / lpw;
    uint64_t* const d_group_sum = encoder_writes_group_sums(g) ? d_group_off : nullptr;
    if (rows_encoder_reads_pixels(g)) {  // planar 1-row slices: the ROWS kernel reads the pixels and runs stage A itself
        auto kernel = (g.flags & kGeoSmallModel) ? k_encode_slices<1, true, uint8_t, false, false, false, true> : k_encode_slices<1, true, uint8_t>;
        kernel<<<dim3(blocks), dim3(64), LLMI_ASM_ENC ? kRowsEncLdsBytes : 0, stream>>>(
            g, lpw, static_cast<const uint8_t*>(d_sym), d_states, d_scratch, d_slice_len, d_group_sum, d_status, gpat, d_counters, 0u, nullptr);
        return hipGetLastError();
    }
    if (model_is_fused(g)) {  // ... tiles too wide for that: 16-bit symbols from launch_model_rows_fwd
        k_encode_slices<1, true, uint16_t><<<dim3(blocks), dim3(64), LLMI_ASM_ENC ? kRowsEncLdsBytes : 0, stream>>>(
            g, lpw, static_cast<const uint16_t*>(d_sym), d_states, d_scratch, d_slice_len, d_group_sum, d_status, gpat, d_counters);
        return hipGetLastError();
    }
    if (g.flags & kGeoSnapshot) {  // d_sym: residuals, d_states: banks before each sample (launch_snapshot), both in piece layout
        k_encode_slices<0, false, uint32_t, false, true><<<dim3(blocks), dim3(64), LLMI_ASM_ENC ? kRowsEncLdsBytes : 0, stream>>>(
            g, lpw, static_cast<const uint32_t*>(d_sym), d_states, d_scratch, d_slice_len, d_group_sum, d_status, 0, d_counters);
        return hipGetLastError();
    }
    const bool lds = states_in_lds(g);
    LLMI_DISPATCH_SLICE(g.nch, rows_mode(g), lds, {
        auto kernel = k_encode_slices<C, R, uint32_t, T>;
        if (T) {
            const hipError_t e = allow_big_lds(kernel);
            if (e != hipSuccess) return e;
        }
        kernel<<<dim3(blocks), dim3(64), T ? kLdsTableBytes : (R && LLMI_ASM_ENC ? kRowsEncLdsBytes : 0), stream>>>(
            g, lpw, static_cast<const uint32_t*>(d_sym), d_states, d_scratch, d_slice_len, d_group_sum, d_status, gpat, d_counters, 0u, nullptr);
    });
    return hipGetLastError();
}

hipError_t launch_decode_slices(const Geometry& g, const uint8_t* d_units, const uint32_t* d_slice_len,
                                uint64_t* d_states, uint32_t generation, int16_t* d_rec, uint32_t* d_status, unsigned long long* d_counters,
                                bool bank_cache, hipStream_t stream) {
    const uint64_t gpat = slices_need_state_tables(g) ? state_generation_tag(generation) : 0;
    const uint32_t lpw = g.lpw;
    const uint32_t blocks = (g.n_slices + lpw - 1) / lpw;
    const uint32_t arg = lpw | ((g.flags & kGeoForceReplay) ? 0x100u : 0u);  // tests: rollback + checked replay everywhere
    const bool lds = states_in_lds(g);
    // 2-D slices, tables in HBM, 1..4 channels: per-lane bank cache in LDS -- unless the caller takes it away for this launch (codec.hip:
    // a codec whose wavefronts all gave the cache up last time runs the plain kernel, which holds no LDS for it)
    if (bank_cache_log2(g) == kBankCacheLog2 && bank_cache) {
#define LLMI_DECODE_CACHED(NCHV)                                                                                          \
    k_decode_slices<NCHV, false, false, kBankCacheLog2><<<dim3(blocks), dim3(64), bank_cache_lds_bytes(kBankCacheLog2), stream>>>( \
        g, arg, d_units, d_slice_len, d_states, d_rec, d_status, gpat, d_counters)
        switch (g.nch) {
            case 1: LLMI_DECODE_CACHED(1); break;
            case 2: LLMI_DECODE_CACHED(2); break;
            case 3: LLMI_DECODE_CACHED(3); break;
            case 4: LLMI_DECODE_CACHED(4); break;
            default: return hipErrorInvalidValue;
        }
#undef LLMI_DECODE_CACHED
        return hipGetLastError();
    }
    LLMI_DISPATCH_SLICE(g.nch, rows_mode(g), lds, {
        auto kernel = k_decode_slices<C, R, T>;
        if constexpr (R) {  // the 1-row-slice kernels have the model as a template flag
            if (g.flags & kGeoSmallModel) kernel = k_decode_slices<C, R, T, 0, true>;
        }
        if (T) {
            const hipError_t e = allow_big_lds(kernel);
            if (e != hipSuccess) return e;
        }
        kernel<<<dim3(blocks), dim3(64), T ? kLdsTableBytes : 0, stream>>>(g, arg, d_units, d_slice_len, d_states,
                                                                          d_rec, d_status, gpat, d_counters);
    });
    return hipGetLastError();
}

}  // namespace llcomp_mi
