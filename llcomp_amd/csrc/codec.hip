// codec.hip -- the device-resident batch codec of libllcomp_mi.so (llcomp_mi_codec_*: frames stay in HBM, work is
// enqueued on the caller's HIP stream) and the small status / version entry points of the C ABI.
// Every byte of coded data is produced by the kernels in model_kernels.hip / slice_kernels.hip; there is no CPU coding
// path anywhere in this library.  Host-buffer drop-in calls: hostapi.hip.  Streaming pipeline: stream.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "codec_internal.hpp"
#include "container.hpp"
#include "geometry.hpp"
#include "batch_ops.hpp"
#include "kernels.hpp"
#include "mix.hpp"
#include "compose.hpp"
#include "compose_rule.hpp"
#include "label_boxes.hpp"
#include "label_boxes_rule.hpp"
#include "label_lists.hpp"
#include "label_targets.hpp"
#include "orient.hpp"
#include "orient_rule.hpp"
#include "alpha.hpp"
#include "alpha_rule.hpp"
#include "paste.hpp"
#include "paste_rule.hpp"
#include "photo.hpp"
#include "resize.hpp"
#include "snapshot.hpp"
#include "tables.hpp"
#include "update.hpp"
#include "warp.hpp"
#include "windows_plan.hpp"

using namespace llcomp_mi;

namespace llcomp_mi {

int status_from_bits(uint32_t bits) {
    if (bits & kStInternal) return LLCOMP_MI_HIP_ERROR;
    if (bits & kStBadExponent) return LLCOMP_MI_BAD_EXPONENT;
    if (bits & kStTruncated) return LLCOMP_MI_TRUNCATED;
    if (bits & kStOverflow) return LLCOMP_MI_OUTPUT_OVERFLOW;
    return LLCOMP_MI_OK;
}

int resolve_device(int32_t device, int* out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return LLCOMP_MI_NO_DEVICE;
    if (device < 0) {
        if (hipGetDevice(out) != hipSuccess) return LLCOMP_MI_NO_DEVICE;
        return LLCOMP_MI_OK;
    }
    if (device >= n) return LLCOMP_MI_BAD_ARGS;
    *out = device;
    return LLCOMP_MI_OK;
}

// The test / tuning hooks of the environment are read ONCE per process (first use) -- never per call or per launch;
// llcomp_mi_reload_tuning() (tests) reads them again.
static std::mutex g_tuning_mu;
static bool g_tuning_loaded = false;
static Tuning g_tuning;
Tuning current_tuning() {
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    if (!g_tuning_loaded) {
        g_tuning = tuning_from_env();
        g_tuning_loaded = true;
    }
    return g_tuning;
}

int check_shape(uint32_t w, uint32_t h, uint32_t c, bool legacy) {
    if (!w || !h || c < 1 || c > kMaxChannels) return LLCOMP_MI_BAD_ARGS;
    if (uint64_t(w) * h * c >= (1ull << 31)) return LLCOMP_MI_OUT_OF_RANGE;  // llcomp.hpp:359 `int size`
    if (legacy && (w > 65535 || h > 65535)) return LLCOMP_MI_OUT_OF_RANGE;  // u16 header fields, llcomp.hpp:377-378
    return LLCOMP_MI_OK;
}

}  // namespace llcomp_mi

namespace {

#define HIP_TRY(expr) LLMI_HIP_TRY(expr)

// The caller's tables and result words are read and written as what they are declared to be (u32 / u64 loads and stores, atomics on the
// status word): a pointer of that kind that does not have its type's alignment is BAD_ARGS before anything is launched or written
// (include/llcomp_mi.h, "Alignment of the device pointers").  Pixels, payloads and d_rect may sit at any byte address.  NULL passes: the
// calls that allow a NULL table check for it themselves.
inline bool misaligned(const void* p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }

// brackets a group of launches with two events when profiling is on
struct Timed {
    llcomp_mi_codec* k;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    int slot;
    Timed(llcomp_mi_codec* k_, hipStream_t s_, int slot_) : k(k_), s(s_), slot(slot_) {
        if (!k->profiling) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, s);
    }
    ~Timed() {
        if (!a) return;
        (void)hipEventRecord(b, s);
        k->spans.push_back({a, b, slot});
    }
};

// State tables in HBM are tagged with the generation of the call that wrote them instead of being cleared per call
// (kernels.hpp): a real clear happens before the first call and whenever the 8-bit generation would repeat.
// (need: the geometry about to run keeps its tables in HBM -- the codec's own, or a region's sub-geometry, which may need them where the
// full geometry does not; the table is sized for the full geometry either way, and region_fits makes sure that is enough)
int ensure_state_tables(llcomp_mi_codec* k, bool need) {
    if (!need || k->d_states) return LLCOMP_MI_OK;
    const Geometry& g = k->g;
    if (dev_alloc(reinterpret_cast<void**>(&k->d_states), (uint64_t(lane_groups(g)) * kContexts << g.lane_shift) * 8) != hipSuccess) {
        k->d_states = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    k->allocated_bytes += (uint64_t(lane_groups(g)) * kContexts << g.lane_shift) * 8;
    k->state_generation = 0;
    return LLCOMP_MI_OK;
}
int next_state_generation(llcomp_mi_codec* k, hipStream_t s, bool need) {
    if (!need) return LLCOMP_MI_OK;
    // first call that needs the tables (an encode-only codec with the snapshot pass never gets here; llcomp_mi_codec_prepare allocates them ahead)
    if (int rc = ensure_state_tables(k, true)) return rc;
    if (k->state_generation == 0 || k->state_generation >= 255) {
        const Geometry& g = k->g;
        if (k->state_generation >= 255) ++k->host_counters[kCtrGenerationWraps];
        HIP_TRY(hipMemsetAsync(k->d_states, 0, (uint64_t(lane_groups(g)) * kContexts << g.lane_shift) * 8, s));
        k->state_generation = 0;
    }
    ++k->state_generation;
    return LLCOMP_MI_OK;
}

// LLCOMP_MI_OVERLAP=2: one second stream per device for the snapshot passes of ALL codec objects (created once, never destroyed)
hipStream_t shared_second_stream(int device) {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[device]) {
        // the highest priority: priority streams sit on hardware queues of their own.  An ordinary stream can land on the queue the
        // caller's stream uses (the NULL stream of a one-pipeline caller did: no overlap at all, 2 419 instead of 2 731 MPix/s at 16
        // frames of 128x128 planes, 3 844 instead of 4 410 at 32; profiles/r06_chunked_snapshot_ab.txt)
        int least = 0, greatest = 0;
        const bool prio = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
        const hipError_t rc = prio ? hipStreamCreateWithPriority(&streams[device], hipStreamNonBlocking, greatest)
                                   : hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking);
        if (rc != hipSuccess) {
            (void)hipGetLastError();
            streams[device] = nullptr;
        }
    }
    return streams[device];
}

// the snapshot pass's arrays (2-D encoder): allocated by the first encode -- a decode-only codec never pays for them.
// g: the geometry about to run -- the codec's own, whose arrays hold every sub-geometry's too (region_encode_fits), or a region update's
// sub-geometry that runs the pass where the codec's family does not: then the arrays are sized for what the call needs and grown
// geometrically, up to region_snapshot_bound (the old ones may still be used by the codec's last call: that call is waited for).
int ensure_snapshot_arrays(llcomp_mi_codec* k, const Geometry& g) {
    const bool own = snapshot_mode(k->g);
    const bool chunked = snapshot_chunked(g);
    const uint64_t need = snapshot_elems(g);
    // (ready: the arrays AND, for chunks, the parking records with the second stream's events behind them -- one condition, so that a
    // call which ran out of memory half way is not taken for one that set everything up)
    if (k->d_snap_sorted && need <= k->snap_el && (!chunked || (k->d_snap_ctx && k->d_seg_state))) return LLCOMP_MI_OK;
    const uint64_t el = own ? snapshot_elems(k->g) : std::max(need, std::min(2 * k->snap_el, region_snapshot_bound(k->g)));
    const bool with_chunks = own ? snapshot_chunked(k->g) : true;  // (a region of a codec without the pass: its slices may be above 4096 samples)
    // the coder's parking records, the second stream and the events of the fork / join come FIRST: a failure here changes nothing, and one
    // of the arrays below leaves records that are complete and counted
    if (with_chunks && !k->d_seg_state) {
        if (dev_alloc(reinterpret_cast<void**>(&k->d_seg_state), uint64_t(k->g.n_slices) * 64) != hipSuccess) { k->d_seg_state = nullptr; return LLCOMP_MI_NOMEM; }
        k->allocated_bytes += uint64_t(k->g.n_slices) * 64;
        if (k->overlap) {
            bool ok = (k->aux_shared ? (k->aux = shared_second_stream(k->device)) != nullptr
                                     : hipStreamCreateWithFlags(&k->aux, hipStreamNonBlocking) == hipSuccess) &&
                      hipEventCreateWithFlags(&k->ev_fork, hipEventDisableTiming) == hipSuccess;
            for (uint32_t c = 0; ok && c < kSnapMaxChunks; ++c)
                if (!k->ev_chunk[c]) ok = hipEventCreateWithFlags(&k->ev_chunk[c], hipEventDisableTiming) == hipSuccess;
            if (!ok) {  // no second stream to be had: the pass runs on the caller's (slower at few frames in flight, same bytes)
                (void)hipGetLastError();
                k->overlap = false;
            }
        }
    }
    if (k->d_snap_sorted) {
        if (k->done && k->done->ev && hipEventSynchronize(k->done->ev) != hipSuccess) return LLCOMP_MI_HIP_ERROR;
        dev_free(k->d_snap_sorted);
        dev_free(k->d_snap_banks);
        dev_free(k->d_snap_res);
        dev_free(k->d_snap_ctx);
        dev_free(k->d_snap_io);
        k->allocated_bytes -= k->snap_el * (k->d_snap_ctx ? 28 : 18);
        k->d_snap_sorted = k->d_snap_banks = k->d_snap_res = k->d_snap_ctx = k->d_snap_io = nullptr;
        k->snap_el = 0;
    }
    if (dev_alloc(&k->d_snap_sorted, el * 8) != hipSuccess || dev_alloc(&k->d_snap_banks, el * 8) != hipSuccess ||
        dev_alloc(&k->d_snap_res, el * 2) != hipSuccess ||
        (with_chunks && (dev_alloc(&k->d_snap_ctx, el * 2) != hipSuccess || dev_alloc(&k->d_snap_io, el * 8) != hipSuccess))) {
        dev_free(k->d_snap_sorted);
        dev_free(k->d_snap_banks);
        dev_free(k->d_snap_res);
        dev_free(k->d_snap_ctx);
        dev_free(k->d_snap_io);
        k->d_snap_sorted = k->d_snap_banks = k->d_snap_res = k->d_snap_ctx = k->d_snap_io = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    k->snap_el = el;
    k->allocated_bytes += el * (with_chunks ? 28 : 18);
    return LLCOMP_MI_OK;
}

// What the decode chain and the encoder on geometry g allocate at their first call: every entry point asks for it AHEAD of the first
// thing it queues or writes, so that LLCOMP_MI_NOMEM leaves the outputs, the status word and the stream as BAD_ARGS does
// (include/llcomp_mi.h, by the status codes).  next_state_generation and encode_streams then find everything in place.
int ensure_decode(llcomp_mi_codec* k, const Geometry& g) { return ensure_state_tables(k, slices_need_state_tables(g)); }
int ensure_encode(llcomp_mi_codec* k, const Geometry& g) {
    if (!snapshot_mode(g) || snapshot_chunked(g))
        if (int rc = ensure_state_tables(k, slices_need_state_tables(g))) return rc;
    return snapshot_mode(g) ? ensure_snapshot_arrays(k, g) : LLCOMP_MI_OK;
}

// The 2-D decoder's bank cache, per LAUNCH (codec_internal.hpp).  A wavefront that finds fewer than one hit in eight gives the cache up
// by itself, but it goes on holding its 18 KB of LDS to the end of the kernel: content that makes EVERY wavefront give up (a dithered
// gradient) paid the occupancy cap and the helper kernels' waits for nothing (round 5: 5 296 -> 4 622 MPix/s at 48 frames x 3).  The
// kernels count {wavefronts, wavefronts that gave up}; when (nearly) all of the last cached launch did, the codec's next kPlainRun
// decode calls run the plain kernel, then one call probes with the cache again.  Nothing waits: a result that has not arrived yet
// leaves things as they are.  Same bytes either way (the tables are per call).
bool use_bank_cache(llcomp_mi_codec* k, const Geometry& g) {
    if (bank_cache_log2(g) == 0) return false;
    if (k->fb_pending && k->fb_event && hipEventQuery(k->fb_event) == hipSuccess) {
        k->fb_pending = false;
        const uint64_t waves = k->h_feedback[0] - k->fb_seen[0], gave_up = k->h_feedback[1] - k->fb_seen[1];
        k->fb_seen[0] = k->h_feedback[0];
        k->fb_seen[1] = k->h_feedback[1];
        if (k->feedback && waves && gave_up * 16 >= waves * 15) k->plain_calls_left = llcomp_mi_codec::kPlainRun;
    } else {
        (void)hipGetLastError();
    }
    if (k->plain_calls_left) {
        --k->plain_calls_left;
        ++k->host_counters[kCtrDecLaunchesPlainByFeedback];
        return false;
    }
    ++k->host_counters[kCtrDecLaunchesCached];
    return true;
}
// ... behind a cached launch: {cached wavefronts, bypassed wavefronts} -> the pinned mailbox, and the event that says it has arrived
void queue_feedback(llcomp_mi_codec* k, hipStream_t s) {
    if (!k->h_feedback) {
        if (host_alloc_pinned(reinterpret_cast<void**>(&k->h_feedback), 16, hipHostMallocDefault) != hipSuccess) { k->h_feedback = nullptr; (void)hipGetLastError(); return; }
        k->h_feedback[0] = k->h_feedback[1] = 0;
        if (hipEventCreateWithFlags(&k->fb_event, hipEventDisableTiming) != hipSuccess) { k->fb_event = nullptr; (void)hipGetLastError(); return; }
    }
    if (!k->fb_event || k->fb_pending) return;  // (the previous answer has not been looked at: its copy may still be in flight)
    if (hipMemcpyAsync(k->h_feedback, k->d_counters + kCtrDecCachedWaves, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipEventRecord(k->fb_event, s) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    k->fb_pending = true;
}

// the codec's completion event: recorded behind the last launch of a call, on the caller's stream
void mark_done(llcomp_mi_codec* k, hipStream_t s) {
    if (!k->done) k->done = llcomp_mi::make_done_event();
    if (k->done && k->done->ev && hipEventRecord(k->done->ev, s) != hipSuccess) (void)hipGetLastError();
}
// ... from a scope guard, so that a call which fails AFTER it has launched kernels leaves the event behind them too (its
// blocks must not be reused while those kernels still run)
struct DoneGuard {
    llcomp_mi_codec* k;
    hipStream_t s;
    ~DoneGuard() { mark_done(k, s); }
};

// region decode: u32 lengths + u64 offsets of the covered slices (at most all of them)
int ensure_region_arrays(llcomp_mi_codec* k) {
    if (k->d_region_len) return LLCOMP_MI_OK;
    const uint64_t n = k->g.n_slices;
    if (dev_alloc(reinterpret_cast<void**>(&k->d_region_len), n * 4) != hipSuccess ||
        dev_alloc(reinterpret_cast<void**>(&k->d_region_off), n * 8) != hipSuccess) {
        dev_free(k->d_region_len);
        dev_free(k->d_region_off);
        k->d_region_len = nullptr;
        k->d_region_off = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    k->allocated_bytes += n * 12;
    return LLCOMP_MI_OK;
}
// region update: the sub-geometry's group offsets (at most one lane group per slice) and the full geometry's for the new table
int ensure_update_arrays(llcomp_mi_codec* k) {
    if (k->d_upd_goff) return LLCOMP_MI_OK;
    const uint64_t bytes = (uint64_t(k->g.n_slices) + 1 + lane_groups(k->g) + 1) * 8;
    if (dev_alloc(reinterpret_cast<void**>(&k->d_upd_goff), bytes) != hipSuccess) {
        k->d_upd_goff = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    k->allocated_bytes += bytes;
    return LLCOMP_MI_OK;
}
// A family that keeps its states on chip for the full geometry may not for a region's: one slice per wavefront (few big slices) can
// become several per wavefront for a sub-image whose tiles were clamped.  (1-row slices stay 1-row slices.)
bool region_may_need_states(const llcomp_mi_codec* k) { return !k->need_states && !rows_mode(k->g); }

// the covered tiles and the sub-geometry of a rectangle; BAD_ARGS for a rectangle the frame does not hold, HIP_ERROR if the
// sub-geometry's arrays would not fit the codec's workspace (region_fits: never by default, checked all the same)
int region_setup(const llcomp_mi_codec* k, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, RegionBox& box, Geometry& sub) {
    const Geometry& g = k->g;
    if (!region_box(g.w, g.h, g.tile_w, g.tile_h, x, y, rw, rh, box)) return LLCOMP_MI_BAD_ARGS;
    if (!region_geometry(g, box, k->tune, sub) || !region_fits(g, sub)) return LLCOMP_MI_HIP_ERROR;
    return LLCOMP_MI_OK;
}

// regions decode: the pinned staging ring with one event per slot (what every regions call copies its tables from) ...
int ensure_regions_ring(llcomp_mi_codec* k) {
    const uint64_t bytes = uint64_t(k->g.frames) * sizeof(RegionsFrame);
    for (uint32_t i = 0; i < llcomp_mi_codec::kRegionsRing; ++i) {
        if (k->h_regions[i]) continue;
        if (host_alloc_pinned(reinterpret_cast<void**>(&k->h_regions[i]), bytes, hipHostMallocDefault) != hipSuccess) {
            k->h_regions[i] = nullptr;
            (void)hipGetLastError();
            return LLCOMP_MI_NOMEM;
        }
        k->h_regions_cap[i] = bytes;
    }
    for (auto& ev : k->regions_ev)
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            ev = nullptr;
            (void)hipGetLastError();
            return LLCOMP_MI_HIP_ERROR;
        }
    return LLCOMP_MI_OK;
}
// ... and the per-frame table in HBM that a regions decode from HBM copies into
int ensure_regions_table(llcomp_mi_codec* k) {
    if (k->d_regions) return LLCOMP_MI_OK;
    if (int rc = ensure_regions_ring(k)) return rc;
    const uint64_t bytes = uint64_t(k->g.frames) * sizeof(RegionsFrame);
    if (dev_alloc(reinterpret_cast<void**>(&k->d_regions), bytes) != hipSuccess) {
        k->d_regions = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    k->allocated_bytes += bytes;
    return LLCOMP_MI_OK;
}
// The ring's next slot, for a call that writes `bytes` to it: the slot's last copy has to have left it (queued four calls ago: this
// waits only when the caller runs that far ahead), and a slot too small is replaced by one of max(bytes, twice its size, at most
// `bound`) bytes.  The caller fills it, queues its copy and then calls regions_slot_queued.
int regions_slot_take(llcomp_mi_codec* k, uint64_t bytes, uint64_t bound, uint32_t& slot) {
    slot = k->regions_slot;
    if (k->regions_ev_live[slot]) {
        if (hipEventSynchronize(k->regions_ev[slot]) != hipSuccess) return LLCOMP_MI_HIP_ERROR;
        k->regions_ev_live[slot] = false;
    }
    if (bytes <= k->h_regions_cap[slot]) return LLCOMP_MI_OK;
    const uint64_t cap = std::max(bytes, std::min(2 * k->h_regions_cap[slot], bound));
    // (the replacement first: a failure leaves the ring as it was, every slot of it still there for the calls that fit)
    uint8_t* grown = nullptr;
    if (host_alloc_pinned(reinterpret_cast<void**>(&grown), cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return LLCOMP_MI_NOMEM;
    }
    (void)host_free_pinned(k->h_regions[slot]);
    k->h_regions[slot] = grown;
    k->h_regions_cap[slot] = cap;
    return LLCOMP_MI_OK;
}
// ... behind the copy out of it, on the caller's stream
int regions_slot_queued(llcomp_mi_codec* k, uint32_t slot, hipStream_t s) {
    HIP_TRY(hipEventRecord(k->regions_ev[slot], s));
    k->regions_ev_live[slot] = true;
    k->regions_slot = (slot + 1) % llcomp_mi_codec::kRegionsRing;
    return LLCOMP_MI_OK;
}

// A buffer `p` of the codec (cap bytes) for `bytes`: grown to max(bytes, twice its size, at most `bound`) when too small.  For the boxes and
// the horizontal pass's rows of a resized regions decode bound = frames * w * h * c, what the boxes never exceed and the rows do not for
// ow <= w.  The old buffer may still be used by the codec's last call: that call is waited for (only a call that grows a buffer waits).
int ensure_grown(llcomp_mi_codec* k, uint8_t*& p, uint64_t& cap, uint64_t bytes, uint64_t bound) {
    if (bytes <= cap) return LLCOMP_MI_OK;
    const uint64_t want = std::max(bytes, std::min(2 * cap, bound));
    if (p) {
        if (k->done && k->done->ev && hipEventSynchronize(k->done->ev) != hipSuccess) return LLCOMP_MI_HIP_ERROR;
        dev_free(p);
        k->allocated_bytes -= cap;
        p = nullptr;
        cap = 0;
    }
    if (dev_alloc(reinterpret_cast<void**>(&p), want) != hipSuccess) {
        p = nullptr;
        return LLCOMP_MI_NOMEM;
    }
    cap = want;
    k->allocated_bytes += want;
    return LLCOMP_MI_OK;
}

// The staging buffer in HBM for `bytes` (bound: stage_bound, plus resized_tables_bound / views_tables_bound for a call with a resample tail)
int ensure_stage(llcomp_mi_codec* k, uint64_t bytes, uint64_t bound) { return ensure_grown(k, k->d_stage, k->stage_cap, bytes, bound); }

// A batch call's table on its way to the device (DESIGN.md "Batch calls: what the three share"): `tab` grown to `bytes` (at most
// `bound`), a slot of the pinned ring, fill(slot) writes the table, ONE copy on s, the slot's event behind it, then launch(tab).  Nothing
// is queued on s before every allocation has succeeded, the one of a second buffer of the call's included (`more`, grown to
// more_bytes behind the table: the mixing's saved heads; 0: none).
template <class Fill, class Launch>
int batch_table_call(llcomp_mi_codec* k, uint8_t*& tab, uint64_t& cap, uint64_t bytes, uint64_t bound, hipStream_t s, Fill&& fill, Launch&& launch,
                     uint8_t** more = nullptr, uint64_t* more_cap = nullptr, uint64_t more_bytes = 0) {
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (int rc = ensure_regions_ring(k)) return rc;
    if (int rc = ensure_grown(k, tab, cap, bytes, bound)) return rc;
    if (more_bytes)
        if (int rc = ensure_grown(k, *more, *more_cap, more_bytes, more_bytes)) return rc;
    uint32_t slot = 0;
    if (int rc = regions_slot_take(k, bytes, bound, slot)) return rc;
    fill(k->h_regions[slot]);
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemcpyAsync(tab, k->h_regions[slot], bytes, hipMemcpyHostToDevice, s));
    if (int rc = regions_slot_queued(k, slot, s)) return rc;
    HIP_TRY(launch(tab));
    return LLCOMP_MI_OK;
}

// The batch copy-paste of either width of id map (DESIGN.md "Batch copy-paste", "Batch copy-paste by 16-bit ids"), P its piece type:
// paste_plan.hpp's checks, plan and table through the width's own table buffer.  A call without a piece that selects anything queues
// nothing.
template <class P>
int paste_batch_call(llcomp_mi_codec* k, uint8_t*& tab, uint64_t& cap, const void* d_src, const void* d_mask, uint32_t n_src, uint32_t iw, uint32_t ih,
                     void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const P* pieces, uint32_t n_pieces,
                     void* stream) {
    constexpr uint32_t MB = kPasteMaskBytesOf<P>;
    if (!k || !d_dst) return LLCOMP_MI_BAD_ARGS;
    const uint32_t c = k->g.c;
    std::vector<uint32_t> value_bits;
    if (int rc = paste_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, value_bits)) return rc;
    const uint32_t esize = batch_esize(dtype);
    if (int rc = paste_check_memory(d_src, uint64_t(n_src) * c * iw * ih * esize, d_mask, MB * uint64_t(n_src) * iw * ih, d_dst,
                                    uint64_t(n_dst) * c * ow * oh * esize, esize, paste_mask_align(MB), n_pieces))
        return rc;
    PastePlan p;
    paste_plan(n_dst, pieces, n_pieces, p);
    if (p.samples.empty()) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, tab, cap, PasteTable<MB>(p.samples.size(), p.order.size()).bytes, paste_table_bound<MB>(n_dst, n_pieces), s,
        [&](uint8_t* at) { paste_table_put(pieces, p, value_bits, c, layout, at); },
        [&](const uint8_t* d_table) {
            PasteLaunch o{};
            o.d_src = static_cast<const uint8_t*>(d_src), o.d_mask = static_cast<const uint8_t*>(d_mask), o.d_dst = static_cast<uint8_t*>(d_dst);
            o.d_table = d_table, o.n_samples = uint32_t(p.samples.size()), o.n_recs = uint32_t(p.order.size());
            o.n_src = n_src, o.iw = iw, o.ih = ih, o.ow = ow, o.oh = oh, o.c = c, o.dtype = dtype, o.layout = layout;
            return launch_paste(o, MB, s);
        });
}

// The decode chain on geometry `sub` -- the codec's own, or the sub-geometry of a region, a box or a class -- in order on `s`: a state
// generation of its own (a sub-geometry maps slices to lane groups differently, and the tagged tables are shared with the full decodes);
// `locate`, which finds the slices' lengths `len` and stages their streams into d_scratch in stream lane order; the decoder, with the
// bank cache's feedback behind it; and the inverse model into `sink(fused, samples)` -- samples: the lane-order array on the fused row
// path, the image-order intermediate otherwise.
template <class Locate, class Sink>
int decode_chain(llcomp_mi_codec* k, const Geometry& sub, const uint32_t* len, uint32_t* d_status, hipStream_t s, Locate&& locate, Sink&& sink) {
    {
        Timed t(k, s, 7);
        if (int rc = next_state_generation(k, s, slices_need_state_tables(sub))) return rc;
    }
    {
        Timed t(k, s, 4);
        if (int rc = locate()) return rc;
    }
    {
        Timed t(k, s, 5);
        const bool cache = use_bank_cache(k, sub);
        HIP_TRY(launch_decode_slices(sub, k->d_scratch, len, k->d_states, k->state_generation, static_cast<int16_t*>(k->d_lane_order), d_status,
                                     k->d_counters, cache, s));
        if (cache) queue_feedback(k, s);
    }
    Timed t(k, s, 6);
    const bool fused = model_is_fused(sub);
    if (!fused) HIP_TRY(launch_from_lane_order_i16(sub, static_cast<const int16_t*>(k->d_lane_order), static_cast<int16_t*>(k->d_sym_or_rec), s));
    return sink(fused, static_cast<const int16_t*>(fused ? k->d_lane_order : k->d_sym_or_rec));
}
// ... the locator of the calls that cut a box out of the full batch in HBM: the full geometry's group offsets, the box's slices in them
int locate_box(llcomp_mi_codec* k, const Geometry& sub, const RegionBox& box, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
               uint32_t* d_status, hipStream_t s) {
    const Geometry& g = k->g;
    HIP_TRY(launch_group_sums(g, static_cast<const uint32_t*>(d_slice_len), k->d_group_off, s));
    HIP_TRY(launch_scan_groups(g, k->d_group_off, k->d_total_tmp, s));
    HIP_TRY(launch_region_index(g, sub, box, static_cast<const uint32_t*>(d_slice_len), k->d_group_off, k->d_region_len, k->d_region_off, s));
    HIP_TRY(launch_stage_region_streams(sub, static_cast<const uint8_t*>(d_payload), payload_bytes, k->d_region_len, k->d_region_off, k->d_scratch,
                                        d_status, s));
    return LLCOMP_MI_OK;
}

// Where the classes of a regions decode find their slices: `payload` (payload_bytes long) and, per slice of a class, its length and offset
// in it -- found by k_regions_index over the FULL table (full_len; the group offsets of the full geometry must be in d_group_off), or
// read from compact arrays that hold every class's slices back to back in class order (staged_len / staged_off: a host-staged call).
struct RegionsSource {
    const uint8_t* payload;
    uint64_t payload_bytes;
    const uint32_t* full_len;
    const uint32_t* staged_len;
    const uint64_t* staged_off;
};
// The decode chain of every class, in order on `s`, each cropping rw x rh per entry into d_px.  d_tab: the per-frame table in HBM (class
// by class, windows_plan.hpp: regions_setup_sized).
int regions_classes(llcomp_mi_codec* k, const RegionsClass* classes, uint32_t n_classes, const RegionsFrame* d_tab, const RegionsSource& src,
                    uint32_t rw, uint32_t rh, uint8_t* d_px, uint32_t* d_status, hipStream_t s) {
    uint64_t base = 0;  // the class's first slice in the staged arrays
    for (uint32_t i = 0; i < n_classes; ++i) {
        const Geometry& sub = classes[i].sub;
        const RegionsFrame* c_tab = d_tab + classes[i].first;
        const uint32_t* len = src.full_len ? k->d_region_len : src.staged_len + base;
        const uint64_t* off = src.full_len ? k->d_region_off : src.staged_off + base;
        base += sub.n_slices;
        const int rc = decode_chain(
            k, sub, len, d_status, s,
            [&]() -> int {
                if (src.full_len)
                    HIP_TRY(launch_regions_index(k->g, sub, c_tab, src.full_len, k->d_group_off, k->d_region_len, k->d_region_off, s));
                HIP_TRY(launch_stage_region_streams(sub, src.payload, src.payload_bytes, len, off, k->d_scratch, d_status, s));
                return LLCOMP_MI_OK;
            },
            [&](bool fused, const int16_t* v) -> int {
                HIP_TRY(fused ? launch_model_rows_inv_crops(sub, v, d_px, c_tab, rw, rh, s) : launch_model_inv_crops(sub, v, d_px, c_tab, rw, rh, s));
                return LLCOMP_MI_OK;
            });
        if (rc) return rc;
    }
    return LLCOMP_MI_OK;
}

// The chains of views [at, at + cnt) of group pg, which lie in d_photo as U8 HWC: step by step on the stream, every view of the chunk
// together (photo.hpp: launch_photo_step); a view's last step writes its place of the group's d_out through the group's format, whose
// table lies at pg.table_at of d_tables.  d_chains: the call's block of chains in HBM.
int windows_photo(llcomp_mi_codec* k, const PhotoTail& photo, const PhotoGroup& pg, const uint8_t* d_tables, const llcomp_mi_photo_chain* d_chains,
                  uint32_t at, uint32_t cnt, hipStream_t s) {
    const uint32_t c = k->g.c;
    const uint64_t view_bytes = uint64_t(pg.oh) * pg.ow * c * pg.out.esize;
    PhotoStep st{};
    st.d_px = k->d_photo, st.d_chains = d_chains + pg.first + at, st.d_halo = pg.halo_at == kPhotoNoHalo ? nullptr : k->d_photo + pg.halo_at;
    st.d_stats = k->d_photo_tab, st.d_luts = k->d_photo_tab + photo.tab_views * photo_stats_stride(c);
    st.out = pg.out, st.d_table = d_tables + pg.table_at, st.d_out = static_cast<uint8_t*>(pg.d_out) + at * view_bytes;
    st.views = cnt, st.c = c, st.ow = pg.ow, st.oh = pg.oh, st.sharp_rows = pg.sharp_rows;
    for (; st.step < pg.steps; ++st.step) {
        st.info = pg.step[st.step];
        HIP_TRY(launch_photo_step(st, s));
    }
    return LLCOMP_MI_OK;
}
const PhotoGroup* photo_group(const PhotoTail* photo, size_t gi) { return photo && photo->groups[gi].active ? &photo->groups[gi] : nullptr; }

// The groups of a tail, one by one behind the classes, timed in slot 6 with the crops: launch(vg, at, cnt, dst) puts views
// [at, at + cnt) of group vg at dst.  A group without photometric chains is one such piece, all its views into its d_out.  A group
// with chains (photo, d_chains) writes plain U8 HWC into d_photo, pg->chunk views at a time, and windows_photo takes every such chunk
// on to the group's output; d_tables: the tail's output tables in HBM.
template <class Group, class Launch>
int windows_groups(llcomp_mi_codec* k, const std::vector<Group>& groups, const uint8_t* d_tables, const PhotoTail* photo,
                   const llcomp_mi_photo_chain* d_chains, hipStream_t s, Launch&& launch) {
    Timed t(k, s, 6);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& vg = groups[gi];
        const PhotoGroup* pg = photo_group(photo, gi);
        const uint32_t pchunk = pg ? pg->chunk : vg.n;
        for (uint32_t pa = 0; pa < vg.n; pa += pchunk) {
            const uint32_t cnt = std::min(pchunk, vg.n - pa);
            if (int rc = launch(vg, pa, cnt, pg ? k->d_photo : static_cast<uint8_t*>(vg.d_out))) return rc;
            if (pg)
                if (int rc = windows_photo(k, *photo, *pg, d_tables, d_chains, pa, cnt, s)) return rc;
        }
    }
    return LLCOMP_MI_OK;
}

// The resample passes of a tail, vg.chunk views per launch: d_block is the tail's block in HBM.
int windows_resample(llcomp_mi_codec* k, const WindowsPlan& p, const ResampleTail& tail, const uint8_t* d_block, const PhotoTail* photo,
                     const llcomp_mi_photo_chain* d_chains, hipStream_t s) {
    const Geometry& g = k->g;
    const ResizeFrame* d_rs = reinterpret_cast<const ResizeFrame*>(d_block);
    const int32_t* d_w = reinterpret_cast<const int32_t*>(d_block + tail.block.w_at());
    const uint8_t* const d_tables = d_block + tail.block.tables_at();
    return windows_groups(k, tail.groups, d_tables, photo, d_chains, s, [&](const ResampleGroup& vg, uint32_t pa, uint32_t n, uint8_t* dst) -> int {
        const uint64_t view_bytes = uint64_t(vg.oh) * vg.ow * g.c * vg.out.esize;
        for (uint32_t at = pa; at < pa + n; at += vg.chunk) {
            const uint32_t cnt = std::min(vg.chunk, pa + n - at);
            // (a padded call with a constant fill other than 0: the bias forms for a chunk that has an entry with a bias, and only for it)
            const std::vector<uint8_t>& biased = tail.block.biased;
            const bool bias = !biased.empty() && std::any_of(biased.begin() + vg.first + at, biased.begin() + vg.first + at + cnt, [](uint8_t b) { return b != 0; });
            if (bias) ++k->host_counters[LLCOMP_MI_CTR_BIAS_LAUNCHES];
            HIP_TRY(launch_resize_out(k->d_box, k->d_mid, dst + (at - pa) * view_bytes, d_rs + vg.first + at, d_w, d_tables + vg.table_at, vg.out, cnt, g.c,
                                      p.wmax, p.hmax, vg.mh, vg.ow, vg.oh, s, bias));
        }
        return LLCOMP_MI_OK;
    });
}

// The gather of a warp tail: d_block is the tail's block in HBM.  One launch per piece -- per group, or per chunk of a group with
// chains -- and no intermediate buffer.
int windows_warp(llcomp_mi_codec* k, const WindowsPlan& p, const WarpTail& tail, const uint8_t* d_block, const PhotoTail* photo,
                 const llcomp_mi_photo_chain* d_chains, hipStream_t s) {
    const Geometry& g = k->g;
    const WarpEntry* d_ws = reinterpret_cast<const WarpEntry*>(d_block);
    const int32_t* d_tabs = reinterpret_cast<const int32_t*>(d_block + tail.tabs_at());
    const uint8_t* const d_tables = d_block + tail.tables_at();
    return windows_groups(k, tail.groups, d_tables, photo, d_chains, s, [&](const WarpOut& vg, uint32_t at, uint32_t cnt, uint8_t* dst) -> int {
        if (!tail.ps.empty()) {  // a perspective call: its own entries, its own gather
            HIP_TRY(launch_persp(k->d_box, reinterpret_cast<const PerspEntry*>(d_block) + vg.first + at, d_block + tail.fills_at() + vg.fill_at,
                                 d_tables + vg.table_at, vg.out, dst, cnt, g.c, p.wmax, p.hmax, g.w, g.h, vg.ow, vg.oh, s));
            return LLCOMP_MI_OK;
        }
        HIP_TRY(launch_warp(k->d_box, d_ws + vg.first + at, d_tabs, d_block + tail.fills_at() + vg.fill_at, d_tables + vg.table_at, vg.out, dst, cnt, g.c,
                            p.wmax, p.hmax, g.w, g.h, vg.ow, vg.oh, s));
        return LLCOMP_MI_OK;
    });
}

// Where a windowed decode finds its slices: the full batch in HBM (d_payload, payload_bytes, d_slice_len), or -- `host` -- the frames'
// containers (data, lens) with the gather planned over the plan's windows (host_gather).
struct WindowsSource {
    const void* d_payload;
    uint64_t payload_bytes;
    const void* d_slice_len;
    const uint8_t* const* data;
    const size_t* lens;
    bool host;
    RegionsGather gather;
};
WindowsSource device_source(const void* d_payload, uint64_t payload_bytes, const void* d_slice_len) {
    return WindowsSource{d_payload, payload_bytes, d_slice_len, nullptr, nullptr, false, {}};
}
WindowsSource host_source(const uint8_t* const* data, const size_t* lens) { return WindowsSource{nullptr, 0, nullptr, data, lens, true, {}}; }
// What every windowed decode refuses before it plans anything: a null codec, source pointer or status word, and a table or status word
// that is not 4-byte aligned
bool source_ok(const llcomp_mi_codec* k, const WindowsSource& src, const void* d_status) {
    if (!k || !d_status || misaligned(d_status, 4)) return false;
    return src.host ? src.data && src.lens : src.d_payload && src.d_slice_len && !misaligned(src.d_slice_len, 4);
}
// The containers of a host source have to be of the codec's shape, tiling, planar setting and model ...
int same_shape(const Geometry& g, const Geometry& cg) {
    return cg.w == g.w && cg.h == g.h && cg.c == g.c && cg.tile_w == g.tile_w && cg.tile_h == g.tile_h && cg.planar == g.planar &&
                   (cg.flags & kGeoSmallModel) == (g.flags & kGeoSmallModel)
               ? LLCOMP_MI_OK
               : LLCOMP_MI_BAD_ARGS;
}
// ... and the gather's slices the classes' (its order is the table's: class by class, and a class's slices are its sub-geometry's)
int gather_matches(const WindowsPlan& p, const WindowsSource& src) {
    uint64_t sub_slices = 0;
    for (uint32_t i = 0; i < p.n_classes; ++i) sub_slices += p.classes[i].sub.n_slices;
    return !src.host || sub_slices == src.gather.n_slices ? LLCOMP_MI_OK : LLCOMP_MI_HIP_ERROR;
}
// The gather of a host source over plan p's windows (container.cpp; nothing for a source in HBM), every error of which comes before
// anything is queued: rects = a rectangle per frame, `used` = the plan's frame list or null for every frame.  A frame list that names
// no frame (a warped views call whose every view is all fill) plans no gather: no container is looked at.
int host_gather(const llcomp_mi_codec* k, WindowsSource& src, const WindowsPlan& p, const uint32_t* rects, const std::vector<uint32_t>* used) {
    if (src.host && !(used && used->empty())) {
        if (int rc = regions_gather_plan_sized(src.data, src.lens, k->g.frames, rects, p.wmax, p.hmax, src.gather, used ? used->data() : nullptr,
                                               used ? uint32_t(used->size()) : 0))
            return rc;
        if (int rc = same_shape(k->g, src.gather.g)) return rc;
    }
    return gather_matches(p, src);
}

// the plan of a plain regions decode: every class crops the rectangle itself
int regions_plan(const llcomp_mi_codec* k, const uint32_t* xy, uint32_t rw, uint32_t rh, WindowsPlan& p) {
    p.tab.resize(k->g.frames);
    p.wmax = rw;
    p.hmax = rh;
    return regions_setup(k->g, k->tune, xy, rw, rh, p.tab.data(), p.classes, p.n_classes);
}

// A call as the driver takes it: the tail is none (the classes crop into d_px), a resample tail or a warp tail.
struct WindowsTail {
    const ResampleTail* resample = nullptr;
    const WarpTail* warp = nullptr;
    WindowsTail() = default;
    WindowsTail(const ResampleTail& t) : resample(&t) {}
    WindowsTail(const WarpTail& t) : warp(&t) {}
    explicit operator bool() const { return resample || warp; }
    uint64_t block_bytes() const { return resample ? resample->block.bytes() : warp ? warp->bytes() : 0; }
};
struct WindowsCall {
    const WindowsPlan& plan;
    WindowsTail tail;
    const PhotoTail* photo;  // the chains beside the tail's groups; null for a call without a chain
    uint64_t tables_bound;   // what the tail's block and the chains add to stage_bound at most
    const WindowsSource& src;
    void* d_px;              // a call without a tail
};

// The driver of every windowed decode (DESIGN.md "Region decode"): the call's plan -- every class crops wmax x hmax per entry -- from its
// source into d_px, or with a tail into the boxes that the tail's groups are resampled from.  Everything the kernels read from the host crosses
// in ONE copy out of a slot of the pinned ring (windows_plan.hpp: CopyLayout): the regions table; for a host source the window slices'
// lengths, offsets and payload bytes behind it, so the classes read their slices straight from the copy and no group sums run; and the
// tail's block at the next multiple of 16.  The copy lands in d_stage, grown up to stage_bound + tables_bound -- but the table alone of
// a plain call from HBM in d_regions.  Each class takes a state generation of its own; for a source in HBM the full geometry's group
// offsets are found once, ahead of the first class.  A warp tail (warp_plan.hpp: WarpTail) carries the block of a warped views decode
// in the same place of the copy and is gathered from the boxes by windows_warp; it has no d_mid.  `photo` (photo_plan.hpp: PhotoTail),
// beside either kind of tail: the views' photometric chains travel at the next multiple of 16 behind the tail's block, and the groups
// that have one go through d_photo (windows_photo).
int decode_windows(llcomp_mi_codec* k, const WindowsCall& c, void* d_status, void* stream) {
    const Geometry& g = k->g;
    const WindowsPlan& p = c.plan;
    const WindowsSource& src = c.src;
    const ResampleTail* tail = c.tail.resample;
    const WarpTail* warp = c.tail.warp;
    const PhotoTail* photo = c.photo;
    const RegionsGather* gp = src.host ? &src.gather : nullptr;
    const bool any_tail = bool(c.tail);
    const CopyLayout cl(p.tab.size(), gp, any_tail, c.tail.block_bytes(), photo ? photo->bytes() : 0);
    const StageLayout& lay = cl.stage;
    const uint64_t bytes = cl.bytes;
    const bool table_only = !gp && !any_tail;
    const uint64_t bound = table_only ? 0 : stage_bound(g) + c.tables_bound;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (!gp)
        if (int rc = ensure_region_arrays(k)) return rc;
    for (uint32_t i = 0; i < p.n_classes; ++i)
        if (int rc = ensure_decode(k, p.classes[i].sub)) return rc;
    if (int rc = any_tail ? ensure_regions_ring(k) : ensure_regions_table(k)) return rc;
    if (!table_only)
        if (int rc = ensure_stage(k, bytes, bound)) return rc;
    if (any_tail) {
        const uint64_t samples = uint64_t(g.frames) * g.w * g.h * g.c;
        if (int rc = ensure_grown(k, k->d_box, k->box_cap, tail ? tail->box_bytes : warp->box_bytes, samples)) return rc;
        if (tail)
            if (int rc = ensure_grown(k, k->d_mid, k->mid_cap, tail->mid_bytes, samples)) return rc;
        if (photo) {
            const uint64_t tab_bytes = photo->tab_views * (photo_stats_stride(g.c) + photo_lut_stride(g.c));
            if (int rc = ensure_grown(k, k->d_photo, k->photo_cap, photo->stage_bytes, samples)) return rc;
            if (int rc = ensure_grown(k, k->d_photo_tab, k->photo_tab_cap, tab_bytes, tab_bytes)) return rc;
        }
    }
    uint32_t slot = 0;
    if (int rc = regions_slot_take(k, bytes, bound, slot)) return rc;
    uint8_t* h = k->h_regions[slot];
    std::memcpy(h, p.tab.data(), p.tab.size() * sizeof(RegionsFrame));
    if (gp) regions_gather_copy(*gp, src.data, h + lay.pay_at, reinterpret_cast<uint32_t*>(h + lay.len_at), reinterpret_cast<uint64_t*>(h + lay.off_at));
    if (tail) tail->block.put(h + cl.rs_at);
    if (warp) warp->put(h + cl.rs_at);
    if (photo) {
        std::memset(h + cl.block_end, 0, size_t(cl.chains_at - cl.block_end));
        photo->put(h + cl.chains_at);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* const d_copy = table_only ? reinterpret_cast<uint8_t*>(k->d_regions) : k->d_stage;
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    {
        Timed t(k, s, 4);
        HIP_TRY(hipMemcpyAsync(d_copy, h, bytes, hipMemcpyHostToDevice, s));
        if (int rc = regions_slot_queued(k, slot, s)) return rc;
        if (!gp && p.n_classes) {  // (no class: a warped views call whose every view is all fill)
            HIP_TRY(launch_group_sums(g, static_cast<const uint32_t*>(src.d_slice_len), k->d_group_off, s));
            HIP_TRY(launch_scan_groups(g, k->d_group_off, k->d_total_tmp, s));
        }
    }
    if (gp) k->host_counters[LLCOMP_MI_CTR_HOST_STAGED_BYTES] += gp->payload_bytes;
    const RegionsSource from = gp ? RegionsSource{d_copy + lay.pay_at, gp->payload_bytes, nullptr, reinterpret_cast<const uint32_t*>(d_copy + lay.len_at),
                                                  reinterpret_cast<const uint64_t*>(d_copy + lay.off_at)}
                                  : RegionsSource{static_cast<const uint8_t*>(src.d_payload), src.payload_bytes,
                                                  static_cast<const uint32_t*>(src.d_slice_len), nullptr, nullptr};
    if (int rc = regions_classes(k, p.classes, p.n_classes, reinterpret_cast<const RegionsFrame*>(d_copy), from, p.wmax, p.hmax,
                                 any_tail ? k->d_box : static_cast<uint8_t*>(c.d_px), static_cast<uint32_t*>(d_status), s))
        return rc;
    const llcomp_mi_photo_chain* d_chains = photo ? reinterpret_cast<const llcomp_mi_photo_chain*>(k->d_stage + cl.chains_at) : nullptr;
    if (tail)
        if (int rc = windows_resample(k, p, *tail, k->d_stage + cl.rs_at, photo, d_chains, s)) return rc;
    if (warp)
        if (int rc = windows_warp(k, p, *warp, k->d_stage + cl.rs_at, photo, d_chains, s)) return rc;
    ++k->n_decode;
    return LLCOMP_MI_OK;
}

// The encoder on geometry g, in the codec's workspace, up to the slices' streams in d_scratch (stream lane order) and their lengths in
// d_slice_len: the codec's own geometry (llcomp_mi_codec_encode) or the sub-geometry of a region update's box, whose kernel family may
// be another one.  d_px: g.frames * g.h * g.w * g.c bytes, exactly (the row encoder that reads pixels sizes its dword reads by it).
// d_group_off: u64[lane groups of g + 1]; it holds the group sums afterwards where encoder_writes_group_sums(g).
int encode_streams(llcomp_mi_codec* k, const Geometry& g, const void* d_px, uint32_t* d_slice_len, uint64_t* d_group_off, uint32_t* d_status,
                   hipStream_t s) {
    // (the snapshot encoder of slices up to 4096 samples never touches the state tables: they are the decoder's alone; above that
    // the pass carries a context's states from chunk to chunk through them, under a generation of its own)
    if (!snapshot_mode(g) || snapshot_chunked(g)) {
        Timed t(k, s, 0);
        if (int rc = next_state_generation(k, s, slices_need_state_tables(g))) return rc;
    }
    {
        Timed t(k, s, 1);
        if (rows_encoder_reads_pixels(g)) {
            // nothing: the coder reads the pixels itself
        } else if (model_is_fused(g)) {
            HIP_TRY(launch_model_rows_fwd(g, static_cast<const uint8_t*>(d_px), static_cast<uint16_t*>(k->d_lane_order), s));
        } else {
            HIP_TRY(launch_model_fwd(g, static_cast<const uint8_t*>(d_px), static_cast<uint32_t*>(k->d_sym_or_rec), s));
            if (!snapshot_mode(g))
                HIP_TRY(launch_to_lane_order_u32(g, static_cast<const uint32_t*>(k->d_sym_or_rec),
                                                 static_cast<uint32_t*>(k->d_lane_order), s));
        }
    }
    if (snapshot_mode(g) && snapshot_chunked(g)) {
        // Slices above 4096 samples: pass and coder chunk by chunk.  The pass of chunk c + 1 needs the WALK of chunk c (the contexts'
        // states travel through the table), the coder of chunk c needs the pass of chunk c only: so the pass runs AHEAD on a second
        // stream and the coder follows on the caller's, each segment behind its chunk's event (fork / join: the caller's stream still
        // orders everything).  A launch of such slices is a few hundred wavefronts -- one wavefront's dependent chain -- and the
        // pass's nine or twelve launches in FRONT of it cost 8-11 % against the table encoder at few frames in flight; beside it they
        // are hidden.  The second stream is ONE PER DEVICE, shared by all codec objects (the passes are throughput kernels: they may
        // queue behind each other): a second stream per codec left the GPU idle as soon as three pipelines made six streams (25 %
        // below in-order; more hardware queues change nothing) -- profiles/r06_chunked_snapshot_ab.txt.  LLCOMP_MI_OVERLAP=0: in order.
        if (int rc = ensure_snapshot_arrays(k, g)) return rc;
        const uint64_t gpat = state_generation_tag(k->state_generation);
        const uint32_t chunks = snapshot_chunks(g);
        hipStream_t ps = k->overlap ? k->aux : s;
        if (k->overlap) {  // fork: the pass starts behind stage A
            HIP_TRY(hipEventRecord(k->ev_fork, s));
            HIP_TRY(hipStreamWaitEvent(k->aux, k->ev_fork, 0));
        }
        auto pass = [&](uint32_t c) -> int {
            Timed t(k, ps, 0);
            HIP_TRY(launch_snapshot_chunk(g, c, static_cast<const uint32_t*>(k->d_sym_or_rec), k->d_lane_order, k->d_snap_sorted, k->d_snap_banks,
                                          k->d_snap_res, k->d_snap_ctx, k->d_snap_io, k->d_states, gpat, ps));
            return LLCOMP_MI_OK;
        };
        auto coder = [&](uint32_t c) -> int {
            Timed t(k, s, 2);
            HIP_TRY(launch_encode_segment(g, k->d_snap_res, static_cast<uint64_t*>(k->d_snap_banks), k->d_scratch, d_slice_len,
                                          d_status, k->d_counters, c * kSnapMaxSamples, k->d_seg_state, s));
            return LLCOMP_MI_OK;
        };
        int rc = LLCOMP_MI_OK;
        if (k->overlap) {
            for (uint32_t c = 0; c < chunks && !rc; ++c) {
                rc = pass(c);
                if (!rc && hipEventRecord(k->ev_chunk[c], k->aux) != hipSuccess) rc = LLCOMP_MI_HIP_ERROR;
            }
            // join: every segment waits for its chunk -- also when something failed above: whatever was queued on the second stream
            // has to be behind the caller's stream before this call returns its buffers to anybody
            for (uint32_t c = 0; c < chunks; ++c) {
                if (hipStreamWaitEvent(s, k->ev_chunk[c], 0) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(k->aux); }
                if (!rc) rc = coder(c);
            }
        } else {
            for (uint32_t c = 0; c < chunks && !rc; ++c) {
                rc = pass(c);
                if (!rc) rc = coder(c);
            }
        }
        if (rc) return rc;
    } else {
    if (snapshot_mode(g)) {  // states replayed ahead of the coder: it reads banks + residuals front to back, no table
        if (int rc = ensure_snapshot_arrays(k, g)) return rc;
        Timed t(k, s, 0);    // (profile slot 0: the pass takes the place of the state tables whose clear the slot times otherwise)
        HIP_TRY(launch_snapshot(g, static_cast<const uint32_t*>(k->d_sym_or_rec), k->d_lane_order, k->d_snap_sorted,
                                k->d_snap_banks, k->d_snap_res, s));
    }
    {
        Timed t(k, s, 2);
        const bool snap = snapshot_mode(g);
        const void* in = snap ? k->d_snap_res : rows_encoder_reads_pixels(g) ? d_px : k->d_lane_order;
        HIP_TRY(launch_encode_slices(g, in, snap ? static_cast<uint64_t*>(k->d_snap_banks) : k->d_states,
                                     k->state_generation, k->d_scratch, d_slice_len,
                                     d_group_off, d_status, k->d_counters, s));
    }
    }
    return LLCOMP_MI_OK;
}
// ... and from there to the packed payload: group sums -> offsets and *d_total, streams -> d_payload (kStOverflow past payload_cap)
int pack_streams(llcomp_mi_codec* k, const Geometry& g, const uint32_t* d_slice_len, uint64_t* d_group_off, uint8_t* d_payload, uint64_t payload_cap,
                 uint64_t* d_total, uint32_t* d_status, hipStream_t s) {
    Timed t(k, s, 3);
    if (!encoder_writes_group_sums(g)) HIP_TRY(launch_group_sums(g, d_slice_len, d_group_off, s));
    HIP_TRY(launch_scan_groups(g, d_group_off, d_total, s));
    HIP_TRY(launch_pack_payload(g, k->d_scratch, d_slice_len, d_group_off, d_payload, payload_cap, d_status, s));
    return LLCOMP_MI_OK;
}

}  // namespace

namespace llcomp_mi {
// parks the codec's blocks behind the event of its last call (nothing waits here: whoever takes a block out of the cache
// waits for that event; the lanes have drained their private stream before they get here anyway)
void codec_release(llcomp_mi_codec* k) {
    if (!k) return;
    DeviceGuard guard(k->device);
    // The event travels with the blocks only while the codec's last call is still running.  Usually it has long finished:
    // then the blocks are parked without it (an event must not outlive the stream it was recorded on -- a lane's private
    // stream is destroyed right after this -- and a finished event has nothing left to say).  A query that fails (the
    // caller destroyed its stream, which drains it) counts as finished.
    if (k->done && k->done->ev && hipEventQuery(k->done->ev) != hipErrorNotReady) {
        (void)hipGetLastError();
        k->done.reset();
    }
    dev_free(k->d_sym_or_rec, k->done);
    dev_free(k->d_lane_order, k->done);
    dev_free(k->d_states, k->done);
    dev_free(k->d_scratch, k->done);
    dev_free(k->d_group_off, k->done);
    dev_free(k->d_total_tmp, k->done);
    dev_free(k->d_region_len, k->done);
    dev_free(k->d_region_off, k->done);
    dev_free(k->d_regions, k->done);
    dev_free(k->d_stage, k->done);
    dev_free(k->d_box, k->done);
    dev_free(k->d_mid, k->done);
    dev_free(k->d_photo, k->done);
    dev_free(k->d_photo_tab, k->done);
    dev_free(k->d_mix_tab, k->done);
    dev_free(k->d_mix, k->done);
    dev_free(k->d_orient_tab, k->done);
    dev_free(k->d_compose_tab, k->done);
    dev_free(k->d_paste_tab, k->done);
    dev_free(k->d_paste16_tab, k->done);
    dev_free(k->d_alpha_tab, k->done);
    dev_free(k->d_label16_tab, k->done);
    dev_free(k->d_target_tab, k->done);
    dev_free(k->d_upd_goff, k->done);
    for (uint32_t i = 0; i < llcomp_mi_codec::kRegionsRing; ++i) {
        if (!k->h_regions[i]) continue;
        // (a copy out of the slot may still be queued on a caller's stream: it must not read freed memory)
        if (k->regions_ev_live[i] && k->regions_ev[i] && hipEventQuery(k->regions_ev[i]) == hipErrorNotReady) (void)hipEventSynchronize(k->regions_ev[i]);
        (void)hipGetLastError();
        (void)host_free_pinned(k->h_regions[i]);
    }
    for (auto& ev : k->regions_ev) if (ev) (void)hipEventDestroy(ev);
    dev_free(k->d_snap_sorted, k->done);
    dev_free(k->d_snap_banks, k->done);
    dev_free(k->d_snap_res, k->done);
    dev_free(k->d_snap_ctx, k->done);
    dev_free(k->d_snap_io, k->done);
    dev_free(k->d_seg_state, k->done);
    // (the second stream's work of a call is joined into the caller's stream before the call's last kernels: behind k->done it is idle)
    if (k->ev_fork) (void)hipEventDestroy(k->ev_fork);
    for (auto& ev : k->ev_chunk) if (ev) (void)hipEventDestroy(ev);
    if (k->aux && !k->aux_shared) (void)hipStreamDestroy(k->aux);
    dev_free(k->d_counters, k->done);
    if (k->h_feedback) {
        // the 16-byte feedback copy of the last cached decode may still be queued on the caller's stream: it must not land in freed
        // memory.  Its own event says when it has arrived (usually long ago); only a codec destroyed right behind such a call waits.
        if (k->fb_pending && k->fb_event && hipEventQuery(k->fb_event) == hipErrorNotReady) (void)hipEventSynchronize(k->fb_event);
        (void)hipGetLastError();
        (void)host_free_pinned(k->h_feedback);
    }
    if (k->fb_event) (void)hipEventDestroy(k->fb_event);
    for (auto& sp : k->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    delete k;
}
}  // namespace llcomp_mi

extern "C" {

int llcomp_mi_abi_version(void) { return LLCOMP_MI_ABI_VERSION; }

void llcomp_mi_reload_tuning(void) {
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    g_tuning = tuning_from_env();
    g_tuning_loaded = true;
}

int llcomp_mi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n < 0 ? 0 : n;
}

const char* llcomp_mi_strerror(int status) {
    switch (status) {
        case LLCOMP_MI_OK: return "ok";
        case LLCOMP_MI_BAD_MAGIC: return "Invalid magic number";  // llcomp.hpp:466, verbatim
        case LLCOMP_MI_BAD_EXPONENT: return "Invalid exponent";   // llcomp.hpp:233, verbatim
        case LLCOMP_MI_TRUNCATED: return "stream shorter than its header or slice table";
        case LLCOMP_MI_BAD_ARGS: return "bad arguments";
        case LLCOMP_MI_OUT_OF_RANGE: return "image dimensions out of range for this format";
        case LLCOMP_MI_OUTPUT_OVERFLOW: return "output capacity too small";
        case LLCOMP_MI_HIP_ERROR: return "HIP runtime error";
        case LLCOMP_MI_NO_DEVICE: return "no HIP device (this library has no CPU path)";
        case LLCOMP_MI_NOMEM: return "out of memory";
        case LLCOMP_MI_BUSY: return "all pipeline slots are in flight (take a finished job first)";
        case LLCOMP_MI_DEVICE_FAILED: return "a device of the device list failed (llcomp_mi_last_device_error tells which); nothing was published";
        default: return "unknown status";
    }
}

void llcomp_mi_free(void* p) { std::free(p); }

// ---- device-resident codec ------------------------------------------------------------------------------------
int llcomp_mi_codec_create(llcomp_mi_codec** out, int32_t device, uint32_t frames, uint32_t w, uint32_t h, uint32_t c,
                           uint32_t tile_w, uint32_t tile_h, uint32_t planar) {
    return llcomp_mi_codec_create_ex(out, device, frames, w, h, c, tile_w, tile_h, planar, 0);
}

int llcomp_mi_codec_create_ex(llcomp_mi_codec** out, int32_t device, uint32_t frames, uint32_t w, uint32_t h, uint32_t c,
                              uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t flags) {
    return llcomp_mi::codec_create(out, device, frames, w, h, c, tile_w, tile_h, planar, flags, 0);
}

}  // extern "C"

int llcomp_mi::codec_create(llcomp_mi_codec** out, int32_t device, uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w,
                            uint32_t tile_h, uint32_t planar, uint32_t flags, uint64_t legacy_stream) {
    if (!out || (flags & ~LLCOMP_MI_FLAG_SMALL_MODEL)) return LLCOMP_MI_BAD_ARGS;
    *out = nullptr;
    if (!frames) return LLCOMP_MI_BAD_ARGS;
    if (int rc = check_shape(w, h, c, false)) return rc;
    Geometry g;
    // kernel family and lane-group width are fixed here, for the life of the codec object
    if (!make_geometry(g, frames, w, h, c, tile_w, tile_h, planar, current_tuning(), (flags & LLCOMP_MI_FLAG_SMALL_MODEL) != 0))
        return LLCOMP_MI_OUT_OF_RANGE;
    if (legacy_stream) fit_legacy_stream(g, legacy_stream);
    int dev = 0;
    if (int rc = resolve_device(device, &dev)) return rc;
    DeviceGuard guard(dev);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    llcomp_mi_codec* k = new (std::nothrow) llcomp_mi_codec;
    if (!k) return LLCOMP_MI_NOMEM;
    k->g = g;
    k->tune = current_tuning();
    k->device = dev;
    k->feedback = !current_tuning().nofeedback;
    k->overlap = current_tuning().overlap != 0;
    k->aux_shared = current_tuning().overlap == 2;
    const uint64_t samples = uint64_t(frames) * w * h * c;
    k->need_states = slices_need_state_tables(g);
    // the fused row path (planar 1-row slices) has no image-order intermediate and 16-bit lane-order arrays in both directions
    const bool fused = model_is_fused(g);
    const uint64_t b_sym = fused ? 8 : samples * 4, b_states = k->need_states ? (uint64_t(lane_groups(g)) * kContexts << g.lane_shift) * 8 : 8,
                   b_scratch = (uint64_t(lane_groups(g)) << g.lane_shift) * g.slice_cap, b_off = (uint64_t(lane_groups(g)) + 1) * 8;
    // the 2-D encoder's snapshot pass: sorted entries (u32, they take the place of the lane-order symbols), banks in sorted and
    // in stream order (u64 each), residuals (i16) -- piece layout, snapshot.hpp
    const bool snap = snapshot_mode(g);
    const uint64_t snap_el = snap ? snapshot_elems(g) : 0;
    const uint64_t b_lanes = std::max((uint64_t(lane_groups(g)) * slice_capacity_samples(g) << g.lane_shift) * (fused ? 2 : 4), snap_el * 4);
    // What the codec can hold at most.  The state tables (decode, and encode without the snapshot pass) and the snapshot arrays
    // (encode) are allocated by the first call that needs them: a codec that only ever encodes, or only ever decodes, 64x64 tiles
    // holds 8.8 GB resp. 6.2 GB less per 16 frames of 4K than this figure.
    // ... plus the two arrays of a region decode (12 B per slice), and the state tables a region's sub-geometry may need where the codec's
    // own family keeps its states on chip (region_may_need_states)
    const uint64_t b_region = uint64_t(g.n_slices) * 12 +
                              (!k->need_states && !rows_mode(g) ? (uint64_t(lane_groups(g)) * kContexts << g.lane_shift) * 8 : 0);
    // ... plus the per-frame table of a regions decode, and the staging buffer of a host-staged one (its upper bound)
    const uint64_t b_regions = uint64_t(frames) * sizeof(RegionsFrame) + stage_bound(g);
    // ... plus the boxes and the horizontal pass's rows of a resized regions decode (frames * w * h * c each) and what its tables add to
    // the staging buffer (resized_tables_bound), for outputs no larger than the image
    const uint64_t b_resized = 2 * samples + resized_tables_bound(g);
    // ... plus a region update's two offset arrays, and the snapshot arrays + parking records of a box whose sub-geometry runs the pass
    // where the codec's family does not (region_snapshot_bound; the decoded box is the resized path's)
    const uint64_t b_update = (uint64_t(g.n_slices) + 1 + lane_groups(g) + 1) * 8 +
                              (snap ? 0 : region_snapshot_bound(g) ? region_snapshot_bound(g) * 28 + uint64_t(g.n_slices) * 64 : 0);
    // (snapshot_chunked: the five arrays and the coder's parking records, 64 bytes per slice)
    const uint64_t b_snap = snap_el * (snapshot_chunked(g) ? 28 : 18) + (snap && snapshot_chunked(g) ? uint64_t(g.n_slices) * 64 : 0);
    k->workspace_bytes = b_sym + b_lanes + b_states + b_scratch + b_off + 8 + b_snap + b_region + b_regions + b_resized + b_update;
    const bool ok = dev_alloc(&k->d_sym_or_rec, b_sym) == hipSuccess && dev_alloc(&k->d_lane_order, b_lanes) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&k->d_scratch), b_scratch) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&k->d_group_off), b_off) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&k->d_total_tmp), 8) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&k->d_counters), kCtrCount * 8) == hipSuccess &&
                    hipMemset(k->d_counters, 0, kCtrCount * 8) == hipSuccess;
    if (!ok) {
        llcomp_mi_codec_destroy(k);
        return LLCOMP_MI_NOMEM;
    }
    k->allocated_bytes = b_sym + b_lanes + b_scratch + b_off + 8;
    *out = k;
    return LLCOMP_MI_OK;
}

extern "C" {

void llcomp_mi_codec_destroy(llcomp_mi_codec* k) {
    // No device-wide wait: the blocks go back to the library's cache (devmem.hip) together with the event recorded behind
    // the codec's last encode / decode, and are handed out again only after it.  Profiling events that were never read
    // are destroyed by codec_release (hipEventDestroy of a pending event is legal: it is released when it completes).
    llcomp_mi::codec_release(k);
}

int llcomp_mi_codec_prepare(llcomp_mi_codec* k, uint32_t what) {
    if (!k || (what & ~(LLCOMP_MI_PREPARE_ENCODE | LLCOMP_MI_PREPARE_DECODE | LLCOMP_MI_PREPARE_REGION | LLCOMP_MI_PREPARE_REGIONS |
                        LLCOMP_MI_PREPARE_RESIZED | LLCOMP_MI_PREPARE_UPDATE | LLCOMP_MI_PREPARE_VIEWS)))
        return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (what & LLCOMP_MI_PREPARE_ENCODE) {
        if (snapshot_mode(k->g)) {
            if (int rc = ensure_snapshot_arrays(k, k->g)) return rc;
        }
        if (!snapshot_mode(k->g) || snapshot_chunked(k->g))
            if (int rc = ensure_state_tables(k, k->need_states)) return rc;
    }
    if (what & LLCOMP_MI_PREPARE_DECODE)
        if (int rc = ensure_state_tables(k, k->need_states)) return rc;
    if (what & (LLCOMP_MI_PREPARE_REGION | LLCOMP_MI_PREPARE_REGIONS | LLCOMP_MI_PREPARE_RESIZED | LLCOMP_MI_PREPARE_UPDATE |
                LLCOMP_MI_PREPARE_VIEWS)) {
        if (int rc = ensure_region_arrays(k)) return rc;
        if (region_may_need_states(k))
            if (int rc = ensure_state_tables(k, true)) return rc;
    }
    if (what & LLCOMP_MI_PREPARE_REGIONS)
        if (int rc = ensure_regions_table(k)) return rc;
    if (what & LLCOMP_MI_PREPARE_UPDATE) {  // (the encoder's own arrays: LLCOMP_MI_PREPARE_ENCODE)
        const uint64_t samples = uint64_t(k->g.frames) * k->g.w * k->g.h * k->g.c;
        if (int rc = ensure_update_arrays(k)) return rc;
        if (int rc = ensure_grown(k, k->d_box, k->box_cap, samples, samples)) return rc;
    }
    if (what & (LLCOMP_MI_PREPARE_RESIZED | LLCOMP_MI_PREPARE_VIEWS)) {
        const uint64_t samples = uint64_t(k->g.frames) * k->g.w * k->g.h * k->g.c;
        if (int rc = ensure_regions_ring(k)) return rc;
        if (int rc = ensure_grown(k, k->d_box, k->box_cap, samples, samples)) return rc;
        if (int rc = ensure_grown(k, k->d_mid, k->mid_cap, samples, samples)) return rc;
    }
    if (what & LLCOMP_MI_PREPARE_VIEWS) {  // (the regions table of every frame and the tables of `frames` views: a call from HBM)
        const uint64_t tables = ((uint64_t(k->g.frames) * sizeof(RegionsFrame) + 15) & ~15ull) + resized_tables_bound(k->g);
        if (int rc = ensure_stage(k, tables, stage_bound(k->g) + resized_tables_bound(k->g))) return rc;
    }
    return LLCOMP_MI_OK;
}

uint32_t llcomp_mi_codec_slices(const llcomp_mi_codec* k) { return k ? k->g.n_slices : 0; }
uint32_t llcomp_mi_codec_kernel_family(const llcomp_mi_codec* k) { return k ? (k->g.flags & 0xFFu) | (k->g.lane_shift << 8) | (k->g.lpw << 16) : 0; }
uint64_t llcomp_mi_codec_workspace_bytes(const llcomp_mi_codec* k) { return k ? k->workspace_bytes : 0; }
uint64_t llcomp_mi_codec_allocated_bytes(const llcomp_mi_codec* k) { return k ? k->allocated_bytes : 0; }
uint64_t llcomp_mi_codec_max_payload_bytes(const llcomp_mi_codec* k) {
    return k ? uint64_t(k->g.n_slices) * k->g.slice_cap : 0;
}

int llcomp_mi_codec_model(llcomp_mi_codec* k, const void* d_px, void* d_sym, void* stream) {
    if (!k || !d_px || !d_sym || misaligned(d_sym, 4)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    HIP_TRY(launch_model_fwd(k->g, static_cast<const uint8_t*>(d_px), static_cast<uint32_t*>(d_sym),
                             static_cast<hipStream_t>(stream)));
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_encode(llcomp_mi_codec* k, const void* d_px, void* d_payload, uint64_t payload_cap, void* d_slice_len,
                           void* d_total, void* d_status, void* stream) {
    if (!k || !d_px || !d_payload || !d_slice_len || !d_total || !d_status) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_slice_len, 4) || misaligned(d_total, 8) || misaligned(d_status, 4)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (int rc = ensure_encode(k, k->g)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    if (int rc = encode_streams(k, k->g, d_px, static_cast<uint32_t*>(d_slice_len), k->d_group_off, static_cast<uint32_t*>(d_status), s)) return rc;
    if (int rc = pack_streams(k, k->g, static_cast<const uint32_t*>(d_slice_len), k->d_group_off, static_cast<uint8_t*>(d_payload), payload_cap,
                              static_cast<uint64_t*>(d_total), static_cast<uint32_t*>(d_status), s))
        return rc;
    ++k->n_encode;
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_decode(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                           void* d_px, void* d_status, void* stream) {
    if (!k || !d_payload || !d_slice_len || !d_px || !d_status) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_slice_len, 4) || misaligned(d_status, 4)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Geometry& g = k->g;
    if (int rc = ensure_decode(k, g)) return rc;
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    const int rc = decode_chain(
        k, g, static_cast<const uint32_t*>(d_slice_len), static_cast<uint32_t*>(d_status), s,
        [&]() -> int {
            HIP_TRY(launch_group_sums(g, static_cast<const uint32_t*>(d_slice_len), k->d_group_off, s));
            HIP_TRY(launch_scan_groups(g, k->d_group_off, k->d_total_tmp, s));
            HIP_TRY(launch_stage_streams(g, static_cast<const uint8_t*>(d_payload), payload_bytes, static_cast<const uint32_t*>(d_slice_len),
                                         k->d_group_off, k->d_scratch, static_cast<uint32_t*>(d_status), s));
            return LLCOMP_MI_OK;
        },
        [&](bool fused, const int16_t* v) -> int {
            HIP_TRY(fused ? launch_model_rows_inv(g, v, static_cast<uint8_t*>(d_px), s) : launch_model_inv(g, v, static_cast<uint8_t*>(d_px), s));
            return LLCOMP_MI_OK;
        });
    if (rc) return rc;
    ++k->n_decode;
    return LLCOMP_MI_OK;
}

uint32_t llcomp_mi_codec_region_family(const llcomp_mi_codec* k, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh) {
    RegionBox box;
    Geometry sub;
    if (!k || region_setup(k, x, y, rw, rh, box, sub)) return 0;
    return (sub.flags & 0xFFu) | (sub.lane_shift << 8) | (sub.lpw << 16);
}

// Region decode (DESIGN.md "Region decode"): the full geometry's group offsets locate the covered slices in the full payload, and the
// decoder runs on the covered sub-image's geometry in the codec's own workspace.  Same verdicts as a full decode, from the covered
// slices only.
int llcomp_mi_codec_decode_region(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                                  uint32_t y, uint32_t rw, uint32_t rh, void* d_px, void* d_status, void* stream) {
    if (!k || !d_payload || !d_slice_len || !d_px || !d_status) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_slice_len, 4) || misaligned(d_status, 4)) return LLCOMP_MI_BAD_ARGS;
    RegionBox box;
    Geometry sub;
    if (int rc = region_setup(k, x, y, rw, rh, box, sub)) return rc;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (int rc = ensure_region_arrays(k)) return rc;
    if (int rc = ensure_decode(k, sub)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Geometry& g = k->g;
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    const int rc = decode_chain(
        k, sub, k->d_region_len, static_cast<uint32_t*>(d_status), s,
        [&]() -> int { return locate_box(k, sub, box, d_payload, payload_bytes, d_slice_len, static_cast<uint32_t*>(d_status), s); },
        [&](bool fused, const int16_t* v) -> int {
            const Crop cr{x - box.tx0 * g.tile_w, y - box.ty0 * g.tile_h, rw, rh};
            HIP_TRY(fused ? launch_model_rows_inv_crop(sub, v, static_cast<uint8_t*>(d_px), cr, s)
                          : launch_model_inv_crop(sub, v, static_cast<uint8_t*>(d_px), cr, s));
            return LLCOMP_MI_OK;
        });
    if (rc) return rc;
    ++k->n_decode;
    return LLCOMP_MI_OK;
}

}  // extern "C"

namespace {
// A region update's plan: the covered box, its sub-geometry, and whether the rectangle is exactly the box's pixels.  BAD_ARGS for a
// rectangle the frame does not hold; HIP_ERROR if the sub-geometry's arrays would not fit the codec's workspace (region_encode_fits:
// never by default, checked all the same) -- both before anything is launched.
struct UpdatePlan {
    RegionBox box;
    Geometry sub;
    bool whole;
};
int update_setup(const llcomp_mi_codec* k, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, UpdatePlan& p) {
    if (int rc = region_setup(k, x, y, rw, rh, p.box, p.sub)) return rc;
    if (!region_encode_fits(k->g, p.sub)) return LLCOMP_MI_HIP_ERROR;
    p.whole = region_is_whole_box(k->g, p.sub, p.box, x, y, rw, rh);
    return LLCOMP_MI_OK;
}
// The box's new pixels, [frames][sub.h][sub.w][c]: the caller's rectangle itself when it is the whole box; else the box is decoded from
// the old batch into the codec's box buffer (llcomp_mi_codec_decode_region's chain up to the inverse model on the sub-geometry, written
// whole: no crop) and the rectangle is pasted over it.  Leaves the old table's group offsets of the FULL geometry in d_group_off.
int update_box_pixels(llcomp_mi_codec* k, const UpdatePlan& p, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                      uint32_t y, uint32_t rw, uint32_t rh, const void* d_rect, uint32_t* d_status, hipStream_t s, const void** d_box_px) {
    const Geometry& g = k->g;
    const Geometry& sub = p.sub;
    if (p.whole) {
        *d_box_px = d_rect;
        return LLCOMP_MI_OK;
    }
    const int rc = decode_chain(
        k, sub, k->d_region_len, d_status, s,
        [&]() -> int { return locate_box(k, sub, p.box, d_payload, payload_bytes, d_slice_len, d_status, s); },
        [&](bool fused, const int16_t* v) -> int {
            HIP_TRY(fused ? launch_model_rows_inv(sub, v, k->d_box, s) : launch_model_inv(sub, v, k->d_box, s));
            HIP_TRY(launch_paste_rect(static_cast<const uint8_t*>(d_rect), k->d_box, sub.frames, sub.c, rw, rh, sub.w, sub.h, x - p.box.tx0 * g.tile_w,
                                      y - p.box.ty0 * g.tile_h, s));
            return LLCOMP_MI_OK;
        });
    if (rc) return rc;
    ++k->n_decode;
    *d_box_px = k->d_box;
    return LLCOMP_MI_OK;
}
// what both calls allocate before they queue anything
int update_ensure(llcomp_mi_codec* k, const UpdatePlan& p) {
    if (int rc = ensure_region_arrays(k)) return rc;
    if (int rc = ensure_update_arrays(k)) return rc;
    if (int rc = ensure_encode(k, p.sub)) return rc;
    if (p.whole) return LLCOMP_MI_OK;
    if (int rc = ensure_decode(k, p.sub)) return rc;
    const uint64_t samples = uint64_t(k->g.frames) * k->g.w * k->g.h * k->g.c;
    return ensure_grown(k, k->d_box, k->box_cap, uint64_t(p.sub.frames) * p.sub.w * p.sub.h * p.sub.c, samples);
}
}  // namespace

extern "C" {

// Region update (DESIGN.md "Region update"): the covered box's new pixels (update_box_pixels) through the encoder on the box's
// sub-geometry (encode_streams), then either packed as they are (encode_region) or spliced into the full batch in HBM (update_region).
int llcomp_mi_codec_encode_region(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                                  uint32_t y, uint32_t rw, uint32_t rh, const void* d_rect, void* d_sub_payload, uint64_t sub_payload_cap,
                                  void* d_sub_len, void* d_sub_total, void* d_status, void* stream) {
    if (!k || !d_rect || !d_sub_payload || !d_sub_len || !d_sub_total || !d_status) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_slice_len, 4) || misaligned(d_sub_len, 4) || misaligned(d_sub_total, 8) || misaligned(d_status, 4)) return LLCOMP_MI_BAD_ARGS;
    UpdatePlan p;
    if (int rc = update_setup(k, x, y, rw, rh, p)) return rc;
    if (!p.whole && (!d_payload || !d_slice_len)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (int rc = update_ensure(k, p)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DoneGuard done_guard{k, s};
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    const void* px = nullptr;
    if (int rc = update_box_pixels(k, p, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_rect, static_cast<uint32_t*>(d_status), s, &px))
        return rc;
    if (int rc = encode_streams(k, p.sub, px, static_cast<uint32_t*>(d_sub_len), k->d_upd_goff, static_cast<uint32_t*>(d_status), s)) return rc;
    if (int rc = pack_streams(k, p.sub, static_cast<const uint32_t*>(d_sub_len), k->d_upd_goff, static_cast<uint8_t*>(d_sub_payload),
                              sub_payload_cap, static_cast<uint64_t*>(d_sub_total), static_cast<uint32_t*>(d_status), s))
        return rc;
    ++k->n_encode;
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_update_region(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                                  uint32_t y, uint32_t rw, uint32_t rh, const void* d_rect, void* d_payload_out, uint64_t payload_cap,
                                  void* d_slice_len_out, void* d_total, void* d_status, void* stream) {
    if (!k || !d_rect || !d_payload_out || !d_slice_len_out || !d_total || !d_status) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_slice_len, 4) || misaligned(d_slice_len_out, 4) || misaligned(d_total, 8) || misaligned(d_status, 4)) return LLCOMP_MI_BAD_ARGS;
    UpdatePlan p;
    if (int rc = update_setup(k, x, y, rw, rh, p)) return rc;
    const Geometry& g = k->g;
    const bool all = p.sub.n_slices == g.n_slices;  // every slice is covered: nothing of the old batch is carried over
    if (!(p.whole && all) && (!d_payload || !d_slice_len)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    if (int rc = update_ensure(k, p)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DoneGuard done_guard{k, s};
    uint32_t* const status = static_cast<uint32_t*>(d_status);
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    const void* px = nullptr;
    if (int rc = update_box_pixels(k, p, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_rect, status, s, &px)) return rc;
    // the covered slices' new lengths go where the decoder's copy of the old ones was (it is done with them: same stream)
    if (int rc = encode_streams(k, p.sub, px, k->d_region_len, k->d_upd_goff, status, s)) return rc;
    {
        Timed t(k, s, 3);
        uint64_t* const new_goff = k->d_upd_goff + g.n_slices + 1;
        if (p.whole && !all) {  // (the decode of an unaligned rectangle has left the old table's offsets in d_group_off)
            HIP_TRY(launch_group_sums(g, static_cast<const uint32_t*>(d_slice_len), k->d_group_off, s));
            HIP_TRY(launch_scan_groups(g, k->d_group_off, k->d_total_tmp, s));
        }
        HIP_TRY(launch_merge_table(g, p.sub, p.box, static_cast<const uint32_t*>(d_slice_len), k->d_region_len, static_cast<uint32_t*>(d_slice_len_out), s));
        HIP_TRY(launch_group_sums(g, static_cast<const uint32_t*>(d_slice_len_out), new_goff, s));
        HIP_TRY(launch_scan_groups(g, new_goff, static_cast<uint64_t*>(d_total), s));
        HIP_TRY(launch_splice_slices(g, p.sub, p.box, static_cast<const uint8_t*>(d_payload), payload_bytes, static_cast<const uint32_t*>(d_slice_len),
                                     k->d_group_off, k->d_scratch, static_cast<const uint32_t*>(d_slice_len_out), new_goff,
                                     static_cast<uint8_t*>(d_payload_out), payload_cap, status, s));
    }
    ++k->n_encode;
    return LLCOMP_MI_OK;
}

}  // extern "C"

extern "C" {

uint32_t llcomp_mi_codec_regions_family(const llcomp_mi_codec* k, const uint32_t* xy, uint32_t rw, uint32_t rh, uint32_t* fam, uint32_t cap) {
    if (!k || (cap && !fam)) return 0;
    WindowsPlan p;
    if (regions_plan(k, xy, rw, rh, p)) return 0;
    for (uint32_t i = 0; i < p.n_classes && i < cap; ++i) {
        const Geometry& sub = p.classes[i].sub;
        fam[i] = (sub.flags & 0xFFu) | (sub.lane_shift << 8) | (sub.lpw << 16);
    }
    return p.n_classes;
}

}  // extern "C"

namespace {

// The windowed decodes (DESIGN.md "Region decode"; "Crops of different sizes, resized to one shape"; "Several views of each frame"): one
// body per family, behind the entry points below, from either kind of source.  Each refuses its pointers (source_ok), builds its plan
// (windows_plan.hpp) -- for host containers also the gather over the plan's windows (host_gather) -- and hands both to decode_windows;
// every refusal comes before anything is queued or grown.

// Regions decode: the region decode, class by class (geometry.hpp: regions_window), in order on the caller's stream.  Of host
// containers only the window slices' bytes cross to the GPU -- and this call alone plans its gather AHEAD of its windows: an input
// that is wrong in both ways keeps the gather's status.
int regions_call(llcomp_mi_codec* k, WindowsSource src, const uint32_t* xy, uint32_t rw, uint32_t rh, void* d_px, void* d_status, void* stream) {
    if (!source_ok(k, src, d_status) || !d_px || !xy) return LLCOMP_MI_BAD_ARGS;
    if (src.host) {
        if (int rc = regions_gather_plan(src.data, src.lens, k->g.frames, xy, rw, rh, src.gather)) return rc;
        if (int rc = same_shape(k->g, src.gather.g)) return rc;
    }
    WindowsPlan p;
    if (int rc = regions_plan(k, xy, rw, rh, p)) return rc;
    if (int rc = gather_matches(p, src)) return rc;
    return decode_windows(k, WindowsCall{p, {}, nullptr, 0, src, d_px}, d_status, stream);
}

// Resized regions decode: the classes crop every frame's box (the batch's largest rectangle size) into d_box; then the two resample passes
// read every frame's rectangle from its box and write d_px, the vertical pass through the output format's table where there is one.
// padded (rects are int32 then, and may leave the image): the plan on the SOURCE rectangles (windows_plan.hpp: padded_setup), driven as
// it is.  The gather of a host source has every window sized for the largest rectangle -- a padded call's over the source rectangles.
int resized_call(llcomp_mi_codec* k, WindowsSource src, const void* rects, const uint8_t* flags, uint32_t ow, uint32_t oh, bool padded,
                 const llcomp_mi_pad* pad, const llcomp_mi_output_format* fmt, void* d_px, void* d_status, void* stream) {
    if (!source_ok(k, src, d_status) || !d_px || !rects) return LLCOMP_MI_BAD_ARGS;
    ResizedPlan p;
    std::vector<uint32_t> from;  // a padded call's source rectangles
    if (int rc = padded ? padded_setup(k->g, k->tune, static_cast<const int32_t*>(rects), flags, ow, oh, pad, fmt, d_px, p, from)
                        : resized_setup(k->g, k->tune, static_cast<const uint32_t*>(rects), flags, ow, oh, fmt, d_px, p))
        return rc;
    if (int rc = host_gather(k, src, p, padded ? from.data() : static_cast<const uint32_t*>(rects), nullptr)) return rc;
    const uint64_t bound = padded ? padded_tables_bound(k->g, k->g.frames) : resized_tables_bound(k->g);
    return decode_windows(k, WindowsCall{p, p.tail, nullptr, bound, src, nullptr}, d_status, stream);
}

// The chains beside a tail's groups (photo_plan.hpp: photo_setup; photo: one entry per group, or null for a call without chains, which
// leaves pt.any() false and the groups as they are).  A group with a chain hands its output -- format, table and d_out -- over to the
// chain's last step and becomes a plain U8 HWC group whose output is the staging buffer (windows_groups puts the address in).
template <class Group>
int photo_tail_of(const Geometry& g, std::vector<Group>& groups, const llcomp_mi_photo_group* photo, PhotoTail& pt) {
    std::vector<uint32_t> n, ow, oh;
    for (const Group& gr : groups) {
        n.push_back(gr.n);
        ow.push_back(gr.ow);
        oh.push_back(gr.oh);
    }
    if (int rc = photo_setup(g.c, uint64_t(g.frames) * g.w * g.h * g.c, photo, uint32_t(groups.size()), n.data(), ow.data(), oh.data(), pt)) return rc;
    for (size_t i = 0; i < groups.size(); ++i) {
        PhotoGroup& pg = pt.groups[i];
        if (!pg.active) continue;
        pg.out = groups[i].out;
        pg.d_out = groups[i].d_out;
        pg.table_at = groups[i].table_at;
        groups[i].out = OutFormat{};
        groups[i].d_out = nullptr;
        groups[i].table_at = 0;
    }
    return LLCOMP_MI_OK;
}

// Views decode: the resized regions decode on the used frames' union rectangles up to the boxes -- the classes unchanged, over the frame
// list -- then every group's views resampled from their frames' boxes.  padded: padded_views_setup, as in resized_call.  The gather of a
// host source runs over the used frames' union rectangles (a frame without a view is not looked at: its container may be NULL).
int views_call(llcomp_mi_codec* k, WindowsSource src, const llcomp_mi_view_group* groups, uint32_t n_groups, bool padded, const llcomp_mi_pad* pad,
               const llcomp_mi_photo_group* photo, void* d_status, void* stream) {
    if (!source_ok(k, src, d_status)) return LLCOMP_MI_BAD_ARGS;
    ViewsPlan p;
    if (int rc = padded ? padded_views_setup(k->g, k->tune, groups, n_groups, pad, p) : views_setup(k->g, k->tune, groups, n_groups, p)) return rc;
    PhotoTail pt;
    if (int rc = photo_tail_of(k->g, p.tail.groups, photo, pt)) return rc;
    if (int rc = host_gather(k, src, p, p.u.rects.data(), &p.u.used)) return rc;
    const uint64_t bound = (padded ? padded_tables_bound(k->g, p.u.total_views) : views_tables_bound(k->g, p.u.total_views)) +
                           (pt.any() ? photo_tables_bound(p.u.total_views) : 0);
    return decode_windows(k, WindowsCall{p, p.tail, pt.any() ? &pt : nullptr, bound, src, nullptr}, d_status, stream);
}

// Warped views: the views decode on the views' SOURCE rectangles up to the boxes (warp_plan.hpp: warp_setup -- views_union and
// regions_setup_sized, unchanged), then the warp tail: one gather launch per group reads every view from its frame's box.  With no
// used frame (every view all fill) nothing is read.
// Perspective groups (llcomp_mi_perspective_group) take the same body: persp_setup stages PerspEntry in the tail, and windows_warp
// launches the perspective gather for them.
int warped_setup(const llcomp_mi_codec* k, const llcomp_mi_warp_group* groups, uint32_t n_groups, WarpPlan& p) {
    return warp_setup(k->g, k->tune, groups, n_groups, p);
}
int warped_setup(const llcomp_mi_codec* k, const llcomp_mi_perspective_group* groups, uint32_t n_groups, WarpPlan& p) {
    return persp_setup(k->g, k->tune, groups, n_groups, p);
}
template <class Group>
int warped_call(llcomp_mi_codec* k, WindowsSource src, const Group* groups, uint32_t n_groups, const llcomp_mi_photo_group* photo, void* d_status,
                void* stream) {
    if (!source_ok(k, src, d_status)) return LLCOMP_MI_BAD_ARGS;
    WarpPlan p;
    if (int rc = warped_setup(k, groups, n_groups, p)) return rc;
    PhotoTail pt;
    if (int rc = photo_tail_of(k->g, p.tail.groups, photo, pt)) return rc;
    if (int rc = host_gather(k, src, p, p.u.rects.data(), &p.u.used)) return rc;
    const uint64_t tables = p.tail.ps.empty() ? warp_tables_bound(k->g, p.total_views) : persp_tables_bound(k->g, p.total_views);
    const uint64_t bound = tables + (pt.any() ? photo_tables_bound(p.total_views) : 0);
    return decode_windows(k, WindowsCall{p, p.tail, pt.any() ? &pt : nullptr, bound, src, nullptr}, d_status, stream);
}

}  // namespace

extern "C" {

int llcomp_mi_codec_decode_regions(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                   const uint32_t* xy, uint32_t rw, uint32_t rh, void* d_px, void* d_status, void* stream) {
    return regions_call(k, device_source(d_payload, payload_bytes, d_slice_len), xy, rw, rh, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_regions_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens, const uint32_t* xy, uint32_t rw,
                                        uint32_t rh, void* d_px, void* d_status, void* stream) {
    return regions_call(k, host_source(data, lens), xy, rw, rh, d_px, d_status, stream);
}

int llcomp_mi_codec_decode_resized_regions_ex(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                              const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                                              const llcomp_mi_output_format* fmt, void* d_px, void* d_status, void* stream) {
    return resized_call(k, device_source(d_payload, payload_bytes, d_slice_len), rects, flags, ow, oh, false, nullptr, fmt, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_resized_regions_host_ex(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens, const uint32_t* rects,
                                                   const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_output_format* fmt,
                                                   void* d_px, void* d_status, void* stream) {
    return resized_call(k, host_source(data, lens), rects, flags, ow, oh, false, nullptr, fmt, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_resized_regions(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                           const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh, void* d_px, void* d_status,
                                           void* stream) {
    return resized_call(k, device_source(d_payload, payload_bytes, d_slice_len), rects, flags, ow, oh, false, nullptr, nullptr, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_resized_regions_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens, const uint32_t* rects,
                                                const uint8_t* flags, uint32_t ow, uint32_t oh, void* d_px, void* d_status, void* stream) {
    return resized_call(k, host_source(data, lens), rects, flags, ow, oh, false, nullptr, nullptr, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_padded_regions(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                          const int32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_pad* pad,
                                          const llcomp_mi_output_format* fmt, void* d_px, void* d_status, void* stream) {
    return resized_call(k, device_source(d_payload, payload_bytes, d_slice_len), rects, flags, ow, oh, true, pad, fmt, d_px, d_status, stream);
}
int llcomp_mi_codec_decode_padded_regions_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens, const int32_t* rects,
                                               const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_pad* pad,
                                               const llcomp_mi_output_format* fmt, void* d_px, void* d_status, void* stream) {
    return resized_call(k, host_source(data, lens), rects, flags, ow, oh, true, pad, fmt, d_px, d_status, stream);
}

int llcomp_mi_codec_decode_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                 const llcomp_mi_view_group* groups, uint32_t n_groups, void* d_status, void* stream) {
    return views_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, false, nullptr, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens, const llcomp_mi_view_group* groups,
                                      uint32_t n_groups, void* d_status, void* stream) {
    return views_call(k, host_source(data, lens), groups, n_groups, false, nullptr, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_padded_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                        const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad, void* d_status,
                                        void* stream) {
    return views_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, true, pad, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_padded_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                             const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad, void* d_status,
                                             void* stream) {
    return views_call(k, host_source(data, lens), groups, n_groups, true, pad, nullptr, d_status, stream);
}
// (the photometric calls: a NULL pad is the unpadded call)
int llcomp_mi_codec_decode_photo_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                       const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                                       const llcomp_mi_photo_group* photo, void* d_status, void* stream) {
    return views_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, pad != nullptr, pad, photo, d_status, stream);
}
int llcomp_mi_codec_decode_photo_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                            const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                                            const llcomp_mi_photo_group* photo, void* d_status, void* stream) {
    return views_call(k, host_source(data, lens), groups, n_groups, pad != nullptr, pad, photo, d_status, stream);
}

int llcomp_mi_codec_decode_warped_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                        const llcomp_mi_warp_group* groups, uint32_t n_groups, void* d_status, void* stream) {
    return warped_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_warped_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                             const llcomp_mi_warp_group* groups, uint32_t n_groups, void* d_status, void* stream) {
    return warped_call(k, host_source(data, lens), groups, n_groups, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_photo_warped_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                              const llcomp_mi_warp_group* groups, uint32_t n_groups, const llcomp_mi_photo_group* photo,
                                              void* d_status, void* stream) {
    return warped_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, photo, d_status, stream);
}
int llcomp_mi_codec_decode_photo_warped_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                                   const llcomp_mi_warp_group* groups, uint32_t n_groups, const llcomp_mi_photo_group* photo,
                                                   void* d_status, void* stream) {
    return warped_call(k, host_source(data, lens), groups, n_groups, photo, d_status, stream);
}

int llcomp_mi_codec_decode_perspective_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                             const llcomp_mi_perspective_group* groups, uint32_t n_groups, void* d_status, void* stream) {
    return warped_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_perspective_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                                  const llcomp_mi_perspective_group* groups, uint32_t n_groups, void* d_status, void* stream) {
    return warped_call(k, host_source(data, lens), groups, n_groups, nullptr, d_status, stream);
}
int llcomp_mi_codec_decode_photo_perspective_views(llcomp_mi_codec* k, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                                   const llcomp_mi_perspective_group* groups, uint32_t n_groups,
                                                   const llcomp_mi_photo_group* photo, void* d_status, void* stream) {
    return warped_call(k, device_source(d_payload, payload_bytes, d_slice_len), groups, n_groups, photo, d_status, stream);
}
int llcomp_mi_codec_decode_photo_perspective_views_host(llcomp_mi_codec* k, const uint8_t* const* data, const size_t* lens,
                                                        const llcomp_mi_perspective_group* groups, uint32_t n_groups,
                                                        const llcomp_mi_photo_group* photo, void* d_status, void* stream) {
    return warped_call(k, host_source(data, lens), groups, n_groups, photo, d_status, stream);
}
uint64_t llcomp_mi_codec_perspective_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    return k->workspace_bytes + persp_tables_bound(k->g, total_views);
}
uint64_t llcomp_mi_codec_photo_perspective_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    return llcomp_mi_codec_photo_workspace_bytes(k, total_views) + persp_tables_bound(k->g, total_views) - warp_tables_bound(k->g, total_views);
}

// The batch calls (DESIGN.md "Batch calls: what the three share"): every refusal first (the call's *_check_call), then the plan, then
// batch_table_call with the call's own table buffer, all on the caller's stream.
//
// Batch mixing (DESIGN.md "Batch mixing"): the heads of the segments of cut cycles go into d_mix (k_mix_save) ahead of k_mix.
int llcomp_mi_codec_mix_batch(llcomp_mi_codec* k, void* d_batch, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                              const llcomp_mi_mix_sample* samples, const float* erase_value, void* stream) {
    if (!k || !d_batch || !samples) return LLCOMP_MI_BAD_ARGS;
    const uint32_t c = k->g.c;
    std::vector<uint32_t> erase_bits;
    if (int rc = mix_check_call(n, c, ow, oh, dtype, layout, samples, erase_value, erase_bits)) return rc;
    if (misaligned(d_batch, batch_esize(dtype))) return LLCOMP_MI_BAD_ARGS;
    MixPlan p;
    mix_plan(n, samples, p);
    const uint64_t saved_bytes = p.n_saved * mix_slot_stride(uint64_t(c) * ow * oh * batch_esize(dtype));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_mix_tab, k->mix_tab_cap, MixTable(n, p.segs.size(), c).bytes, mix_table_bound(n, c), s,
        [&](uint8_t* at) { mix_table_put(n, samples, p, erase_bits, at); },
        [&](const uint8_t* d_table) {
            MixLaunch m{};
            m.d_batch = static_cast<uint8_t*>(d_batch), m.d_saved = saved_bytes ? k->d_mix : nullptr, m.d_table = d_table;
            m.n = n, m.c = c, m.ow = ow, m.oh = oh, m.dtype = dtype, m.layout = layout;
            m.n_segments = uint32_t(p.segs.size()), m.n_saved = p.n_saved;
            return launch_mix(m, s);
        },
        &k->d_mix, &k->mix_cap, saved_bytes);
}

uint64_t llcomp_mi_codec_mix_workspace_bytes(const llcomp_mi_codec* k, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype) {
    if (!k || !batch_esize(dtype)) return 0;
    return k->workspace_bytes + mix_table_bound(n, k->g.c) + mix_saved_bound(n) * mix_slot_stride(uint64_t(k->g.c) * ow * oh * batch_esize(dtype));
}

// Batch orientation (DESIGN.md "Batch orientation"): the table holds the oriented samples.  Codes that are all 0: nothing is queued.
int llcomp_mi_codec_orient_batch(llcomp_mi_codec* k, void* d_batch, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                 const uint8_t* codes, void* stream) {
    if (!k || !d_batch || !codes) return LLCOMP_MI_BAD_ARGS;
    const uint32_t c = k->g.c;
    if (int rc = orient_check_call(n, c, ow, oh, dtype, layout, codes)) return rc;
    if (misaligned(d_batch, batch_esize(dtype))) return LLCOMP_MI_BAD_ARGS;
    std::vector<OrientEntry> table;
    orient_table(n, codes, table);
    if (table.empty()) return LLCOMP_MI_OK;
    const uint64_t bytes = table.size() * sizeof(OrientEntry);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_orient_tab, k->orient_tab_cap, bytes, orient_table_bound(n), s, [&](uint8_t* at) { std::memcpy(at, table.data(), bytes); },
        [&](const uint8_t* d_table) {
            OrientLaunch o{};
            o.d_batch = static_cast<uint8_t*>(d_batch), o.d_table = d_table, o.n_entries = uint32_t(table.size());
            for (const OrientEntry& e : table) o.code_set |= 1u << e.code;
            o.c = c, o.ow = ow, o.oh = oh, o.dtype = dtype, o.layout = layout;
            return launch_orient(o, s);
        });
}

uint64_t llcomp_mi_codec_orient_workspace_bytes(const llcomp_mi_codec* k, uint32_t n) {
    if (!k) return 0;
    return k->workspace_bytes + orient_table_bound(n);
}

// Batch composition (DESIGN.md "Batch composition"): compose_check_memory refuses too.  Under KEEP a call without a piece of w and h
// above 0 queues nothing.
int llcomp_mi_codec_compose_batch(llcomp_mi_codec* k, const void* d_src, uint32_t n_src, uint32_t iw, uint32_t ih, void* d_dst, uint32_t n_dst,
                                  uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_compose_piece* pieces,
                                  uint32_t n_pieces, const float* fill_value, uint32_t flags, void* stream) {
    if (!k || !d_dst) return LLCOMP_MI_BAD_ARGS;
    const uint32_t c = k->g.c;
    std::vector<uint32_t> fill_bits;
    if (int rc = compose_check_call(n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, fill_value, flags, fill_bits)) return rc;
    const uint32_t esize = batch_esize(dtype);
    if (int rc = compose_check_memory(d_src, uint64_t(n_src) * c * iw * ih * esize, d_dst, uint64_t(n_dst) * c * ow * oh * esize, esize)) return rc;
    ComposePlan p;
    compose_plan(n_dst, pieces, n_pieces, flags, p);
    if (p.samples.empty()) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_compose_tab, k->compose_tab_cap, ComposeTable(p.samples.size(), p.order.size(), c).bytes, compose_table_bound(n_dst, n_pieces, c), s,
        [&](uint8_t* at) { compose_table_put(pieces, p, fill_bits, layout, at); },
        [&](const uint8_t* d_table) {
            ComposeLaunch o{};
            o.d_src = n_src ? static_cast<const uint8_t*>(d_src) : nullptr, o.d_dst = static_cast<uint8_t*>(d_dst), o.d_table = d_table;
            o.n_samples = uint32_t(p.samples.size()), o.n_recs = uint32_t(p.order.size());
            o.n_src = n_src, o.iw = iw, o.ih = ih, o.ow = ow, o.oh = oh, o.c = c, o.dtype = dtype, o.layout = layout;
            o.keep = flags & LLCOMP_MI_COMPOSE_KEEP;
            return launch_compose(o, s);
        });
}

uint64_t llcomp_mi_codec_compose_workspace_bytes(const llcomp_mi_codec* k, uint32_t n_dst, uint32_t n_pieces) {
    if (!k) return 0;
    return k->workspace_bytes + compose_table_bound(n_dst, n_pieces, k->g.c);
}

// Batch copy-paste (DESIGN.md "Batch copy-paste"): paste_batch_call with the 8-bit call's table buffer.
int llcomp_mi_codec_paste_batch(llcomp_mi_codec* k, const void* d_src, const void* d_mask, uint32_t n_src, uint32_t iw, uint32_t ih, void* d_dst,
                                uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece* pieces,
                                uint32_t n_pieces, void* stream) {
    if (!k) return LLCOMP_MI_BAD_ARGS;
    return paste_batch_call(k, k->d_paste_tab, k->paste_tab_cap, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, dtype, layout, pieces, n_pieces, stream);
}

uint64_t llcomp_mi_codec_paste_workspace_bytes(const llcomp_mi_codec* k, uint32_t n_dst, uint32_t n_pieces) {
    if (!k) return 0;
    return k->workspace_bytes + paste_table_bound<1>(n_dst, n_pieces);
}

// Batch copy-paste by 16-bit ids (DESIGN.md "Batch copy-paste by 16-bit ids"): the same with the 16-bit call's table buffer.
int llcomp_mi_codec_paste_batch16(llcomp_mi_codec* k, const void* d_src, const void* d_mask, uint32_t n_src, uint32_t iw, uint32_t ih, void* d_dst,
                                  uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces,
                                  uint32_t n_pieces, void* stream) {
    if (!k) return LLCOMP_MI_BAD_ARGS;
    return paste_batch_call(k, k->d_paste16_tab, k->paste16_tab_cap, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, dtype, layout, pieces, n_pieces, stream);
}

uint64_t llcomp_mi_codec_paste16_workspace_bytes(const llcomp_mi_codec* k, uint32_t n_dst, uint32_t n_pieces) {
    if (!k) return 0;
    return k->workspace_bytes + paste_table_bound<2>(n_dst, n_pieces);
}

// Batch copy-paste by wide ids (DESIGN.md "Wide id maps"): the same for masks of 3 or 4 bytes per pixel, the pieces cast to the
// width's type, in the 16-bit call's table buffer (the records have its size).
int llcomp_mi_codec_paste_batch32(llcomp_mi_codec* k, const void* d_src, const void* d_mask, uint32_t map_bytes, uint32_t n_src, uint32_t iw, uint32_t ih,
                                  void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece32* pieces,
                                  uint32_t n_pieces, void* stream) {
    if (!k) return LLCOMP_MI_BAD_ARGS;
    if (map_bytes == 3)
        return paste_batch_call(k, k->d_paste16_tab, k->paste16_tab_cap, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, dtype, layout,
                                static_cast<const PastePiece3*>(pieces), n_pieces, stream);
    if (map_bytes == 4)
        return paste_batch_call(k, k->d_paste16_tab, k->paste16_tab_cap, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, dtype, layout,
                                static_cast<const PastePiece4*>(pieces), n_pieces, stream);
    return LLCOMP_MI_BAD_ARGS;
}

uint64_t llcomp_mi_codec_paste32_workspace_bytes(const llcomp_mi_codec* k, uint32_t n_dst, uint32_t n_pieces) {
    if (!k) return 0;
    return k->workspace_bytes + paste_table_bound<4>(n_dst, n_pieces);
}

// Batch alpha paste (DESIGN.md "Batch alpha paste"): alpha_plan.hpp's checks, the copy-paste's plan and the table through the call's own
// table buffer, which the first such call allocates.  A call without a piece that has w and h queues nothing.
int llcomp_mi_codec_alpha_paste_batch(llcomp_mi_codec* k, const void* d_src, const void* d_alpha, uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src,
                                      uint32_t iw, uint32_t ih, void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                      const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, void* stream) {
    if (!k || !d_dst) return LLCOMP_MI_BAD_ARGS;
    const uint32_t c = k->g.c;
    AlphaUses uses;
    if (int rc = alpha_check_call(alpha_px_bytes, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, dtype, layout, pieces, n_pieces, uses)) return rc;
    const uint32_t esize = batch_esize(dtype);
    if (int rc = alpha_check_memory(d_src, uint64_t(n_src) * c * iw * ih * esize, d_alpha, uint64_t(alpha_px_bytes) * n_src * iw * ih, d_dst,
                                    uint64_t(n_dst) * c * ow * oh * esize, esize, uses))
        return rc;
    PastePlan p;
    alpha_plan(n_dst, pieces, n_pieces, p);
    if (p.samples.empty()) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_alpha_tab, k->alpha_tab_cap, AlphaTable(p.samples.size(), p.order.size()).bytes, alpha_table_bound(n_dst, n_pieces), s,
        [&](uint8_t* at) { alpha_table_put(pieces, p, c, layout, at); },
        [&](const uint8_t* d_table) {
            AlphaLaunch o{};
            o.d_src = static_cast<const uint8_t*>(d_src), o.d_alpha = static_cast<const uint8_t*>(d_alpha), o.d_dst = static_cast<uint8_t*>(d_dst);
            o.d_table = d_table, o.n_samples = uint32_t(p.samples.size()), o.n_recs = uint32_t(p.order.size());
            o.alpha_px_bytes = alpha_px_bytes, o.alpha_byte = alpha_byte;
            o.n_src = n_src, o.iw = iw, o.ih = ih, o.n_dst = n_dst, o.ow = ow, o.oh = oh, o.c = c, o.dtype = dtype, o.layout = layout, o.over = uses.over;
            return launch_alpha_paste(o, s);
        });
}

uint64_t llcomp_mi_codec_alpha_paste_workspace_bytes(const llcomp_mi_codec* k, uint32_t n_dst, uint32_t n_pieces) {
    if (!k) return 0;
    return k->workspace_bytes + alpha_table_bound(n_dst, n_pieces);
}

// Label boxes (DESIGN.md "Label boxes"): the codec gives the device; no table, no workspace.
int llcomp_mi_codec_label_boxes(llcomp_mi_codec* k, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, void* d_boxes, void* stream) {
    if (!k || !d_maps || !d_boxes) return LLCOMP_MI_BAD_ARGS;
    if (int rc = label_boxes_check_call(n, ow, oh)) return rc;
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps), b = reinterpret_cast<uintptr_t>(d_boxes);
    const uint64_t map_bytes = uint64_t(n) * ow * oh, box_bytes = uint64_t(n) * kLabelIds * sizeof(llcomp_mi_label_box);
    if (misaligned(d_boxes, 4) || (m < b + box_bytes && b < m + map_bytes)) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    HIP_TRY(launch_label_boxes(static_cast<const uint8_t*>(d_maps), n, ow, oh, static_cast<uint8_t*>(d_boxes), static_cast<hipStream_t>(stream)));
    return LLCOMP_MI_OK;
}

// Label boxes of listed ids (DESIGN.md "Label boxes of listed ids"): the lists travel as the batch calls' tables do.  A call without
// a listed id has no record to write and queues nothing.
int llcomp_mi_codec_label_boxes16(llcomp_mi_codec* k, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids,
                                  const uint32_t* first, void* d_boxes, void* stream) {
    if (!k || !d_maps) return LLCOMP_MI_BAD_ARGS;
    uint32_t longest = 0, n_listed = 0;
    if (int rc = label_boxes16_check_call(n, ow, oh, ids, first, &longest, &n_listed)) return rc;
    const uint32_t total = first[n];
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps), b = reinterpret_cast<uintptr_t>(d_boxes);
    const uint64_t map_bytes = 2 * uint64_t(n) * ow * oh, box_bytes = uint64_t(total) * sizeof(llcomp_mi_label_box);
    if (misaligned(d_maps, 2) || (total && (!d_boxes || misaligned(d_boxes, 4) || (m < b + box_bytes && b < m + map_bytes)))) return LLCOMP_MI_BAD_ARGS;
    if (!total) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_label16_tab, k->label16_tab_cap, Label16Table(n, n_listed, total).bytes, label16_table_bound(n, total), s,
        [&](uint8_t* at) { label16_table_put(n, ids, first, n_listed, at); },
        [&](const uint8_t* d_table) {
            return launch_label_boxes16(static_cast<const uint8_t*>(d_maps), n, ow, oh, d_table, n_listed, total, longest, static_cast<uint8_t*>(d_boxes), s);
        });
}

uint64_t llcomp_mi_codec_label_boxes16_workspace_bytes(const llcomp_mi_codec* k, uint32_t n, uint32_t total_ids) {
    if (!k) return 0;
    return k->workspace_bytes + label16_table_bound(n, total_ids);
}

// Label targets (DESIGN.md "Label targets"): the lists, the values and the planes travel as the batch calls' tables do.  A call without
// a sample that gets workgroups -- PLANES without a plane -- has nothing to write and queues nothing.
int llcomp_mi_codec_label_targets(llcomp_mi_codec* k, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* targets,
                                  void* d_out, void* stream) {
    if (!k || !d_maps || !d_out) return LLCOMP_MI_BAD_ARGS;
    TargetCall c;
    if (int rc = label_targets_check_call(n, ow, oh, targets, c)) return rc;
    const llcomp_mi_label_targets& t = *targets;
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps), o = reinterpret_cast<uintptr_t>(d_out);
    const uint64_t map_bytes = uint64_t(n) * ow * oh * t.map_bytes;
    if (misaligned(d_maps, t.map_bytes) || misaligned(d_out, c.esize) || (m < o + c.out_bytes && o < m + map_bytes)) return LLCOMP_MI_BAD_ARGS;
    if (!c.n_work) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_target_tab, k->target_tab_cap, TargetTable(n, c.n_work, c.total, t.kind == LLCOMP_MI_TARGET_PLANES).bytes, target_table_bound(n, c.total), s,
        [&](uint8_t* at) { target_table_put(n, t, c, at); },
        [&](const uint8_t* d_table) {
            return launch_label_targets(static_cast<const uint8_t*>(d_maps), n, ow, oh, t, c, d_table, static_cast<uint8_t*>(d_out), s);
        });
}

uint64_t llcomp_mi_codec_label_targets_workspace_bytes(const llcomp_mi_codec* k, uint32_t n, uint32_t total_ids) {
    if (!k) return 0;
    return k->workspace_bytes + target_table_bound(n, total_ids);
}

// Wide id maps (DESIGN.md "Wide id maps"): the two calls above for maps of 3 or 4 bytes per pixel and lists of uint32_t ids, in the
// 16-bit calls' table buffers.
int llcomp_mi_codec_label_boxes32(llcomp_mi_codec* k, const void* d_maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint32_t* ids,
                                  const uint32_t* first, void* d_boxes, void* stream) {
    if (!k || !d_maps) return LLCOMP_MI_BAD_ARGS;
    uint32_t longest = 0, n_listed = 0;
    if (int rc = label_boxes32_check_call(map_bytes, n, ow, oh, ids, first, &longest, &n_listed)) return rc;
    const uint32_t total = first[n];
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps), b = reinterpret_cast<uintptr_t>(d_boxes);
    const uint64_t maps_bytes = map_bytes * uint64_t(n) * ow * oh, box_bytes = uint64_t(total) * sizeof(llcomp_mi_label_box);
    if (label_map32_misaligned(m, map_bytes) || (total && (!d_boxes || misaligned(d_boxes, 4) || (m < b + box_bytes && b < m + maps_bytes)))) return LLCOMP_MI_BAD_ARGS;
    if (!total) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_label16_tab, k->label16_tab_cap, Label16Table(n, n_listed, total, 4).bytes, label32_table_bound(n, total), s,
        [&](uint8_t* at) { label32_table_put(n, ids, first, n_listed, at); },
        [&](const uint8_t* d_table) {
            return launch_label_boxes32(static_cast<const uint8_t*>(d_maps), map_bytes, n, ow, oh, d_table, n_listed, total, longest, static_cast<uint8_t*>(d_boxes), s);
        });
}

uint64_t llcomp_mi_codec_label_boxes32_workspace_bytes(const llcomp_mi_codec* k, uint32_t n, uint32_t total_ids) {
    if (!k) return 0;
    return k->workspace_bytes + label32_table_bound(n, total_ids);
}

int llcomp_mi_codec_label_targets32(llcomp_mi_codec* k, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* targets,
                                    void* d_out, void* stream) {
    if (!k || !d_maps || !d_out) return LLCOMP_MI_BAD_ARGS;
    TargetCall c;
    if (int rc = label_targets32_check_call(n, ow, oh, targets, c)) return rc;
    const llcomp_mi_label_targets32& t = *targets;
    const uint64_t m = reinterpret_cast<uintptr_t>(d_maps), o = reinterpret_cast<uintptr_t>(d_out);
    const uint64_t maps_bytes = uint64_t(n) * ow * oh * t.map_bytes;
    if (label_map32_misaligned(m, t.map_bytes) || misaligned(d_out, c.esize) || (m < o + c.out_bytes && o < m + maps_bytes)) return LLCOMP_MI_BAD_ARGS;
    if (!c.n_work) return LLCOMP_MI_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return batch_table_call(
        k, k->d_target_tab, k->target_tab_cap, TargetTable(n, c.n_work, c.total, t.kind == LLCOMP_MI_TARGET_PLANES, 4).bytes, target32_table_bound(n, c.total), s,
        [&](uint8_t* at) { target32_table_put(n, t, c, at); },
        [&](const uint8_t* d_table) {
            return launch_label_targets32(static_cast<const uint8_t*>(d_maps), n, ow, oh, t, c, d_table, static_cast<uint8_t*>(d_out), s);
        });
}

uint64_t llcomp_mi_codec_label_targets32_workspace_bytes(const llcomp_mi_codec* k, uint32_t n, uint32_t total_ids) {
    if (!k) return 0;
    return k->workspace_bytes + target32_table_bound(n, total_ids);
}

uint64_t llcomp_mi_codec_photo_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    const Geometry& g = k->g;
    const uint64_t views = std::max<uint64_t>(total_views, 1);
    return std::max(llcomp_mi_codec_padded_workspace_bytes(k, total_views), llcomp_mi_codec_warp_workspace_bytes(k, total_views)) +
           uint64_t(g.frames) * g.w * g.h * g.c + views * (photo_stats_stride(g.c) + photo_lut_stride(g.c)) + photo_tables_bound(total_views);
}

uint64_t llcomp_mi_codec_warp_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    return k->workspace_bytes + warp_tables_bound(k->g, total_views);
}

uint64_t llcomp_mi_codec_padded_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    return llcomp_mi_codec_views_workspace_bytes(k, total_views) + std::max<uint64_t>(total_views, k->g.frames) * padded_term(k->g) + 4 * uint64_t(k->g.c);
}

uint64_t llcomp_mi_codec_views_workspace_bytes(const llcomp_mi_codec* k, uint64_t total_views) {
    if (!k) return 0;
    return k->workspace_bytes + (total_views > k->g.frames ? (total_views - k->g.frames) * view_term(k->g) : 0);
}

uint32_t llcomp_mi_status_from_bits(uint32_t bits) { return uint32_t(status_from_bits(bits)); }

int llcomp_mi_device_copy_segments(const void* d_src, void* d_dst, const void* d_src_off, const void* d_dst_off, const void* d_len,
                                   uint32_t n_seg, uint64_t max_len, void* stream) {
    if (!n_seg) return LLCOMP_MI_OK;
    if (!d_src || !d_dst || !d_src_off || !d_dst_off || !d_len || n_seg > 65535) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_src_off, 8) || misaligned(d_dst_off, 8) || misaligned(d_len, 8)) return LLCOMP_MI_BAD_ARGS;  // (u64 tables; the bytes: any address)
    HIP_TRY(launch_copy_segments(static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), static_cast<const uint64_t*>(d_src_off),
                                 static_cast<const uint64_t*>(d_dst_off), static_cast<const uint64_t*>(d_len), n_seg, max_len,
                                 static_cast<hipStream_t>(stream)));
    return LLCOMP_MI_OK;
}

int llcomp_mi_device_range_sums(const void* d_vals, const void* d_start, const void* d_count, void* d_out, uint32_t n, uint32_t cap,
                                void* stream) {
    if (!n) return LLCOMP_MI_OK;
    if (!d_vals || !d_start || !d_count || !d_out) return LLCOMP_MI_BAD_ARGS;
    if (misaligned(d_vals, 4) || misaligned(d_start, 8) || misaligned(d_count, 8) || misaligned(d_out, 8)) return LLCOMP_MI_BAD_ARGS;
    HIP_TRY(launch_range_sums(static_cast<const uint32_t*>(d_vals), static_cast<const uint64_t*>(d_start), static_cast<const uint64_t*>(d_count),
                              static_cast<uint64_t*>(d_out), n, cap, static_cast<hipStream_t>(stream)));
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_get_counters(llcomp_mi_codec* k, uint64_t* out, uint32_t n, int reset) {
    if (!k || !out || n > kCtrCount) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    // the codec's last call has to be done before its counts mean anything: wait for ITS event (not for the device)
    if (k->done && k->done->ev && hipEventSynchronize(k->done->ev) != hipSuccess) (void)hipGetLastError();
    uint64_t dev[kCtrCount];
    HIP_TRY(hipMemcpy(dev, k->d_counters, sizeof(dev), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) out[i] = dev[i] + k->host_counters[i];
    if (reset) {
        HIP_TRY(hipMemset(k->d_counters, 0, sizeof(dev)));
        for (auto& h : k->host_counters) h = 0;
        k->fb_seen[0] = k->fb_seen[1] = 0;
        k->fb_pending = false;  // (a mailbox copy still in flight would carry pre-reset values)
        if (k->h_feedback) k->h_feedback[0] = k->h_feedback[1] = 0;
    }
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_set_profiling(llcomp_mi_codec* k, int enable) {
    if (!k) return LLCOMP_MI_BAD_ARGS;
    k->profiling = enable != 0;
    return LLCOMP_MI_OK;
}

int llcomp_mi_codec_get_profile(llcomp_mi_codec* k, double* ms8, uint32_t* n_encode, uint32_t* n_decode) {
    if (!k || !ms8) return LLCOMP_MI_BAD_ARGS;
    DeviceGuard guard(k->device);
    for (int i = 0; i < 8; ++i) ms8[i] = 0.0;
    int rc = LLCOMP_MI_OK;
    for (auto& sp : k->spans) {
        float ms = 0.f;
        if (hipEventSynchronize(sp.b) != hipSuccess || hipEventElapsedTime(&ms, sp.a, sp.b) != hipSuccess) rc = LLCOMP_MI_HIP_ERROR;
        ms8[sp.slot] += ms;
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    k->spans.clear();
    if (n_encode) *n_encode = k->n_encode;
    if (n_decode) *n_decode = k->n_decode;
    k->n_encode = k->n_decode = 0;
    return rc;
}

}  // extern "C"

#if defined(LLMI_TEST_FAIL_ALLOC) && LLMI_TEST_FAIL_ALLOC
// The guard build with the allocation fault injector (devmem.hip; tests/test_gpu_alloc_failures.py calls this after every injected
// failure and makes its follow-up call only on 0): a host-only walk of the codec object.  0, or the number of the first broken invariant:
//    1  a buffer the codec is created with is missing
//    2  the snapshot arrays are there in part (sorted / banks / residuals / snap_el; context / chunk states)
//    3  snapshot arrays with chunks without the coder's parking records
//    4  parking records, overlap on, and the second stream or one of its events missing
//    5  d_region_len without d_region_off, or the reverse
//    6  d_regions without a slot of the pinned ring or one of its events, or a slot too small for a table
//    7  a slot of the ring and its capacity disagree
//    8  a grown buffer and its capacity disagree (the n-th of the list below: 8 + 100 * n)
//    9  a pointer of the object is no live block of the allocator (the n-th of the walk: 9 + 100 * n)
//   10  allocated_bytes is not the sum of what the object's blocks were asked for
//   11  what the codec holds, the batch calls' tables and the chains' buffers aside, is above workspace_bytes
extern "C" int llmi_test_codec_consistent(const llcomp_mi_codec* k) {
    if (!k) return -1;
    if (!k->d_sym_or_rec || !k->d_lane_order || !k->d_scratch || !k->d_group_off || !k->d_total_tmp || !k->d_counters) return 1;
    const bool some = k->d_snap_sorted || k->d_snap_banks || k->d_snap_res || k->snap_el;
    const bool all = k->d_snap_sorted && k->d_snap_banks && k->d_snap_res && k->snap_el;
    if (some != all || !k->d_snap_ctx != !k->d_snap_io || (k->d_snap_ctx && !all)) return 2;
    if (k->d_snap_ctx && !k->d_seg_state) return 3;
    if (k->d_seg_state && k->overlap) {
        if (!k->aux || !k->ev_fork) return 4;
        for (hipEvent_t ev : k->ev_chunk)
            if (!ev) return 4;
    }
    if (!k->d_region_len != !k->d_region_off) return 5;
    for (uint32_t i = 0; i < llcomp_mi_codec::kRegionsRing; ++i) {
        if (k->d_regions && (!k->h_regions[i] || !k->regions_ev[i] || k->h_regions_cap[i] < uint64_t(k->g.frames) * sizeof(RegionsFrame))) return 6;
        if (!k->h_regions[i] != !k->h_regions_cap[i]) return 7;
    }
    const struct { const void* p; uint64_t cap; } grown[] = {
        {k->d_stage, k->stage_cap},           {k->d_box, k->box_cap},           {k->d_mid, k->mid_cap},           {k->d_photo, k->photo_cap},
        {k->d_photo_tab, k->photo_tab_cap},   {k->d_mix_tab, k->mix_tab_cap},   {k->d_mix, k->mix_cap},           {k->d_orient_tab, k->orient_tab_cap},
        {k->d_compose_tab, k->compose_tab_cap}, {k->d_paste_tab, k->paste_tab_cap}, {k->d_paste16_tab, k->paste16_tab_cap}, {k->d_alpha_tab, k->alpha_tab_cap},
        {k->d_label16_tab, k->label16_tab_cap}, {k->d_target_tab, k->target_tab_cap}};
    int n = 0;
    for (const auto& gb : grown) {
        if (!gb.p != !gb.cap) return 8 + 100 * n;
        ++n;
    }
    const void* const held[] = {k->d_sym_or_rec,  k->d_lane_order, k->d_states,     k->d_scratch,     k->d_group_off,   k->d_total_tmp, k->d_region_len,
                                k->d_region_off,  k->d_regions,    k->d_stage,      k->d_box,         k->d_mid,         k->d_photo,     k->d_photo_tab,
                                k->d_mix_tab,     k->d_mix,        k->d_orient_tab, k->d_compose_tab, k->d_paste_tab,   k->d_paste16_tab, k->d_alpha_tab,
                                k->d_label16_tab, k->d_target_tab, k->d_upd_goff,   k->d_snap_sorted, k->d_snap_banks,  k->d_snap_res,
                                k->d_snap_ctx,    k->d_snap_io,    k->d_seg_state};
    uint64_t sum = 0;
    n = 0;
    for (const void* p : held) {
        if (p) {
            const uint64_t asked = test_block_requested(p);
            if (asked == ~0ull) return 9 + 100 * n;
            sum += asked;
        }
        ++n;
    }
    if (test_block_requested(k->d_counters) == ~0ull) return 9 + 100 * n;  // (the counters are not part of allocated_bytes)
    if (sum != k->allocated_bytes) return 10;
    uint64_t aside = k->photo_cap + k->photo_tab_cap + k->mix_tab_cap + k->mix_cap + k->orient_tab_cap + k->compose_tab_cap + k->paste_tab_cap +
                     k->paste16_tab_cap + k->alpha_tab_cap + k->label16_tab_cap + k->target_tab_cap;
    const uint64_t stage = stage_bound(k->g) + resized_tables_bound(k->g);  // (what workspace_bytes counts for d_stage: more views add more)
    if (k->stage_cap > stage) aside += k->stage_cap - stage;
    if (k->allocated_bytes - aside > k->workspace_bytes) return 11;
    return 0;
}
#endif
