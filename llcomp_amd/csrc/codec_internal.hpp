// codec_internal.hpp -- the codec object behind llcomp_mi_codec_* and the helpers the host-side translation units share
// (codec.hip: device-resident batch codec; hostapi.hip: host-buffer drop-in calls; stream.hip: streaming pipeline).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "geometry.hpp"
#include "kernels.hpp"

namespace llcomp_mi {
struct DoneEvent {  // devmem.hip: completion event that travels with parked device blocks
    hipEvent_t ev = nullptr;
    ~DoneEvent();
};
std::shared_ptr<DoneEvent> make_done_event();
}  // namespace llcomp_mi

struct llcomp_mi_codec {
    llcomp_mi::Geometry g{};
    int device = 0;
    // workspace (all on `device`)
    void* d_sym_or_rec = nullptr;    // image order: encode u32 symbols per sample / decode int16 reconstructed samples
    void* d_lane_order = nullptr;    // the same data in lane order [group][k][64] for the serial kernels
    uint64_t* d_states = nullptr;    // u64[lane group][kContexts][lanes of the group]
    uint8_t* d_scratch = nullptr;    // slice streams in stream lane order: 16-byte units [group][unit][lane]
    uint64_t* d_group_off = nullptr; // u64[lane groups + 1]: payload offset of every lane group's first slice
    uint64_t* d_total_tmp = nullptr;
    // region decode (llcomp_mi_codec_decode_region): length and payload offset of every covered slice, u32[n_slices] + u64[n_slices],
    // allocated by the first region call (or llcomp_mi_codec_prepare(LLCOMP_MI_PREPARE_REGION))
    uint32_t* d_region_len = nullptr;
    uint64_t* d_region_off = nullptr;
    llcomp_mi::Tuning tune{};        // the hooks the geometry was made with (a region's sub-geometry is made with the same)
    // regions decode (llcomp_mi_codec_decode_regions): the per-frame table (RegionsFrame[frames], class by class) in HBM, and the
    // pinned staging it is copied from -- a ring of kRegionsRing slots, each reused only after the event behind ITS last copy
    // (the copy of a call sits in the stream behind that call's predecessors: one slot would make every call wait for the last one).
    // A slot holds one table; a host-staged call (llcomp_mi_codec_decode_regions_host) grows the slot it uses to hold all it stages.
    static constexpr uint32_t kRegionsRing = 4;
    llcomp_mi::RegionsFrame* d_regions = nullptr;
    uint8_t* h_regions[kRegionsRing] = {};       // pinned, h_regions_cap[i] bytes each (at least frames table entries)
    uint64_t h_regions_cap[kRegionsRing] = {};
    hipEvent_t regions_ev[kRegionsRing] = {};
    bool regions_ev_live[kRegionsRing] = {};     // the slot's event has been recorded (a copy from it may be queued)
    uint32_t regions_slot = 0;                   // the slot the next call uses
    // host-staged regions decode: where a slot's one copy lands -- [RegionsFrame table][u32 window lengths][u64 offsets][payload]
    // (windows_plan.hpp: StageLayout), the resample block of a resized or views call behind it; grown geometrically up to stage_bound(g)
    // plus the call's tables bound, allocated by the first such call
    uint8_t* d_stage = nullptr;
    uint64_t stage_cap = 0;
    // resized regions decode (llcomp_mi_codec_decode_resized_regions): every frame's box [frames][bh][bw][c] and the horizontal pass's
    // rows [frames][bh][ow][c], each grown geometrically (LLCOMP_MI_PREPARE_RESIZED allocates both at frames * w * h * c)
    uint8_t* d_box = nullptr;
    uint64_t box_cap = 0;
    uint8_t* d_mid = nullptr;
    uint64_t mid_cap = 0;
    // photometric chains (llcomp_mi_codec_decode_photo_views / _photo_warped_views): the staging buffer a group with chains is resampled
    // or warped into as U8 HWC, a chunk of views at a time, grown like d_mid and never past frames * w * h * c for outputs no larger than
    // the image; and the statistics (u64 + c * 256 u32 per view) and tables (c * 256 bytes per view) of the largest chunk's views
    uint8_t* d_photo = nullptr;
    uint64_t photo_cap = 0;
    uint8_t* d_photo_tab = nullptr;
    uint64_t photo_tab_cap = 0;
    // batch mixing (llcomp_mi_codec_mix_batch): where a call's one copy lands -- the records, the order, the segments and the erase values
    // (mix_plan.hpp: MixTable) -- and the saved heads of the segments of cut cycles, one slot of mix_slot_stride bytes each; both grown
    // by the calls that need more
    uint8_t* d_mix_tab = nullptr;
    uint64_t mix_tab_cap = 0;
    uint8_t* d_mix = nullptr;
    uint64_t mix_cap = 0;
    // batch orientation (llcomp_mi_codec_orient_batch): where a call's one copy lands, the oriented samples and their codes
    // (orient_plan.hpp: OrientEntry); grown by the calls that need more
    uint8_t* d_orient_tab = nullptr;
    uint64_t orient_tab_cap = 0;
    // batch composition (llcomp_mi_codec_compose_batch): where a call's one copy lands, the samples, the pieces and the fill values
    // (compose_plan.hpp: ComposeTable); grown by the calls that need more
    uint8_t* d_compose_tab = nullptr;
    uint64_t compose_tab_cap = 0;
    // batch copy-paste (llcomp_mi_codec_paste_batch): where a call's one copy lands, the samples and the pieces with their id sets
    // (paste_plan.hpp: PasteTable); grown by the calls that need more
    uint8_t* d_paste_tab = nullptr;
    uint64_t paste_tab_cap = 0;
    // batch copy-paste by 16-bit ids (llcomp_mi_codec_paste_batch16): the same with records of 72 bytes (paste_plan.hpp: PasteTable<2>)
    uint8_t* d_paste16_tab = nullptr;
    uint64_t paste16_tab_cap = 0;
    // batch alpha paste (llcomp_mi_codec_alpha_paste_batch): where a call's one copy lands, the samples and the pieces with their values
    // (alpha_plan.hpp: AlphaTable, records of 36 bytes); allocated by the first such call, grown by the calls that need more
    uint8_t* d_alpha_tab = nullptr;
    uint64_t alpha_tab_cap = 0;
    // label boxes of listed ids (llcomp_mi_codec_label_boxes16): where a call's one copy lands, the lists' bounds, the listed samples and
    // the ids (label_lists.hpp: Label16Table); grown by the calls that need more
    uint8_t* d_label16_tab = nullptr;
    uint64_t label16_tab_cap = 0;
    // label targets (llcomp_mi_codec_label_targets): where a call's one copy lands, the lists' and the planes' bounds, the samples that
    // get workgroups, the values and the ids (label_targets_rule.hpp: TargetTable); grown by the calls that need more
    uint8_t* d_target_tab = nullptr;
    uint64_t target_tab_cap = 0;
    // region update (llcomp_mi_codec_encode_region / _update_region): the encoder runs on the box's sub-geometry, which can have MORE lane
    // groups than the full one, so its group offsets go to an array of their own, u64[n_slices + 1]; behind it, u64[lane groups + 1], the
    // full geometry's group offsets for the NEW table (d_group_off holds the old table's).  The decoded box shares d_box with the resized
    // path.  Allocated by the first such call (or LLCOMP_MI_PREPARE_UPDATE).
    uint64_t* d_upd_goff = nullptr;
    uint64_t snap_el = 0;            // elements every snapshot array holds
    void* d_snap_sorted = nullptr;   // snapshot pass of the 2-D encoder (snapshot.hpp): banks in context-sorted order,
    void* d_snap_banks = nullptr;    // banks in stream order, residuals in stream order; null unless snapshot_mode(g)
    void* d_snap_res = nullptr;
    void* d_snap_ctx = nullptr;      // ... slices above 4096 samples (snapshot_chunked): the context of every sorted position (u16) and the
    void* d_snap_io = nullptr;       // states every context run of a chunk starts from (u64), both scratch of the pass
    // ... their coder runs in segments of 4096 samples (a lane parks its coder in 64 bytes per slice in between), each behind ITS chunk
    // of the pass only: the pass works ahead of the coder on a second stream (one per device, shared by all codecs; fork / join with
    // events, so the caller's stream still orders everything; LLCOMP_MI_OVERLAP=0: in order, =1: a second stream of the codec's own)
    uint32_t* d_seg_state = nullptr;
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_chunk[llcomp_mi::kSnapMaxChunks] = {};
    bool overlap = true;             // (LLCOMP_MI_OVERLAP when the codec was made)
    bool aux_shared = true;          // (`aux` is the device's shared second stream, not this codec's to destroy)
    uint64_t workspace_bytes = 0;    // what the codec can hold at most
    uint64_t allocated_bytes = 0;    // what it holds right now (state tables / snapshot arrays come with the first call that needs them)
    // Event counters (kernels.hpp kCtr*): kernel-side u64[kCtrCount] in HBM, host-side additions, and the feedback that takes the bank
    // cache away from a codec whose 2-D decode wavefronts ALL gave it up: a cached launch is followed by a 16-byte copy of
    // {cached wavefronts, bypassed wavefronts} into a pinned mailbox + an event; the next decode call looks at the event WITHOUT waiting
    // (no result yet = no change) and runs the plain kernel -- no LDS held for a cache nobody uses, so the helper kernels beside it find
    // room on the CUs -- for kPlainRun calls before it probes with the cache again.
    unsigned long long* d_counters = nullptr;
    uint64_t host_counters[llcomp_mi::kCtrCount] = {};
    uint64_t* h_feedback = nullptr;    // pinned: [0] cached wavefronts, [1] bypassed wavefronts (cumulative), as of fb_event
    hipEvent_t fb_event = nullptr;
    bool fb_pending = false;           // a mailbox copy has been queued and not looked at yet
    uint64_t fb_seen[2] = {0, 0};      // the mailbox's values at the last look
    uint32_t plain_calls_left = 0;     // > 0: this many decode calls run without the bank cache
    bool feedback = true;              // (LLCOMP_MI_NOFEEDBACK=1 when the codec was made: the cache stays on in every launch)
    static constexpr uint32_t kPlainRun = 15;
    bool need_states = true;  // false when the states live in LDS (1-row slices; one slice per wavefront)
    uint32_t state_generation = 0;  // tag of the last call that used d_states (kernels.hpp); 0 = the table has not been cleared yet
    // optional per-kernel timing (hipEvents on the caller's stream)
    bool profiling = false;
    struct Span { hipEvent_t a, b; int slot; };
    std::vector<Span> spans;
    uint32_t n_encode = 0, n_decode = 0;
    // recorded on the caller's stream behind the last launch of every encode / decode: the codec's device blocks are
    // parked with it when the codec is destroyed (no device-wide wait on destroy)
    std::shared_ptr<llcomp_mi::DoneEvent> done;
};

namespace llcomp_mi {

#define LLMI_HIP_TRY(expr)                                \
    do {                                                  \
        hipError_t _e = (expr);                           \
        if (_e != hipSuccess) return LLCOMP_MI_HIP_ERROR; \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) return;
        ok = (dev == prev) || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (ok && prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int status_from_bits(uint32_t bits);
Tuning current_tuning();  // environment hooks, read once per process (llcomp_mi_reload_tuning re-reads them)
int resolve_device(int32_t device, int* out);
// argument checks shared by every entry point that takes an image shape: BAD_ARGS for nonsense, OUT_OF_RANGE for sizes
// the formats cannot express (reference: silent truncation / int overflow)
int check_shape(uint32_t w, uint32_t h, uint32_t c, bool legacy);

// One coding lane of the host-side calls: a codec object for ONE frame plus everything a host buffer needs on its way
// through the GPU -- a private HIP stream (never the NULL stream: concurrent callers do not serialise device-wide),
// the frame and the container in HBM laid out exactly as on the wire ([header][slice table][payload], so a container
// crosses PCIe in ONE copy), and a pinned 16-byte mailbox for {payload bytes, status}.
struct HostLane {
    llcomp_mi_codec* k = nullptr;
    hipStream_t stream = nullptr;
    uint8_t* d_px = nullptr;
    uint8_t* d_container = nullptr;  // [header][u32 length table (sliced only)][payload capacity]
    uint32_t* d_len_legacy = nullptr;  // the legacy format has no table on the wire: its single length lives here
    uint64_t* d_meta = nullptr;      // [0] payload bytes (u64)  [1] low dword: status bits of the last call  [2 + f] payload bytes of frame f
    uint64_t* h_meta = nullptr;      // pinned mirror of d_meta
    uint32_t frames = 1;             // frames per call (> 1 only in the streaming pipeline)
    uint64_t payload_cap = 0;
    uint32_t head_bytes = 0;         // 6 (legacy) or 24 + 4 * slices (all frames' tables back to back)
    bool legacy = false;
    uint64_t bytes = 0;              // device bytes held (idle-cache budget)

    uint32_t* d_len() const { return legacy ? d_len_legacy : reinterpret_cast<uint32_t*>(d_container + LLCOMP_MI_SLICED_HEADER_BYTES); }
    uint8_t* d_payload() const { return d_container + head_bytes; }
    uint64_t raw_bytes() const { return uint64_t(k->g.w) * k->g.h * k->g.c * frames; }
    size_t meta_bytes() const { return 16 + 8 * size_t(frames); }
};
// builds a lane for this shape on `dev` (geometry + tuning hooks are fixed here); payload capacity `cap` bytes
// legacy_stream: bytes of the LEGACY stream the lane's decoder has to stage (fit_legacy_stream; 0 = the proven encoder bound)
int lane_create(HostLane** out, int dev, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar,
                bool legacy, uint64_t payload_cap, bool small_model = false, uint32_t frames = 1, uint64_t legacy_stream = 0);
int lane_grow(HostLane* l, uint64_t payload_cap);  // reallocates the container buffer (contents lost)
void lane_destroy(HostLane* l);
// enqueue on the lane's stream (asynchronous): frame in d_px -> container in d_container, {bytes, status} -> h_meta
int lane_enqueue_encode(HostLane* l);
// container in d_container (header + tables + `payload_bytes` of payload) -> frame(s) in d_px, status -> h_meta
int lane_enqueue_decode(HostLane* l, uint64_t payload_bytes);
// drains the lane's stream and returns the status the last enqueued call left in the mailbox
int lane_wait_status(HostLane* l);
// lane_enqueue_encode + lane_wait_status; a payload that overflows the lane's capacity is coded once more with room for the codec's
// proven bound (lane_grow; the frame is still in d_px).  The one OUTPUT_OVERFLOW retry of the encoders.
int lane_encode_sync(HostLane* l);

// hostapi.hip: a lane for this shape on `device` (-1 = current) from the cache of idle lanes, or a new one; lane_release parks it again
int lane_acquire(HostLane** out, int32_t device, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar,
                 bool legacy, uint64_t min_cap, bool small_model, uint64_t legacy_stream = 0);
void lane_release(HostLane* l);

// multidev.hip: one image over a device list, in this process (llcomp_mi_opts.devices / llcomp_mi_decode_devices)
struct DeviceList {
    const int32_t* devices;
    uint32_t n;
    uint32_t chunks_per_device;  // 0 = 4
};
// `out` != nullptr: caller's buffer of out_cap bytes; else the container is malloc'ed and returned through *out_alloc
int encode_multi(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, bool small_model,
                 const DeviceList& dl, uint8_t* out, size_t out_cap, uint8_t** out_alloc, size_t* out_len);
// *handled = false (and nothing done) when the container has to go through the one-device path (its table does not fit its payload)
int decode_multi(const uint8_t* data, size_t len, const llcomp_mi_info& info, const DeviceList& dl, uint8_t* px, size_t px_cap,
                 uint8_t** px_alloc, uint32_t* w, uint32_t* h, uint32_t* c, bool* handled);
// the thread's record behind LLCOMP_MI_DEVICE_FAILED (llcomp_mi_last_device_error)
void clear_device_error();
int device_failed(int32_t device, uint32_t index, int status);  // records it and returns LLCOMP_MI_DEVICE_FAILED

void codec_release(llcomp_mi_codec* k);
// codec.hip: llcomp_mi_codec_create_ex whose slices can stage a LEGACY stream of `legacy_stream` bytes (fit_legacy_stream)
int codec_create(llcomp_mi_codec** out, int32_t device, uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h,
                 uint32_t planar, uint32_t flags, uint64_t legacy_stream);  // codec.hip: destroy without the device-wide wait (its work is known to be done)

// devmem.hip: every device buffer of the library comes from here.  dev_alloc is hipMalloc on the current device through a
// cache of parked blocks; dev_free parks a block -- either the caller has made sure nothing in flight still uses it (the
// lanes drain their private stream), or it passes the event behind the last use and the block is handed out again only
// after that event; dev_release_idle hands the parked blocks back to the driver.
hipError_t dev_alloc(void** p, uint64_t bytes);
void dev_free(void* p, const std::shared_ptr<DoneEvent>& done = nullptr);  // done: reuse only after this event
void dev_release_idle();
uint64_t dev_idle_bytes();
void dev_set_limit(uint64_t bytes_per_device);  // parked bytes allowed per device (0: every free goes to the driver)
uint64_t dev_limit();
// ... and every pinned buffer from here: hipHostMalloc and hipHostFree
hipError_t host_alloc_pinned(void** p, size_t bytes, unsigned int flags);
hipError_t host_free_pinned(void* p);
#if defined(LLMI_TEST_FAIL_ALLOC) && LLMI_TEST_FAIL_ALLOC
// the guard build with the allocation fault injector (devmem.hip): the bytes the holder of live block p asked for, ~0 for a pointer that
// is no live block
uint64_t test_block_requested(const void* p);
#endif

}  // namespace llcomp_mi
