// hostapi.hip -- host-buffer calls of libllcomp_mi.so: the drop-in for llcomp::compressImage / decompressImage
// (/root/reference/llcomp.hpp:358, 461; callers llcompc.cpp:33, llcompd.cpp:26).
//
// A call takes a "lane" (codec_internal.hpp: codec object for one frame + private HIP stream + the frame and the container
// in HBM in wire layout) from a small cache keyed by device + geometry, copies the input over PCIe, enqueues the kernels,
// reads back {payload bytes, status} through a pinned mailbox and then the container / the pixels in ONE copy of the
// exact size.  Nothing runs on the NULL stream and nothing synchronises the device: concurrent callers overlap.
// With buffers from llcomp_mi_host_alloc (pinned) on both sides the copies are plain DMA; with pageable buffers the HIP
// runtime stages them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <optional>
#include <vector>

#include "../../include/llcomp_mi.h"
#include "codec_internal.hpp"
#include "container.hpp"
#include "host_result.hpp"

using namespace llcomp_mi;

namespace llcomp_mi {

void lane_destroy(HostLane* l) {
    if (!l) return;
    {
        DeviceGuard guard(l->k ? l->k->device : 0);
        if (l->stream) (void)hipStreamSynchronize(l->stream);
        if (l->k) l->k->done.reset();  // the lane's stream is drained and about to be destroyed: no event may refer to it afterwards
        dev_free(l->d_px);
        dev_free(l->d_container);
        dev_free(l->d_len_legacy);
        dev_free(l->d_meta);
        if (l->h_meta) (void)host_free_pinned(l->h_meta);
        if (l->stream) (void)hipStreamDestroy(l->stream);
    }
    codec_release(l->k);  // the lane's stream was synchronised above; nothing else runs on this codec
    delete l;
}

static int lane_write_header(HostLane* l) {
    uint8_t head[LLCOMP_MI_SLICED_HEADER_BYTES];
    const Geometry& g = l->k->g;
    if (l->legacy) write_legacy_header(head, g.w, g.h, g.c);
    else write_sliced_header(head, g);
    LLMI_HIP_TRY(hipMemcpyAsync(l->d_container, head, l->legacy ? 6 : LLCOMP_MI_SLICED_HEADER_BYTES, hipMemcpyHostToDevice, l->stream));
    LLMI_HIP_TRY(hipStreamSynchronize(l->stream));  // `head` lives on this stack frame
    return LLCOMP_MI_OK;
}

int lane_grow(HostLane* l, uint64_t payload_cap) {
    if (payload_cap <= l->payload_cap) return LLCOMP_MI_OK;
    DeviceGuard guard(l->k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    (void)hipStreamSynchronize(l->stream);
    dev_free(l->d_container);
    l->d_container = nullptr;
    l->bytes -= l->head_bytes + l->payload_cap;
    l->payload_cap = 0;
    if (dev_alloc(reinterpret_cast<void**>(&l->d_container), l->head_bytes + payload_cap + 16) != hipSuccess) return LLCOMP_MI_NOMEM;
    l->payload_cap = payload_cap;
    l->bytes += l->head_bytes + payload_cap;
    return lane_write_header(l);
}

int lane_create(HostLane** out, int dev, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar,
                bool legacy, uint64_t payload_cap, bool small_model, uint32_t frames, uint64_t legacy_stream) {
    *out = nullptr;
    HostLane* l = new (std::nothrow) HostLane;
    if (!l) return LLCOMP_MI_NOMEM;
    l->legacy = legacy;
    l->frames = frames;
    if (int rc = codec_create(&l->k, dev, frames, w, h, c, tile_w, tile_h, planar, small_model ? LLCOMP_MI_FLAG_SMALL_MODEL : 0,
                              legacy ? legacy_stream : 0)) {
        delete l;
        return rc;
    }
    DeviceGuard guard(dev);
    const Geometry& g = l->k->g;
    l->head_bytes = legacy ? 6u : uint32_t(LLCOMP_MI_SLICED_HEADER_BYTES) + 4u * g.n_slices;
    const uint64_t raw = l->raw_bytes();
    const bool ok = guard.ok && hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&l->d_px), raw + 4) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&l->d_len_legacy), 4) == hipSuccess &&
                    dev_alloc(reinterpret_cast<void**>(&l->d_meta), l->meta_bytes()) == hipSuccess &&
                    host_alloc_pinned(reinterpret_cast<void**>(&l->h_meta), l->meta_bytes(), hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        lane_destroy(l);
        return LLCOMP_MI_NOMEM;
    }
    l->bytes = raw + 24;
    if (int rc = lane_grow(l, payload_cap)) {
        lane_destroy(l);
        return rc;
    }
    *out = l;
    return LLCOMP_MI_OK;
}

int lane_enqueue_encode(HostLane* l) {
    if (int rc = llcomp_mi_codec_encode(l->k, l->d_px, l->d_payload(), l->payload_cap, l->d_len(), l->d_meta, l->d_meta + 1, l->stream))
        return rc;
    if (l->frames > 1) LLMI_HIP_TRY(launch_frame_bytes(l->k->g, l->d_len(), l->d_meta + 2, l->stream));
    LLMI_HIP_TRY(hipMemcpyAsync(l->h_meta, l->d_meta, l->meta_bytes(), hipMemcpyDeviceToHost, l->stream));
    return LLCOMP_MI_OK;
}

// a LEGACY stream has no table on the wire: its one length is what follows the header
static int lane_set_legacy_len(HostLane* l, uint64_t payload_bytes) {
    if (!l->legacy) return LLCOMP_MI_OK;
    const uint32_t one = uint32_t(std::min<uint64_t>(payload_bytes, 0xFFFFFFFFull));
    LLMI_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(l->d_len_legacy), int(one), 1, l->stream));
    return LLCOMP_MI_OK;
}

int lane_enqueue_decode(HostLane* l, uint64_t payload_bytes) {
    if (int rc = lane_set_legacy_len(l, payload_bytes)) return rc;
    if (int rc = llcomp_mi_codec_decode(l->k, l->d_payload(), payload_bytes, l->d_len(), l->d_px, l->d_meta + 1, l->stream)) return rc;
    LLMI_HIP_TRY(hipMemcpyAsync(l->h_meta, l->d_meta, 16, hipMemcpyDeviceToHost, l->stream));
    return LLCOMP_MI_OK;
}

int lane_wait_status(HostLane* l) {
    LLMI_HIP_TRY(hipStreamSynchronize(l->stream));
    return status_from_bits(uint32_t(l->h_meta[1]));
}

int lane_encode_sync(HostLane* l) {
    return with_overflow_retry(l->payload_cap, llcomp_mi_codec_max_payload_bytes(l->k), [&](uint64_t cap) {
        if (int rc = lane_grow(l, cap)) return rc;  // (the container buffer's contents are lost, the frame is still in d_px)
        if (int rc = lane_enqueue_encode(l)) return rc;
        return lane_wait_status(l);
    });
}

}  // namespace llcomp_mi

namespace {

// A lane holds GBs of workspace for a 4K frame; allocating it per call costs more than the coding.  A few idle ones are
// kept, keyed by device + geometry (which includes the kernel family the tuning hooks selected when the lane was
// made).  Never torn down at exit on purpose (the HIP runtime may already be gone by then).
struct LaneCache {
    struct Item { HostLane* l; uint64_t stamp; };
    std::mutex mu;
    std::vector<Item> idle;
    uint64_t clock = 0;
    // per device: a device list parks a lane on every GPU, concurrent callers one each (an 8192 x 8192 lane holds about 10 GB of the
    // GPU's 288)
    static constexpr size_t kMaxIdle = 6;
    static constexpr uint64_t kMaxIdleBytes = 40ull << 30;

    HostLane* take(int dev, const Geometry& g, bool legacy) {
        std::lock_guard<std::mutex> lock(mu);
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].l->k->device == dev && idle[i].l->legacy == legacy && std::memcmp(&idle[i].l->k->g, &g, sizeof(Geometry)) == 0) {
                HostLane* l = idle[i].l;
                idle.erase(idle.begin() + long(i));
                return l;
            }
        return nullptr;
    }
    void give(HostLane* l) {
        std::vector<HostLane*> drop;
        {
            std::lock_guard<std::mutex> lock(mu);
            idle.push_back({l, ++clock});
            // the limits hold PER DEVICE (a device list parks one lane on every GPU); bytes = what the lane holds right now (the
            // codec's state tables / snapshot arrays only once a call has allocated them)
            const int dev = l->k->device;
            auto count = [&]() { size_t n = 0; for (auto& it : idle) n += it.l->k->device == dev; return n; };
            auto bytes = [&]() { uint64_t b = 0; for (auto& it : idle) if (it.l->k->device == dev) b += it.l->k->allocated_bytes + it.l->bytes; return b; };
            while (count() > kMaxIdle || (count() > 1 && bytes() > kMaxIdleBytes)) {
                size_t oldest = idle.size();
                for (size_t i = 0; i < idle.size(); ++i)
                    if (idle[i].l->k->device == dev && (oldest == idle.size() || idle[i].stamp < idle[oldest].stamp)) oldest = i;
                drop.push_back(idle[oldest].l);
                idle.erase(idle.begin() + long(oldest));
            }
        }
        for (auto* d : drop) lane_destroy(d);
    }
};
void drop_idle_lanes(LaneCache& c) {
    std::vector<HostLane*> drop;
    {
        std::lock_guard<std::mutex> lock(c.mu);
        for (auto& it : c.idle) drop.push_back(it.l);
        c.idle.clear();
    }
    for (auto* d : drop) lane_destroy(d);
}
LaneCache& lane_cache() {
    static LaneCache* c = new LaneCache;  // leaked deliberately
    return *c;
}

}  // namespace

namespace llcomp_mi {
int lane_acquire(HostLane** out, int32_t device, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar,
                 bool legacy, uint64_t min_cap, bool small_model, uint64_t legacy_stream) {
    Geometry g;
    std::memset(&g, 0, sizeof(g));
    if (!make_geometry(g, 1, w, h, c, tile_w, tile_h, planar, current_tuning(), small_model)) return LLCOMP_MI_OUT_OF_RANGE;
    if (legacy && legacy_stream) fit_legacy_stream(g, legacy_stream);  // (part of the key: such a lane serves streams up to its size)
    int dev = 0;
    if (int rc = resolve_device(device, &dev)) return rc;
    if ((*out = lane_cache().take(dev, g, legacy))) {
        if (int rc = lane_grow(*out, min_cap)) {  // (a lane whose container buffer could not be reallocated is of no use to anybody)
            lane_destroy(*out);
            *out = nullptr;
            return rc;
        }
        return LLCOMP_MI_OK;
    }
    return lane_create(out, dev, w, h, c, tile_w, tile_h, planar, legacy, min_cap, small_model, 1, legacy_stream);
}
void lane_release(HostLane* l) {
    if (l) lane_cache().give(l);
}
}  // namespace llcomp_mi

namespace {

// Copies between a CALLER's buffer and HBM, stream-ordered on the lane's private stream and complete on return (staged by
// the runtime for pageable memory, plain DMA for pinned memory).  Measured on a 4K noise frame, buffers reused across
// calls: 2.1 ms encode + 2.1 ms decode with pageable and with pinned buffers alike; what makes the allocating calls
// slower is the first touch of a fresh 30 MB allocation per call, not the copy.
inline hipError_t copy_user(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
    return n ? hipMemcpyWithStream(dst, src, n, kind, s) : hipSuccess;
}

struct LaneLease {  // returns the lane to the cache on every exit path
    HostLane* l = nullptr;
    ~LaneLease() { lane_release(l); }
};

// lane_wait_status behind a codec call that was made on the lane's buffers directly: the 16-byte mailbox copy first
int lane_read_status(HostLane* l) {
    LLMI_HIP_TRY(hipMemcpyAsync(l->h_meta, l->d_meta, 16, hipMemcpyDeviceToHost, l->stream));
    return lane_wait_status(l);
}

// A container on its way into a decode, a region decode or a region update: probed, its shape checked, a LEGACY stream's length clamped
// to what a decoder can read, a lane of its full shape leased and that lane's device current until the call returns.
struct Opened {
    llcomp_mi_info info{};
    size_t len = 0;  // (clamped)
    bool legacy = false;
    LaneLease lease;
    std::optional<DeviceGuard> guard;  // (after the lease: the device is restored before the lane goes back)
    uint64_t payload() const { return len - info.payload_offset; }
};
// header_check(info) runs on the probed header before a lane is taken: what a call refuses or reports from the header alone
template <typename Check>
int open_container(const uint8_t* data, size_t len, int32_t device, uint32_t flags, Opened& o, Check header_check) {
    if (flags & ~LLCOMP_MI_FLAG_SMALL_MODEL) return LLCOMP_MI_BAD_ARGS;
    llcomp_mi_info& info = o.info;
    if (int rc = llcomp_mi_probe(data, len, &info)) return rc;
    o.legacy = info.format == LLCOMP_MI_FORMAT_LEGACY;
    if (int rc = check_shape(info.width, info.height, info.channels, o.legacy)) return rc;
    if (int rc = header_check(info)) return rc;
    const uint64_t raw = uint64_t(info.width) * info.height * info.channels;
    o.len = o.legacy ? size_t(std::min<uint64_t>(len, info.payload_offset + legacy_read_bound(raw))) : len;  // the rest is never read
    if (int rc = lane_acquire(&o.lease.l, device, info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar, o.legacy,
                              o.payload() + 16, o.legacy ? (flags & LLCOMP_MI_FLAG_SMALL_MODEL) != 0 : info.small_model != 0,
                              o.legacy ? o.payload() : 0))
        return rc;
    o.guard.emplace(o.lease.l->k->device);
    return o.guard->ok ? LLCOMP_MI_OK : LLCOMP_MI_HIP_ERROR;
}

// Up goes what a decode of tile box `box` reads and no more: the header + slice table, and the payload span of the covered slices at its
// own offset in the lane's container buffer (the bytes around it are never read)
int stage_covered(HostLane* l, const uint8_t* data, const Opened& o, const uint32_t box[4]) {
    const PayloadSpan s = covered_span(o.info, data, o.len, box);
    LLMI_HIP_TRY(copy_user(l->d_container, data, l->head_bytes, hipMemcpyHostToDevice, l->stream));
    LLMI_HIP_TRY(copy_user(l->d_payload() + s.begin, data + l->head_bytes + s.begin, s.end - s.begin, hipMemcpyHostToDevice, l->stream));
    return lane_set_legacy_len(l, o.payload());
}

// encode into `out` (capacity out_cap) when out != nullptr, else into an allocated buffer returned through *out_alloc (HostOut)
int encode_common(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_opts* opts, uint8_t* out, size_t out_cap,
                  uint8_t** out_alloc, size_t* out_len) {
    *out_len = 0;
    llcomp_mi_opts o{};
    o.struct_size = sizeof(o);
    o.format = LLCOMP_MI_FORMAT_LEGACY;
    o.device = -1;
    if (opts) {  // one layout per ABI version: a caller built against another header is refused, not half-read
        if (opts->struct_size != sizeof(llcomp_mi_opts)) return LLCOMP_MI_BAD_ARGS;
        std::memcpy(&o, opts, sizeof(o));
        if (o.small_model > 1 || o.reserved) return LLCOMP_MI_BAD_ARGS;
        if (o.n_devices && (!o.devices || o.n_devices > LLCOMP_MI_MAX_DEVICES)) return LLCOMP_MI_BAD_ARGS;
    }
    if (o.format != LLCOMP_MI_FORMAT_LEGACY && o.format != LLCOMP_MI_FORMAT_SLICED) return LLCOMP_MI_BAD_ARGS;
    const bool legacy = o.format == LLCOMP_MI_FORMAT_LEGACY;
    if (int rc = check_shape(w, h, c, legacy)) return rc;
    const uint32_t tile_w = legacy ? w : (o.tile_w == 0 || o.tile_w > w ? w : o.tile_w);
    const uint32_t tile_h = legacy ? h : (o.tile_h == 0 || o.tile_h > h ? h : o.tile_h);
    const uint32_t planar = legacy ? 0 : (o.planar ? 1 : 0);
    const uint64_t raw = uint64_t(w) * h * c;
    clear_device_error();
    if (o.n_devices) {
        // a device list: the tile rows are dealt over the devices (multidev.hip).  One serial stream does not shard, and a list of
        // one device is the plain call on that device.
        if (!legacy && o.n_devices > 1)
            return encode_multi(px, w, h, c, tile_w, tile_h, planar, o.small_model != 0, DeviceList{o.devices, o.n_devices, o.chunks_per_device}, out,
                                out_cap, out_alloc, out_len);
        o.device = o.devices[0];
        if (o.device < 0) return LLCOMP_MI_BAD_ARGS;
    }

    LaneLease lease;
    if (int rc = lane_acquire(&lease.l, o.device, w, h, c, tile_w, tile_h, planar, legacy, 0, o.small_model != 0)) return rc;
    HostLane* l = lease.l;
    // room for 2x raw first (incompressible noise needs ~1.25x); lane_encode_sync grows to the proven worst case if it has to
    const uint64_t first_cap = 2 * raw + 64ull * llcomp_mi_slice_count(w, h, c, tile_w, tile_h, planar) + 4096;
    if (int rc = lane_grow(l, std::min(first_cap, llcomp_mi_codec_max_payload_bytes(l->k)))) return rc;
    DeviceGuard guard(l->k->device);
    if (!guard.ok) return LLCOMP_MI_HIP_ERROR;
    LLMI_HIP_TRY(copy_user(l->d_px, px, raw, hipMemcpyHostToDevice, l->stream));
    if (int rc = lane_encode_sync(l)) return rc;
    const size_t n = size_t(l->head_bytes) + size_t(l->h_meta[0]);
    HostOut res(out, out_cap, out_alloc, out_len);
    uint8_t* dst = nullptr;
    if (int rc = res.take(n, dst)) return rc;
    // header, slice table and payload sit in HBM exactly as on the wire (little-endian u32 on both sides): one copy
    LLMI_HIP_TRY(copy_user(dst, l->d_container, n, hipMemcpyDeviceToHost, l->stream));
    res.commit();
    return LLCOMP_MI_OK;
}

int decode_common(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint8_t* px, size_t px_cap, uint8_t** px_alloc,
                  uint32_t* w, uint32_t* h, uint32_t* c) {
    HostOut res(px, px_cap, px_alloc, nullptr);
    uint8_t* dst = nullptr;
    uint64_t raw = 0;
    Opened o;
    if (int rc = open_container(data, len, device, flags, o, [&](const llcomp_mi_info& info) {
            *w = info.width;
            *h = info.height;
            *c = info.channels;
            raw = uint64_t(info.width) * info.height * info.channels;
            return res.take(raw, dst);  // (the dimensions are reported: the caller of an OUTPUT_OVERFLOW can size its buffer)
        }))
        return rc;
    HostLane* l = o.lease.l;
    // the container goes to HBM as it is: the slice table is read where it lies (offset 24, dword aligned)
    LLMI_HIP_TRY(copy_user(l->d_container, data, o.len, hipMemcpyHostToDevice, l->stream));
    if (int rc = lane_enqueue_decode(l, o.payload())) return rc;
    if (int rc = lane_wait_status(l)) return rc;
    LLMI_HIP_TRY(copy_user(dst, l->d_px, raw, hipMemcpyDeviceToHost, l->stream));
    res.commit();
    return LLCOMP_MI_OK;
}

// Region decode (llcomp_mi_decode_region): the lane of the container's full shape, but only what stage_covered sends crosses PCIe, and
// only the rectangle comes back
int decode_region_common(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                         uint8_t* px, size_t px_cap, uint8_t** px_alloc, uint32_t* c) {
    HostOut res(px, px_cap, px_alloc, nullptr);
    uint8_t* dst = nullptr;
    uint32_t box[4], covered = 0;
    uint64_t out = 0;
    Opened o;
    if (int rc = open_container(data, len, device, flags, o, [&](const llcomp_mi_info& info) {
            if (int rc = llcomp_mi_region_plan(info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar, x, y, rw, rh, box, &covered))
                return rc;
            *c = info.channels;
            out = uint64_t(rw) * rh * info.channels;
            return res.take(out, dst);  // (the channel count is reported: the caller of an OUTPUT_OVERFLOW can size its buffer)
        }))
        return rc;
    HostLane* l = o.lease.l;
    if (int rc = stage_covered(l, data, o, box)) return rc;
    if (int rc = llcomp_mi_codec_decode_region(l->k, l->d_payload(), o.payload(), l->d_len(), x, y, rw, rh, l->d_px, l->d_meta + 1, l->stream))
        return rc;
    if (int rc = lane_read_status(l)) return rc;
    LLMI_HIP_TRY(copy_user(dst, l->d_px, out, hipMemcpyDeviceToHost, l->stream));
    res.commit();
    return LLCOMP_MI_OK;
}

// Region update (llcomp_mi_update_region): the lane of the container's full shape.  Up: the rectangle's pixels and -- only when the
// rectangle is not exactly its box's pixels, so that the box has to be decoded -- what stage_covered sends, as for a region decode.
// llcomp_mi_codec_encode_region codes the box; down come {bytes, status}, then the covered slices' new lengths and streams in one copy;
// llcomp_mi_replace_slices assembles the container here.  Nothing else of the container crosses PCIe in either direction.
int update_region_common(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                         const uint8_t* px, uint8_t* out, size_t out_cap, uint8_t** out_alloc, size_t* out_len) {
    uint32_t box[4], covered = 0;
    Opened o;
    if (int rc = open_container(data, len, device, flags, o, [&](const llcomp_mi_info& info) {
            return llcomp_mi_region_plan(info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar, x, y, rw, rh, box, &covered);
        }))
        return rc;
    HostLane* l = o.lease.l;
    const Geometry& g = l->k->g;
    RegionBox b{box[0], box[1], box[2], box[3]};
    Geometry sub;
    if (!region_geometry(g, b, l->k->tune, sub)) return LLCOMP_MI_HIP_ERROR;
    const bool whole = region_is_whole_box(g, sub, b, x, y, rw, rh);
    if (!whole)
        if (int rc = stage_covered(l, data, o, box)) return rc;
    // the rectangle rides in the lane's frame buffer (rw * rh <= w * h); the new slices come back through a block of their own:
    // [u32 lengths][streams], first with room for twice the box's raw bytes, then for the proven worst case
    LLMI_HIP_TRY(copy_user(l->d_px, px, uint64_t(rw) * rh * o.info.channels, hipMemcpyHostToDevice, l->stream));
    const uint64_t table_bytes = (4ull * covered + 15) & ~15ull, max_sub = uint64_t(covered) * g.slice_cap;
    struct Block {
        uint8_t* p = nullptr;
        ~Block() { dev_free(p); }  // (the lane's stream has been drained on every path that gets here with p set)
    } blk;
    if (int rc = with_overflow_retry(std::min<uint64_t>(2 * uint64_t(sub.w) * sub.h * sub.c + 64ull * covered + 4096, max_sub), max_sub, [&](uint64_t cap) {
            dev_free(blk.p);
            blk.p = nullptr;
            if (dev_alloc(reinterpret_cast<void**>(&blk.p), table_bytes + cap + 16) != hipSuccess) {
                blk.p = nullptr;
                return int(LLCOMP_MI_NOMEM);
            }
            int rc = llcomp_mi_codec_encode_region(l->k, whole ? nullptr : l->d_payload(), o.payload(), whole ? nullptr : l->d_len(), x, y, rw, rh,
                                                   l->d_px, blk.p + table_bytes, cap, blk.p, l->d_meta, l->d_meta + 1, l->stream);
            if (!rc) rc = lane_read_status(l);
            if (rc) (void)hipStreamSynchronize(l->stream);  // whatever was queued may still write the block that is about to be freed
            return rc;
        }))
        return rc;
    const uint64_t sub_bytes = l->h_meta[0];
    std::vector<uint8_t> host(size_t(table_bytes + sub_bytes));
    LLMI_HIP_TRY(copy_user(host.data(), blk.p, host.size(), hipMemcpyDeviceToHost, l->stream));
    const uint32_t* new_len = reinterpret_cast<const uint32_t*>(host.data());  // (little-endian hosts, as the table on the wire)
    if (!o.legacy) {
        if (out) return llcomp_mi_replace_slices_into(data, o.len, box, new_len, host.data() + table_bytes, out, out_cap, out_len);
        return llcomp_mi_replace_slices(data, o.len, box, new_len, host.data() + table_bytes, out_alloc, out_len);
    }
    // a LEGACY stream: the 6-byte header and the one new stream
    HostOut res(out, out_cap, out_alloc, out_len);
    uint8_t* dst = nullptr;
    if (int rc = res.take(6 + size_t(sub_bytes), dst)) return rc;
    std::memcpy(dst, data, 6);
    std::memcpy(dst + 6, host.data() + table_bytes, size_t(sub_bytes));
    res.commit();
    return LLCOMP_MI_OK;
}

// decode over a device list: sliced containers whose table fits their payload are dealt over the devices (multidev.hip); a legacy
// stream, a list of one device and damaged containers (the one-device path forms their verdict) go to devices[0]
int decode_devices_common(const uint8_t* data, size_t len, const DeviceList& dl, uint32_t flags, uint8_t* px, size_t px_cap, uint8_t** px_alloc,
                          uint32_t* w, uint32_t* h, uint32_t* c) {
    if (flags & ~LLCOMP_MI_FLAG_SMALL_MODEL) return LLCOMP_MI_BAD_ARGS;
    clear_device_error();
    for (uint32_t i = 0; i < dl.n; ++i)
        if (dl.devices[i] < 0) return LLCOMP_MI_BAD_ARGS;
    llcomp_mi_info info;
    if (int rc = llcomp_mi_probe(data, len, &info)) return rc;
    if (info.format == LLCOMP_MI_FORMAT_SLICED && dl.n > 1) {
        bool handled = false;
        const int rc = decode_multi(data, len, info, dl, px, px_cap, px_alloc, w, h, c, &handled);
        if (handled) return rc;
    }
    return decode_common(data, len, dl.devices[0], flags, px, px_cap, px_alloc, w, h, c);
}

}  // namespace

extern "C" {

int llcomp_mi_encode(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_opts* opts, uint8_t** out, size_t* out_len) {
    if (!px || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    *out = nullptr;
    const int rc = encode_common(px, w, h, c, opts, nullptr, 0, out, out_len);
    if (rc) *out_len = 0;
    return rc;
}

int llcomp_mi_encode_into(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_opts* opts, uint8_t* out,
                          size_t out_cap, size_t* out_len) {
    if (!px || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    return encode_common(px, w, h, c, opts, out, out_cap, nullptr, out_len);
}

int llcomp_mi_decode(const uint8_t* data, size_t len, int32_t device, uint8_t** px, uint32_t* w, uint32_t* h, uint32_t* c) {
    if (!data || !px || !w || !h || !c) return LLCOMP_MI_BAD_ARGS;
    *px = nullptr;
    return decode_common(data, len, device, 0, nullptr, 0, px, w, h, c);
}

int llcomp_mi_decode_flags(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint8_t** px, uint32_t* w, uint32_t* h,
                           uint32_t* c) {
    if (!data || !px || !w || !h || !c) return LLCOMP_MI_BAD_ARGS;
    *px = nullptr;
    return decode_common(data, len, device, flags, nullptr, 0, px, w, h, c);
}

int llcomp_mi_decode_into(const uint8_t* data, size_t len, int32_t device, uint8_t* px, size_t px_cap, uint32_t* w, uint32_t* h,
                          uint32_t* c) {
    return llcomp_mi_decode_into_flags(data, len, device, 0, px, px_cap, w, h, c);
}

int llcomp_mi_decode_into_flags(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint8_t* px, size_t px_cap, uint32_t* w,
                                uint32_t* h, uint32_t* c) {
    if (!data || !px || !w || !h || !c || (flags & ~LLCOMP_MI_FLAG_SMALL_MODEL)) return LLCOMP_MI_BAD_ARGS;
    return decode_common(data, len, device, flags, px, px_cap, nullptr, w, h, c);
}

int llcomp_mi_decode_devices(const uint8_t* data, size_t len, const int32_t* devices, uint32_t n_devices, uint32_t chunks_per_device,
                             uint32_t flags, uint8_t** px, uint32_t* w, uint32_t* h, uint32_t* c) {
    if (!data || !px || !w || !h || !c || !devices || !n_devices || n_devices > LLCOMP_MI_MAX_DEVICES) return LLCOMP_MI_BAD_ARGS;
    *px = nullptr;
    return decode_devices_common(data, len, DeviceList{devices, n_devices, chunks_per_device}, flags, nullptr, 0, px, w, h, c);
}

int llcomp_mi_decode_into_devices(const uint8_t* data, size_t len, const int32_t* devices, uint32_t n_devices, uint32_t chunks_per_device,
                                  uint32_t flags, uint8_t* px, size_t px_cap, uint32_t* w, uint32_t* h, uint32_t* c) {
    if (!data || !px || !w || !h || !c || !devices || !n_devices || n_devices > LLCOMP_MI_MAX_DEVICES) return LLCOMP_MI_BAD_ARGS;
    return decode_devices_common(data, len, DeviceList{devices, n_devices, chunks_per_device}, flags, px, px_cap, nullptr, w, h, c);
}

int llcomp_mi_decode_region(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                            uint32_t rh, uint8_t** px, uint32_t* c) {
    if (!data || !px || !c) return LLCOMP_MI_BAD_ARGS;
    *px = nullptr;
    return decode_region_common(data, len, device, flags, x, y, rw, rh, nullptr, 0, px, c);
}

int llcomp_mi_decode_region_into(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                                 uint32_t rh, uint8_t* px, size_t px_cap, uint32_t* c) {
    if (!data || !px || !c) return LLCOMP_MI_BAD_ARGS;
    return decode_region_common(data, len, device, flags, x, y, rw, rh, px, px_cap, nullptr, c);
}

int llcomp_mi_update_region(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                            const uint8_t* px, uint8_t** out, size_t* out_len) {
    if (!data || !px || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    uint8_t* o = nullptr;
    size_t n = 0;
    if (int rc = update_region_common(data, len, device, flags, x, y, rw, rh, px, nullptr, 0, &o, &n)) return rc;
    *out = o;
    *out_len = n;
    return LLCOMP_MI_OK;
}

int llcomp_mi_update_region_into(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                                 uint32_t rh, const uint8_t* px, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!data || !px || !out || !out_len) return LLCOMP_MI_BAD_ARGS;
    return update_region_common(data, len, device, flags, x, y, rw, rh, px, out, out_cap, nullptr, out_len);
}

void llcomp_mi_trim(void) {
    drop_idle_lanes(lane_cache());
    dev_release_idle();
}

void llcomp_mi_set_pool_limit(uint64_t bytes_per_device) { dev_set_limit(bytes_per_device); }
uint64_t llcomp_mi_pool_limit(void) { return dev_limit(); }
uint64_t llcomp_mi_pool_idle_bytes(void) { return dev_idle_bytes(); }

void* llcomp_mi_host_alloc(size_t bytes) {
    // portable: a buffer from here is handed to EVERY device of a device list (multidev.hip: each GPU copies its rows / its payload
    // straight out of / into the caller's buffer), not only to the device that was current when it was allocated
    void* p = nullptr;
    if (host_alloc_pinned(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return nullptr;
    return p;
}

void llcomp_mi_host_free(void* p) {
    if (p) (void)host_free_pinned(p);
}

}  // extern "C"
