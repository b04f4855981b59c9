/* llcomp_mi.h -- C ABI of the MI355X-native llcomp coding path (libllcomp_mi.so).
 *
 * The reference (vovach777/llcomp) is a header-only C++ library with exactly two entry points and no
 * FFI of its own; this header is the boundary a maintainer would bind instead of them:
 *
 *   llcomp::compressImage(const std::vector<uint8_t>& rgb, int w, int h, int channels)
 *        -> std::vector<uint8_t>                         /root/reference/llcomp.hpp:358
 *   llcomp::decompressImage(const std::vector<uint8_t>& data) -> RawImage{pixels,width,height,channels}
 *                                                        /root/reference/llcomp.hpp:454-461
 *   callers: llcompc.cpp:33, llcompd.cpp:26
 *
 * Everything here is plain C: pointers, sizes, integer status codes.  No torch, no C++ types.
 * All compute runs in hand-written HIP kernels for gfx950; there is NO CPU code path behind these
 * calls -- without a HIP device they return LLCOMP_MI_NO_DEVICE.
 * include/llcomp_mi.hpp layers the reference's own C++ signatures on top; INTEGRATION.md shows the
 * binding.
 */
#ifndef LLCOMP_MI_H
#define LLCOMP_MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 4 (round 6: device lists -- llcomp_mi_opts.devices, llcomp_mi_decode_devices, llcomp_mi_stream_create_multi,
 * llcomp_mi_plan_chunks, llcomp_mi_codec_get_counters; later, functions only: region decode -- llcomp_mi_region_plan,
 * llcomp_mi_decode_region(_into), llcomp_mi_codec_decode_region, llcomp_mi_codec_region_family, LLCOMP_MI_PREPARE_REGION; a rectangle
 * per frame -- llcomp_mi_regions_plan, llcomp_mi_codec_decode_regions, llcomp_mi_codec_regions_family, LLCOMP_MI_PREPARE_REGIONS; crops
 * of host containers -- llcomp_mi_regions_gather, llcomp_mi_codec_decode_regions_host, llcomp_mi_stream_submit_decode_regions,
 * LLCOMP_MI_JOB_DECODE_REGIONS, LLCOMP_MI_CTR_HOST_STAGED_BYTES; crops of different sizes resized to one shape -- llcomp_mi_resize_weights,
 * llcomp_mi_resize_filter_weights (PIL's filters, one per frame through bits 4-6 of the flags),
 * llcomp_mi_resized_regions_plan, llcomp_mi_codec_decode_resized_regions(_host), llcomp_mi_stream_submit_decode_resized_regions,
 * LLCOMP_MI_PREPARE_RESIZED, LLCOMP_MI_JOB_DECODE_RESIZED_REGIONS, llcomp_mi_codec_allocated_bytes; their output as a model takes it,
 * float or normalised, CHW or HWC -- llcomp_mi_output_format, llcomp_mi_output_table and the _ex forms of the three resized calls; region
 * update -- llcomp_mi_replace_slices(_into), llcomp_mi_update_region(_into), llcomp_mi_codec_encode_region,
 * llcomp_mi_codec_update_region, LLCOMP_MI_PREPARE_UPDATE; several views of each frame, each frame decoded once -- llcomp_mi_view,
 * llcomp_mi_view_group, llcomp_mi_views_plan, llcomp_mi_codec_decode_views(_host), llcomp_mi_codec_views_workspace_bytes,
 * LLCOMP_MI_PREPARE_VIEWS; crops that leave the image -- llcomp_mi_pad, llcomp_mi_pad_axis, llcomp_mi_padded_filter_weights,
 * llcomp_mi_padded_regions_plan, llcomp_mi_codec_decode_padded_regions(_host), llcomp_mi_codec_decode_padded_views(_host),
 * llcomp_mi_codec_padded_workspace_bytes, LLCOMP_MI_CTR_BIAS_LAUNCHES).  The library and its callers are built from ONE header: structs have one layout per ABI version (llcomp_mi_opts is
 * checked through struct_size and refused when it differs; llcomp_mi_info and llcomp_mi_stream_result are written in full),
 * so a binding compares llcomp_mi_abi_version() with the LLCOMP_MI_ABI_VERSION it was generated from and refuses to run on
 * a mismatch -- there is no cross-version compatibility mode. */
#define LLCOMP_MI_ABI_VERSION 4

/* Wire formats.  LEGACY is the reference's own: [0x79][channels u8][width u16 LE][height u16 LE] + ONE
 * range-coded stream (llcomp.hpp:375-378); it is a single serial chain (one GPU lane).  SLICED is this
 * project's container: independent slices, each a bare reference-compatible stream with fresh state:
 *   [0x9C][ver=1][channels][flags bit0=planar, bit1=small model] [w u32][h u32][tile_w u32][tile_h u32][n_slices u32]
 *   [len u32] x n_slices  [payload bytes ...]                                  (all little-endian)
 * "Small model" = the bitstream of a reference built with `LargeModel = false` (llcomp.hpp:21, 26-32, 427-429: the two
 * quant5 terms are left out of the context).  The reference's header does not record that build option (the magic
 * stays 0x79), so for the LEGACY format the caller has to say so on both sides; the SLICED header carries a flag. */
#define LLCOMP_MI_MAGIC_LEGACY 0x79
#define LLCOMP_MI_MAGIC_SLICED 0x9C
#define LLCOMP_MI_SLICED_HEADER_BYTES 24

typedef enum llcomp_mi_status {
    LLCOMP_MI_OK = 0,
    LLCOMP_MI_BAD_MAGIC = 1,       /* reference throws "Invalid magic number"  (llcomp.hpp:465-467) */
    LLCOMP_MI_BAD_EXPONENT = 2,    /* reference throws "Invalid exponent"      (llcomp.hpp:232-234) */
    LLCOMP_MI_TRUNCATED = 3,       /* header or slice table longer than the data (reference: UB, D5), or a SLICED table entry longer
                                      than no encoder writes: 13 * n + 16 bytes rounded up to a multiple of 16, n = samples of a full
                                      tile (tile_w * tile_h * (planar ? 1 : c)).  A LEGACY stream has no such limit: bytes beyond the
                                      65 * w * h * c + 2 a decoder can read are ignored, as the reference ignores them. */
    LLCOMP_MI_BAD_ARGS = 4,        /* null pointers, zero sizes, unsupported channel count, bad opts */
    LLCOMP_MI_OUT_OF_RANGE = 5,    /* legacy format with w or h > 65535, or w*h*c >= 2^31 (reference: silent truncation, D4) */
    LLCOMP_MI_OUTPUT_OVERFLOW = 6, /* caller-provided output capacity too small (reference: heap overflow, D1) */
    LLCOMP_MI_HIP_ERROR = 7,       /* a HIP call failed, or a kernel found its own launch assumptions violated and refused to run */
    LLCOMP_MI_NO_DEVICE = 8,
    LLCOMP_MI_NOMEM = 9,           /* An allocation of device or pinned memory failed.  The contract, for EVERY call that can return it: it
                                      is returned before anything is queued on the caller's stream and before an output or the status
                                      word is written (as BAD_ARGS is); the object the call was made on stays usable -- what it already
                                      held it still holds or has given back whole, and the same call succeeds once the memory is there;
                                      llcomp_mi_codec_allocated_bytes stays true; nothing leaks.  A buffer that had to grow may have been
                                      given back before its replacement was refused: the codec then holds less, never something half set
                                      up.  The host-buffer calls (llcomp_mi_encode, _decode, _decode_region, _update_region and their
                                      _into forms) work on a lane of the library's own: they may have copied the caller's INPUT into the
                                      lane's buffers by then, and the caller's output buffer is untouched.  Two allocations are optional
                                      and never fail a call: the 2-D decoder's 16-byte feedback mailbox (without it the bank cache stays
                                      on in every launch) and the events of the chunked encoder's second stream (without them the pass
                                      runs in order on the caller's stream); the bytes are the same. */
    LLCOMP_MI_BUSY = 10,           /* streaming pipeline: every slot is occupied / the oldest job is still in flight */
    LLCOMP_MI_DEVICE_FAILED = 11   /* a call over a device list: one of the devices failed (HIP error, out of memory, no such device) and
                                      nothing was published; llcomp_mi_last_device_error tells which one and why.  Verdicts about the
                                      DATA (BAD_EXPONENT, TRUNCATED, OUTPUT_OVERFLOW) come back as themselves from any device, and so
                                      does NO_DEVICE (a machine without any HIP device: no member of the list to blame). */
} llcomp_mi_status;

typedef enum llcomp_mi_format { LLCOMP_MI_FORMAT_LEGACY = 0, LLCOMP_MI_FORMAT_SLICED = 1 } llcomp_mi_format;

typedef struct llcomp_mi_opts {
    uint32_t struct_size; /* = sizeof(llcomp_mi_opts) */
    uint32_t format;      /* llcomp_mi_format */
    uint32_t tile_w;      /* slice width  in pixels, 0 = full width   (SLICED only) */
    uint32_t tile_h;      /* slice height in pixels, 0 = full height  (SLICED only) */
    uint32_t planar;      /* 1 = one slice per colour-transformed channel plane, 0 = channels interleaved */
    int32_t device;       /* HIP device ordinal, -1 = current device */
    uint32_t small_model; /* 1 = code like a reference built with LargeModel = false */
    /* One image over several GPUs, in this process (BASELINE config 4; SURVEY 8b "device list").  n_devices == 0: one device
     * (`device`).  n_devices >= 1 (SLICED only; at most LLCOMP_MI_MAX_DEVICES): the image's tile rows are dealt in chunks
     * round-robin over devices[0..n_devices) (llcomp_mi_plan_chunks), every device gets ONLY its rows over its own PCIe link,
     * codes them with its own lane and copies its payload straight to its place in the container -- there is no exchange between
     * the GPUs and no collective, and the container is byte-identical to the one-device container.  An ordinal may repeat (two
     * lanes on one GPU: how the path is tested on a one-GPU box).  A LEGACY stream is one serial chain and does not shard:
     * devices[0] codes it.  `device` is ignored when n_devices > 0. */
    uint32_t n_devices;
    const int32_t* devices;
    uint32_t chunks_per_device; /* chunks of tile rows per device (0 = 4): finer chunks balance content whose cost varies over the image */
    uint32_t reserved;          /* 0 */
} llcomp_mi_opts;
#define LLCOMP_MI_MAX_DEVICES 64
#define LLCOMP_MI_FLAG_SMALL_MODEL 1u /* llcomp_mi_decode_flags / llcomp_mi_codec_create_ex */

/* ---- host-buffer API: drop-in for compressImage / decompressImage ------------------------------------ */
/* px: h*w*c bytes, row-major, channels interleaved (exactly the reference's `rgb` vector).  opts==NULL means
 * LEGACY on the current device.  *out is allocated by the library; release with llcomp_mi_free. */
int llcomp_mi_encode(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_opts* opts,
                     uint8_t** out, size_t* out_len);
/* Accepts either wire format (dispatch on the magic byte).  *px allocated by the library. */
int llcomp_mi_decode(const uint8_t* data, size_t len, int32_t device, uint8_t** px, uint32_t* w, uint32_t* h,
                     uint32_t* c);
/* The same with flags: LLCOMP_MI_FLAG_SMALL_MODEL = a LEGACY stream that was written with the small model (a SLICED
 * container says so itself; the flag is ignored for it). */
int llcomp_mi_decode_flags(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint8_t** px, uint32_t* w,
                           uint32_t* h, uint32_t* c);
void llcomp_mi_free(void* p);
/* Region decode: the rectangle (x, y, rw, rh) of the picture, rw >= 1, rh >= 1, x + rw <= w, y + rh <= h (checked in 64 bits;
 * anything else is BAD_ARGS), as rh x rw x c bytes, row-major, channels interleaved -- the same bytes as that rectangle of the full
 * decode.  Only the slices of the tiles the rectangle touches are read, copied to the GPU and decoded (llcomp_mi_region_plan): the
 * header and slice table cross PCIe, then the payload bytes from the first covered slice's first byte to the last one's end, and
 * only rw * rh * c bytes come back.  A LEGACY stream, and a container of one tile, is one serial chain: it is decoded whole and
 * cropped on the GPU.  BAD_EXPONENT and TRUNCATED come from covered slices only (a covered slice whose bytes run past the data is
 * TRUNCATED); a region decode does NOT validate the container -- damage in slices outside the rectangle is never seen.  A header or
 * slice table that is cut short fails as in llcomp_mi_probe.  flags: LLCOMP_MI_FLAG_SMALL_MODEL as in llcomp_mi_decode_flags.  *c
 * reports the channel count.  One device only: there is no region decode over a device list.  Crops of many containers at once:
 * llcomp_mi_codec_decode_regions_host (into HBM) and llcomp_mi_stream_submit_decode_regions (host to host). */
int llcomp_mi_decode_region(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                            uint32_t rh, uint8_t** px, uint32_t* c);
/* ... into a caller's buffer: OUTPUT_OVERFLOW (with *c set, nothing written) when px_cap < rw * rh * c. */
int llcomp_mi_decode_region_into(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                                 uint32_t rh, uint8_t* px, size_t px_cap, uint32_t* c);
/* Region update, the write side of llcomp_mi_decode_region: the rectangle (x, y, rw, rh) of the picture (the same rule; anything else
 * is BAD_ARGS) is replaced by px (rh x rw x c bytes, row-major, channels interleaved; c = the container's channel count), and *out is
 * the container a full encode of the modified picture gives, byte for byte, in the container's own format, tiling and model.  Only the
 * slices of the tiles the rectangle touches are coded again (llcomp_mi_codec_encode_region), and only their bytes cross PCIe: the
 * header and slice table and rw * rh * c bytes of pixels go up; when the rectangle is not exactly its box's pixels (tile-aligned, or
 * reaching the image edge) the covered slices' payload span goes up too, to be decoded and pasted into; the new lengths and streams of
 * the covered slices come down, and llcomp_mi_replace_slices assembles the result on the host.  BAD_EXPONENT and TRUNCATED come from
 * the covered slices when they had to be decoded, and never otherwise: with an aligned rectangle the old covered slices are not read
 * at all.  Damage in slices outside the box is never seen and is carried over verbatim; an uncovered slice whose bytes run past the data
 * is TRUNCATED.  A LEGACY stream is one serial chain: unless the rectangle is the whole picture it is decoded whole, pasted into and
 * encoded whole, and the result is a LEGACY stream again.  flags as in llcomp_mi_decode_region.  On any error *out is untouched (_into:
 * the buffer; OUTPUT_OVERFLOW with *out_len = the size it takes when out_cap is too small).  One device only. */
int llcomp_mi_update_region(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                            uint32_t rh, const uint8_t* px, uint8_t** out, size_t* out_len);
int llcomp_mi_update_region_into(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint32_t x, uint32_t y, uint32_t rw,
                                 uint32_t rh, const uint8_t* px, uint8_t* out, size_t out_cap, size_t* out_len);
/* Decoding over a device list: the mirror image of llcomp_mi_opts.devices -- every device receives the table entries and payload
 * bytes of its chunks of tile rows, decodes them and copies its rows straight to their place in the picture.  Nothing is written to
 * the output before EVERY device has reported success (the first failing device in list order decides the status).  How the
 * container was encoded (one device or many, which chunking) does not matter.  A LEGACY stream goes to devices[0]; so does a
 * container whose slice table does not fit its payload (the one-device path forms the verdict for damaged input).
 * n_devices == 0 or devices == NULL: BAD_ARGS.  chunks_per_device: 0 = 4. */
int llcomp_mi_decode_devices(const uint8_t* data, size_t len, const int32_t* devices, uint32_t n_devices, uint32_t chunks_per_device,
                             uint32_t flags, uint8_t** px, uint32_t* w, uint32_t* h, uint32_t* c);
int llcomp_mi_decode_into_devices(const uint8_t* data, size_t len, const int32_t* devices, uint32_t n_devices, uint32_t chunks_per_device,
                                  uint32_t flags, uint8_t* px, size_t px_cap, uint32_t* w, uint32_t* h, uint32_t* c);
/* After a call of THIS thread returned LLCOMP_MI_DEVICE_FAILED: the HIP ordinal that failed, its position in the device list and the
 * status it reported (HIP_ERROR, NOMEM, NO_DEVICE, BAD_ARGS for an ordinal that does not exist).  Returns 0 and leaves the outputs
 * alone when the thread's last device-list call did not fail that way.  Any pointer may be NULL. */
int llcomp_mi_last_device_error(int32_t* device, uint32_t* index, int* status);
/* The same two calls with CALLER-PROVIDED output buffers (nothing is allocated for the caller).  If the capacity is too
 * small they return LLCOMP_MI_OUTPUT_OVERFLOW and report what it takes (*out_len; *w,*h,*c), and nothing is written.
 * Every host-buffer call works on a private HIP stream (never the NULL stream); with input and output buffers from
 * llcomp_mi_host_alloc (pinned memory) the PCIe copies are plain DMA, pageable buffers are staged by the HIP runtime. */
int llcomp_mi_encode_into(const uint8_t* px, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_opts* opts, uint8_t* out,
                          size_t out_cap, size_t* out_len);
int llcomp_mi_decode_into(const uint8_t* data, size_t len, int32_t device, uint8_t* px, size_t px_cap, uint32_t* w,
                          uint32_t* h, uint32_t* c);
/* ... with flags, as llcomp_mi_decode_flags (a LEGACY stream written with the small model) */
int llcomp_mi_decode_into_flags(const uint8_t* data, size_t len, int32_t device, uint32_t flags, uint8_t* px, size_t px_cap,
                                uint32_t* w, uint32_t* h, uint32_t* c);
/* The host-buffer calls keep a few idle coding lanes (GBs of HBM workspace for a 4K frame) for the next call of the same
 * shape, and the library parks the device memory of destroyed codecs / streams / lanes for reuse instead of returning it
 * to the driver (up to the pool limit per device; released by itself when an allocation OF THE LIBRARY fails).  This
 * releases both.  Codec and stream objects in use are not touched.  A process that shares the GPU with another allocator
 * (PyTorch's caching allocator, say) calls this when that allocator reports out-of-memory. */
void llcomp_mi_trim(void);
/* Parked device memory allowed PER DEVICE (default 16 GiB, or the environment's LLCOMP_MI_POOL_MAX_BYTES read once);
 * blocks beyond it go back to the driver, largest first.  0 = park nothing: every release is a hipFree. */
void llcomp_mi_set_pool_limit(uint64_t bytes_per_device);
uint64_t llcomp_mi_pool_limit(void);
uint64_t llcomp_mi_pool_idle_bytes(void); /* bytes parked right now, all devices */
void* llcomp_mi_host_alloc(size_t bytes); /* pinned host memory, NULL on failure */
void llcomp_mi_host_free(void* p);
const char* llcomp_mi_strerror(int status);
int llcomp_mi_abi_version(void);
/* Test / tuning hooks (LLCOMP_MI_LPW, _LANE_SHIFT, _NOROWS, _NOLDSTAB, _NOSNAP, _NOCACHE, _NOFEEDBACK, _OVERLAP, _FORCE_REPLAY; none
 * changes an output byte) are
 * read from the environment once per process; a test that changes them calls this to have them read again. */
void llcomp_mi_reload_tuning(void);
/* Number of usable HIP devices (0 when there is none; never fails). */
int llcomp_mi_device_count(void);

/* ---- host-side container tools (no GPU involved) ------------------------------------------------------ */
typedef struct llcomp_mi_info {
    uint32_t format, channels, width, height, tile_w, tile_h, planar, n_slices;
    uint64_t table_offset;   /* byte offset of the slice length table (0 for LEGACY) */
    uint64_t payload_offset; /* byte offset of the first payload byte */
    uint32_t small_model;    /* SLICED: the header's small-model flag; LEGACY: always 0 (not recorded in that header) */
    uint32_t reserved;
} llcomp_mi_info;
int llcomp_mi_probe(const uint8_t* data, size_t len, llcomp_mi_info* info);
/* The tiles a rectangle (x, y, rw, rh) of one frame covers: box = {tx0, ty0, tx1, ty1} (tile columns [tx0, tx1), tile rows
 * [ty0, ty1)), *slices_per_frame = the covered slices of one frame ((tx1 - tx0) * (ty1 - ty0), times c for planar slices).  tile_w /
 * tile_h 0 = the whole width / height.  BAD_ARGS for an empty rectangle or one outside the image (see llcomp_mi_decode_region).
 * Host-only: no GPU involved.  Every region call plans with this. */
int llcomp_mi_region_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t x, uint32_t y,
                          uint32_t rw, uint32_t rh, uint32_t box[4], uint32_t* slices_per_frame);
/* A rectangle of one size (rw, rh) at an offset of its own in each of n frames: xy = {x_0, y_0, x_1, y_1, ...} (2 * n).  To decode
 * every frame on ONE sub-geometry, frame f decodes a WINDOW of tiles of a fixed size that contains its covered box:
 *   Wx = min(ntx, (rw + tile_w - 2) / tile_w + 1)  -- the most tile columns a rectangle of width rw can touch --
 *   wx0_f = min(x_f / tile_w, ntx - Wx), and the same in y (tile_w / tile_h 0 = the whole width / height, as in llcomp_mi_region_plan).
 * windows (4 * n, NULL ok) = {wx0, wy0, wx1, wy1} per frame (tile columns [wx0, wx1), tile rows [wy0, wy1)).  A window that holds the
 * partial last tile column (row) is narrower (lower) in pixels, so the frames fall into at most 2 x 2 classes -- "the window ends at a
 * partial last tile column: yes / no" x the same for rows; the x split exists only when w % tile_w != 0, the y split only when
 * h % tile_h != 0 -- and *n_classes = the number of classes that have frames.  A decode runs one launch chain per class.  BAD_ARGS for
 * n = 0, a NULL xy or n_classes, or any rectangle outside the image.  Host-only; every regions call plans with this rule. */
int llcomp_mi_regions_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t rw, uint32_t rh,
                           const uint32_t* xy, uint32_t n, uint32_t* windows, uint32_t* n_classes);
/* The bytes a regions decode of n single-frame SLICED containers (data[f], lens[f]; one shape, tiling, planar setting and model) needs:
 * the table entries and payload bytes of every frame's window (llcomp_mi_regions_plan) and nothing else.  slice_len (room for len_cap
 * entries) gets the windows' table entries verbatim, payload (room for payload_cap bytes) the same slices' bytes back to back, both in
 * one order: class by class (class 0..3), frame order inside a class, and inside a frame tile row, tile column, plane.  A window's tile
 * row is one run of consecutive slices of its container, so this is one memcpy per window tile row and frame.  *payload_bytes,
 * *n_slices (entries) and *n_classes are always set (0 on an error); payload == NULL or slice_len == NULL only reports them, and a
 * capacity too small is OUTPUT_OVERFLOW with nothing written.  Errors, all decided before anything is written: BAD_ARGS for n = 0, a
 * NULL pointer among data / lens / xy / the three counts, a LEGACY stream, a container that differs from container 0, or any rectangle
 * outside the image; a header or table cut short fails as in llcomp_mi_probe; TRUNCATED for a window slice whose bytes run past its
 * container or whose table entry is above the SLICED limit (LLCOMP_MI_TRUNCATED).  Damage outside every window is never seen.
 * Host-only: no GPU involved. */
int llcomp_mi_regions_gather(const uint8_t* const* data, const size_t* lens, uint32_t n, const uint32_t* xy, uint32_t rw, uint32_t rh,
                             uint8_t* payload, uint64_t payload_cap, uint32_t* slice_len, uint32_t len_cap, uint64_t* payload_bytes,
                             uint32_t* n_slices, uint32_t* n_classes);
/* Splice of a SLICED container: the slices of the tiles box = {tx0, ty0, tx1, ty1} covers (as llcomp_mi_region_plan returns it) are
 * replaced, every other slice stays byte for byte where it was in the payload's order.  new_len = the covered slices' new lengths,
 * u32[covered]; new_payload = their streams back to back; both in sub-slice order: tile row, tile column, plane.  The result has the
 * same header, the new table, the unchanged runs of the old payload (one memcpy each) and the new slices in between.  Because every
 * slice is the reference stream of its own crop, new slices that are the streams of the modified crops make the result the container
 * a full encode of the modified picture gives, byte for byte.  Old covered slices are never read: they may be damaged.  Errors, all
 * decided before anything is written (*out and the _into buffer stay untouched): BAD_ARGS for a NULL pointer, a LEGACY stream, an empty
 * box or one outside the tile grid; a header or table cut short fails as in llcomp_mi_probe; TRUNCATED for a new length above the SLICED
 * limit (LLCOMP_MI_TRUNCATED) or an uncovered slice whose bytes run past the data; _into: OUTPUT_OVERFLOW for a buffer too small, with
 * *out_len = the size it takes.  Bytes of `data` behind the last slice are dropped.  Host-only: no GPU involved. */
int llcomp_mi_replace_slices(const uint8_t* data, size_t len, const uint32_t box[4], const uint32_t* new_len, const uint8_t* new_payload,
                             uint8_t** out, size_t* out_len);
int llcomp_mi_replace_slices_into(const uint8_t* data, size_t len, const uint32_t box[4], const uint32_t* new_len, const uint8_t* new_payload,
                                  uint8_t* out, size_t out_cap, size_t* out_len);
/* The resampling rule of llcomp_mi_codec_decode_resized_regions for one axis, in_len -> out_len, under one of PIL's filters: the rule of
 * PIL's 8-bit resampler (Image.resize of a crop), in integers.  With the filter's kernel function f and radius S:
 *   scale = in_len / out_len, fs = max(scale, 1), support = S * fs, ss = 1 / fs (double); output i: center = (i + 0.5) * scale,
 *   lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), in_len),
 *   w_j = f((lo + j - center + 0.5) * ss) for j in [0, hi - lo), divided by their sum when it is not 0,
 *   q_j = int(w_j * 2^22 + 0.5) for w_j >= 0, int(w_j * 2^22 - 0.5) for w_j < 0, both truncating toward zero (Q22);
 *   out = clamp((sum_j q_j * in[lo + j] + 2^21) >> 22, 0, 255).
 * A frame is resampled horizontally first, rounded to u8, then vertically.  The filters:
 *   BILINEAR  S = 1    f(x) = max(0, 1 - |x|)  (the triangle; also torch's interpolate(mode="bilinear", antialias=True))
 *   BOX       S = 0.5  f(x) = 1 for -0.5 < x <= 0.5, else 0
 *   HAMMING   S = 1    f(0) = 1, f(x) = 0 for |x| >= 1, else sin(pi x) / (pi x) * (0.54 + 0.46 * cos(pi x))
 *   BICUBIC   S = 2    a = -0.5: ((a + 2)|x| - (a + 3)) x^2 + 1 for |x| < 1, (((|x| - 5)|x| + 8)|x| - 4) a for |x| < 2, else 0
 *   LANCZOS   S = 3    sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, sinc(x) = sin(pi x) / (pi x)
 *   NEAREST   one tap of 2^22 at lo_i = ((2 i + 1) * in_len) div (2 * out_len), in exact integers (K = 1): floor((i + 0.5) * in / out)
 *             without rounding error, torch's "nearest-exact" -- the filter for label images, it invents no value
 * in_len == out_len is the identity for every filter (one weight 2^22 at lo <= i).  Only BICUBIC and LANCZOS have negative weights; the
 * sum of |q_j| * 255 stays below 2^31.  Returns K, the taps per output (trailing taps that are 0 for every output are left out; K <= 129),
 * and, when lo / q are not NULL, fills lo[out_len] and q[out_len][K] (zero-padded).  0 for in_len or out_len 0, an unknown filter, or a
 * downscale above the filter's limit: R * in_len > 64 * out_len with R = 1 (64x), but 2 for BICUBIC (32x) and 3 for LANCZOS (21.33x).
 * Host-only; the GPU runs exactly these weights.  llcomp_mi_resize_weights is filter 0, BILINEAR. */
enum {
    LLCOMP_MI_FILTER_BILINEAR = 0,
    LLCOMP_MI_FILTER_NEAREST = 1,
    LLCOMP_MI_FILTER_BOX = 2,
    LLCOMP_MI_FILTER_HAMMING = 3,
    LLCOMP_MI_FILTER_BICUBIC = 4,
    LLCOMP_MI_FILTER_LANCZOS = 5
};
uint32_t llcomp_mi_resize_filter_weights(uint32_t filter, uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q);
/* The per-frame flags byte of the resized calls: bit 0 mirrors the frame's output horizontally, bits 4-6 hold the frame's filter code
 * (0 = BILINEAR, so a flags byte of 0 or 1 and a NULL flags mean what they always meant; codes 6 and 7 are BAD_ARGS); bits 1-3 and 7 are
 * ignored. */
#define LLCOMP_MI_FLAG_MIRROR 1u
#define LLCOMP_MI_FLAG_FILTER_SHIFT 4
#define LLCOMP_MI_FLAG_FILTER_MASK 0x70u
#define LLCOMP_MI_FLAG_FILTER(code) (((code) << LLCOMP_MI_FLAG_FILTER_SHIFT) & LLCOMP_MI_FLAG_FILTER_MASK)
#define LLCOMP_MI_FLAG_FILTER_OF(flags) (((flags) & LLCOMP_MI_FLAG_FILTER_MASK) >> LLCOMP_MI_FLAG_FILTER_SHIFT)
uint32_t llcomp_mi_resize_weights(uint32_t in_len, uint32_t out_len, uint32_t* lo, int32_t* q);
/* The windows of a rectangle of its own size per frame: rects = {x_0, y_0, rw_0, rh_0, x_1, ...} (4 * n).  The rule of
 * llcomp_mi_regions_plan, sized by the batch's LARGEST rectangle: Wx from max_f rw_f, wx0_f = min(x_f / tile_w, ntx - Wx), the same in
 * y, so every window has one tile count and contains its frame's rectangle; the 2 x 2 class rule is unchanged.  With every rectangle of
 * one size this is llcomp_mi_regions_plan window for window.  A frame with a small rectangle decodes a window sized for the largest one.
 * windows (4 * n, NULL ok) and *n_classes as in llcomp_mi_regions_plan.  BAD_ARGS for n = 0, a NULL rects or n_classes, or any rectangle
 * empty or outside the image.  Host-only. */
int llcomp_mi_resized_regions_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, const uint32_t* rects,
                                   uint32_t n, uint32_t* windows, uint32_t* n_classes);
/* The output of a resized regions decode as a model takes it (the _ex calls below): the element type, the layout, and torchvision's
 * ToTensor() + Normalize(mean, std).  The rule, for the u8 value v the u8 call writes for output pixel (f, y, x) and channel ch (the
 * mirror included), in IEEE binary32 with no fused operations, in this order:
 *   t = (float)v;  if scale: t = t / 255.0f (a division);  if mean: t = t - mean[ch];  if std: t = t / std[ch];
 *   F32: t;  F16 / BF16: t rounded to nearest even (overflow to +-inf);  U8: v.
 * Normalisation comes after the u8 rounding of the resample.  v takes 256 values: the rule is a table of c x 256 entries, which
 * llcomp_mi_output_table states and the GPU only looks up.  A NULL format is U8 HWC: the u8 call's bytes. */
enum { LLCOMP_MI_DTYPE_U8 = 0, LLCOMP_MI_DTYPE_F32 = 1, LLCOMP_MI_DTYPE_F16 = 2, LLCOMP_MI_DTYPE_BF16 = 3 };
enum { LLCOMP_MI_LAYOUT_HWC = 0, LLCOMP_MI_LAYOUT_CHW = 1 };
typedef struct llcomp_mi_output_format {
    uint32_t struct_size; /* sizeof(llcomp_mi_output_format) (at least) */
    uint32_t dtype;       /* LLCOMP_MI_DTYPE_* */
    uint32_t layout;      /* HWC: [frames][oh][ow][c]; CHW: [frames][c][oh][ow] */
    uint32_t scale;       /* 1: divide by 255 first (float dtypes only) */
    const float* mean;    /* c values or NULL; read during the call only */
    const float* std;     /* c values or NULL; read during the call only */
} llcomp_mi_output_format; /* 32 bytes on LP64 */
/* The rule above as a table: table[ch * 256 + v] for ch < c, elements of the dtype's size (1, 2 or 4 bytes; F16 / BF16 as their bit
 * patterns).  BAD_ARGS for a NULL fmt or table, c = 0 or above 255, a struct_size below the struct's, an unknown dtype or layout, a scale
 * above 1, U8 with scale, mean or std set, a mean that is not finite, a std that is 0 or not finite.  Host-only. */
int llcomp_mi_output_table(const llcomp_mi_output_format* fmt, uint32_t c, void* table);
/* Several views of each frame in one call (llcomp_mi_codec_decode_views below; multi-crop and two-view training).  A VIEW is a rectangle
 * of one frame with the per-frame flags byte of the resized calls (bit 0 mirror, bits 4-6 the filter); a VIEW GROUP is a list of views
 * that share one output: ow x oh, an output format (NULL = U8 HWC) and a device pointer, written dense in view order as
 * [n_views][oh][ow][c] (CHW: [n_views][c][oh][ow]).  A frame may have any number of views across the groups of a call, including none. */
typedef struct llcomp_mi_view {
    uint32_t frame;        /* the frame of the batch the view is cut from */
    uint32_t x, y, rw, rh; /* its rectangle */
    uint32_t flags;        /* the flags byte of the resized calls (LLCOMP_MI_FLAG_MIRROR, LLCOMP_MI_FLAG_FILTER); bits above 7 are ignored */
} llcomp_mi_view; /* 24 bytes */
typedef struct llcomp_mi_view_group {
    uint32_t struct_size;               /* = sizeof(llcomp_mi_view_group); also the stride of an array of groups */
    uint32_t n_views;                   /* 1 .. 65535 */
    const llcomp_mi_view* views;        /* HOST memory, read during the call only */
    uint32_t ow, oh;                    /* the output shape of every view of the group */
    const llcomp_mi_output_format* fmt; /* NULL = U8 HWC; read during the call only */
    void* d_out;                        /* device memory, aligned to the format's element size (llcomp_mi_views_plan does not read it) */
} llcomp_mi_view_group; /* 40 bytes on LP64 */
/* What a views decode of these groups decodes: per frame the UNION rectangle (bounding box) of the frame's views over all groups ->
 * unions[4f .. 4f + 3] = {x, y, rw, rh}, or four zeros for a frame without a view; from the union rectangles of the USED frames alone,
 * in frame order, the windows and classes exactly as llcomp_mi_resized_regions_plan gives them for those rectangles -> windows[4f .. 4f + 3]
 * (four zeros for an unused frame), *n_used and *n_classes.  A frame decodes its window ONCE however many views it has -- and it decodes
 * everything inside the bounding box: a frame with two small views far apart decodes all that lies between them.  unions and windows
 * hold 4 * frames values each and may be NULL.  BAD_ARGS, with every output untouched: no groups, a NULL groups / n_used / n_classes, a
 * struct_size that is not the struct's, a group with no views, more than 65535 views, a NULL views or ow or oh 0; a view whose frame is
 * >= frames; a rectangle empty or outside the image; a filter code of 6 or 7 in a view's flags; a downscale above the view's filter's
 * limit for its group's output on either axis (llcomp_mi_resize_filter_weights).  Host-only. */
int llcomp_mi_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                         const llcomp_mi_view_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows, uint32_t* n_used,
                         uint32_t* n_classes);
/* Crops that leave the image (the padded calls below: RandomCrop(padding=...), pad_if_needed, a CenterCrop larger than the picture, a
 * random translate).  "Pad, then crop, then resize" without a padded copy: for one axis of side n and the rectangle [x, x + r) -- x a
 * signed 32-bit value, r >= 1, left pad p = max(-x, 0), right pad e = max(x + r - n, 0) -- an index t outside [0, n) stands for
 *   mode                         t < 0        t >= n            limit
 *   LLCOMP_MI_PAD_CONSTANT  0    the channel's fill value       p, e <= n
 *   LLCOMP_MI_PAD_EDGE      1    0            n - 1             p, e <= n
 *   LLCOMP_MI_PAD_REFLECT   2    -t           2 (n - 1) - t     p, e <= n - 1
 *   LLCOMP_MI_PAD_SYMMETRIC 3    -t - 1       2 n - 1 - t       p, e <= n
 * (source index m(t); numpy's np.pad modes and torchvision's padding_mode of the same names).  The rectangle must hold at least one
 * image pixel on each axis (x < n and x + r > 0), so r <= 3 n.
 * SOURCE INTERVAL [s0, s0 + s_len): the set of m(t) over the rectangle's indices -- contiguous, and for CONSTANT and EDGE
 * [max(x, 0), min(x + r, n)).  A frame's SOURCE RECTANGLE is the product of its two intervals: it lies inside the image and is all the
 * decoder sees.
 * FOLDED WEIGHTS AND BIAS: with (lo_i, q_ij) = llcomp_mi_resize_filter_weights(filter, r, out) -- the downscale limit is checked on
 * r -> out -- output i of the axis has Q_i[s] = sum_j { q_ij : m(x + lo_i + j) = s } over the source interval, and the bias
 * B_i = sum_j { q_ij : x + lo_i + j outside the image } for CONSTANT, 0 for every other mode; emitted as lo'[out] (relative to s0) and
 * q'[out][K'], zero taps trimmed, lo' + K' <= s_len (a run moved left over zero weights where needed).  K' <= K and
 * sum |Q| + |B| <= sum |q|, so the int32 accumulators hold.
 * OUTPUT: a pass computes clamp((sum_s Q_i[s] * in[s] + B_i * fill[ch] + 2^21) >> 22, 0, 255) -- the horizontal pass first, over the
 * SOURCE ROWS only, rounded to u8, then the vertical pass, the mirror and the output table.  A padded row needs no row in between: its
 * horizontal result is exactly fill[ch] (|fill * (sum q - 2^22)| < 2^21), which is what the vertical bias adds.  A rectangle inside the
 * image gives s0 = x, the unfolded weights and no bias: the unpadded call, byte for byte. */
enum { LLCOMP_MI_PAD_CONSTANT = 0, LLCOMP_MI_PAD_EDGE = 1, LLCOMP_MI_PAD_REFLECT = 2, LLCOMP_MI_PAD_SYMMETRIC = 3 };
typedef struct llcomp_mi_pad {
    uint32_t struct_size; /* sizeof(llcomp_mi_pad) (at least) */
    uint32_t mode;        /* LLCOMP_MI_PAD_*: one mode per call */
    const uint8_t* fill;  /* CONSTANT: c HOST values, NULL = zeros; ignored by every other mode; read during the call only */
} llcomp_mi_pad; /* 16 bytes on LP64 */
/* The source interval of one axis.  BAD_ARGS for a NULL s0 or s_len, a mode above 3, n or r 0, a rectangle with no image pixel, or a
 * pad above the mode's limit.  Host-only. */
int llcomp_mi_pad_axis(uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t* s0, uint32_t* s_len);
/* The folded rule of one axis: returns K' and fills *s0, lo[out_len], q[out_len][K'] (zero-padded) and bias[out_len]; each of the four
 * may be NULL.  For a rectangle inside the image lo and q are llcomp_mi_resize_filter_weights' with every run moved left until
 * lo + K <= r.  0 for what llcomp_mi_pad_axis or llcomp_mi_resize_filter_weights(filter, r, out_len) refuse.  Host-only; the GPU runs
 * exactly these weights. */
uint32_t llcomp_mi_padded_filter_weights(uint32_t filter, uint32_t mode, uint32_t n, int32_t x, uint32_t r, uint32_t out_len, uint32_t* s0,
                                         uint32_t* lo, int32_t* q, int32_t* bias);
/* Every frame's source rectangle: rects = {x, y, rw, rh} per frame (4 * n, x and y signed) -> src[4 * n] = {s0x, s0y, s_len_x, s_len_y}.
 * What a padded call decodes is what the unpadded calls decode for these rectangles: llcomp_mi_resized_regions_plan on them gives the
 * windows of a padded resized call, llcomp_mi_views_plan on the views' source rectangles the unions and windows of a padded views call.
 * BAD_ARGS, with src untouched: n = 0, a NULL rects, pad or src, a struct_size below the struct's, a mode above 3, a size below 1, a
 * rectangle with no image pixel on an axis, a pad above the mode's limit.  Host-only. */
int llcomp_mi_padded_regions_plan(uint32_t w, uint32_t h, const int32_t* rects, uint32_t n, const llcomp_mi_pad* pad, uint32_t* src);
/* Views under an affine map (llcomp_mi_codec_decode_warped_views below: RandomRotation, RandomAffine, PIL's Image.rotate and
 * Image.transform(AFFINE)).  A WARP VIEW is a frame and six numbers m[0..5]; view v of a group is byte for byte what
 *   PIL.Image.transform((ow, oh), Image.AFFINE, m, resample, fillcolor=fill)
 * gives on the decoded frame, for resample NEAREST, BILINEAR or BICUBIC.  Channels are independent bands, PIL's modes L, RGB and CMYK:
 * PIL premultiplies alpha for RGBA and LA under the two smooth filters, this library does not.
 * THE RULE.  The frame is P[h][w][c] of u8, the output ow x oh, fill[c] the fill.  All arithmetic is IEEE binary64, every operation
 * rounded by itself -- no fused multiply-add -- in the order written; cl(t, n) = min(max(t, 0), n - 1); every channel by itself.
 *   BILINEAR and BICUBIC, output pixel (x, y): xs = x + 0.5, ys = y + 0.5; xin = (m0 xs + m1 ys) + m2, yin = (m3 xs + m4 ys) + m5.  If not
 *     (0 <= xin < w and 0 <= yin < h) the pixel is fill.  Otherwise xin -= 0.5, yin -= 0.5, X = floor(xin), Y = floor(yin), dx = xin - X,
 *     dy = yin - Y, and
 *     BILINEAR: row(r) = P[r][cl(X, w)] + (P[r][cl(X + 1, w)] - P[r][cl(X, w)]) dx; v1 = row(cl(Y, h)); v2 = row(Y + 1) if 0 <= Y + 1 < h,
 *       else v1; v = v1 + (v2 - v1) dy; the output is v truncated toward zero.
 *     BICUBIC: cub(p0, p1, p2, p3, d) = p1 + d ((-p0 + p2) + d ((((2 (p0 - p1)) + p2) - p3) + d ((((-p0) + p1) - p2) + p3)));
 *       r0 = cub over columns cl(X - 1 .. X + 2, w) of row cl(Y - 1, h); for k = 1, 2, 3: the same on row Y - 1 + k if 0 <= Y - 1 + k < h,
 *       else r_k = r_(k-1); v = cub(r0, r1, r2, r3, dy); the output is 0 for v <= 0, 255 for v >= 255, else v truncated.
 *   NEAREST.  FIX(t) = floor(t * 65536 + 0.5) as int32.
 *     A pure scale (m1 == 0 and m3 == 0): xo_0 = m2 + m0 * 0.5, xo_(k+1) = xo_k + m0 -- accumulated, not k * m0; xi_k = -1 if xo_k < 0, else
 *       xo_k truncated; yi likewise from m5 + m4 * 0.5 in steps of m4.
 *     Any other matrix (PIL's 16.16 path): A0, A1, A3, A4 = FIX(m0), FIX(m1), FIX(m3), FIX(m4); A2 = FIX(m2 + m0 * 0.5 + m1 * 0.5),
 *       A5 = FIX(m5 + m3 * 0.5 + m4 * 0.5); xi = (A2 + x A0 + y A1) >> 16, yi = (A5 + x A3 + y A4) >> 16, in wrapping int32 with an
 *       arithmetic shift.
 *     Both: the output is P[yi][xi] if 0 <= xi < w and 0 <= yi < h, else fill.
 *   The mirror bit mirrors the view's output horizontally afterwards, and the output table (llcomp_mi_output_table) comes last, as in the other calls.
 * LIMITS (BAD_ARGS): a coefficient that is not finite; NEAREST: PIL's check_fixed must hold at (p, q) = (0, 0), (ow, 0), (0, oh),
 * (ow, oh): |p m0 + q m1 + m2| < 32768 and |p m3 + q m4 + m5| < 32768 (outside it PIL accumulates floats along every row, which is not
 * reproduced); BILINEAR and BICUBIC: |xin|, |yin| < 2^30 at the four corner pixels; a filter other than these three.  A view with no
 * pixel inside the image is NOT an error: its output is all fill. */
typedef struct llcomp_mi_warp_view {
    uint32_t frame; /* the frame of the batch the view is taken from */
    uint32_t flags; /* the flags byte of the resized calls: bit 0 mirrors the view's output, bits 4-6 hold the filter code; bits above 7 are ignored */
    double m[6];    /* output pixel -> source coordinate, as PIL's AFFINE data */
} llcomp_mi_warp_view; /* 56 bytes */
typedef struct llcomp_mi_warp_group {
    uint32_t struct_size;               /* = sizeof(llcomp_mi_warp_group); also the stride of an array of groups */
    uint32_t n_views;                   /* 1 .. 65535 */
    const llcomp_mi_warp_view* views;   /* HOST memory, read during the call only */
    uint32_t ow, oh;                    /* the output shape of every view of the group */
    const llcomp_mi_output_format* fmt; /* NULL = U8 HWC; read during the call only */
    void* d_out;                        /* device memory, aligned to the format's element size (the plan does not read it) */
    const uint8_t* fill;                /* c HOST bytes, NULL = zeros; read during the call only */
} llcomp_mi_warp_group; /* 48 bytes on LP64 */
/* The rectangle rect = {x, y, rw, rh} of image pixels one view reads: the bounding box of the rule's taps over the output pixels that lie
 * inside the image; *empty = 1 and four zeros when no output pixel does.  The coordinates are monotone in x and in y under the rule's
 * rounding, so every output row's inside pixels are one interval with the extremes at its ends (and, with all four corner pixels inside,
 * at those).  BAD_ARGS, outputs untouched: a NULL pointer, w or h 0, ow or oh 0, and the rule's limits.  Host-only. */
int llcomp_mi_warp_source_rect(uint32_t w, uint32_t h, const double* m, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4],
                               uint32_t* empty);
/* What a warped views decode of these groups decodes, in the shape of llcomp_mi_views_plan: a frame's union is the bounding box of its
 * views' source rectangles, the windows and classes are llcomp_mi_views_plan's for those rectangles; a frame whose views are all empty
 * is unused (four zeros), and with no used frame *n_used = *n_classes = 0.  BAD_ARGS, with every output untouched: no groups, a NULL
 * groups / n_used / n_classes, a struct_size that is not the struct's, a group with no views, more than 65535 views, a NULL views, ow or
 * oh 0, a view whose frame is >= frames, and the rule's limits.  Host-only. */
int llcomp_mi_warp_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                              const llcomp_mi_warp_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows, uint32_t* n_used,
                              uint32_t* n_classes);
/* The rule above on a host image: src [h][w][c] -> out [oh][ow][c] (no mirror, no output format), fill = c bytes or NULL for zeros.  It
 * is compiled from the same functions as the GPU's kernel and states the rule as llcomp_mi_resize_filter_weights does for the resized
 * calls; it is not fast.  BAD_ARGS, out untouched: a NULL src, m or out, a side or c of 0, and the rule's limits.  Host-only. */
int llcomp_mi_warp_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* m, uint32_t filter, const uint8_t* fill,
                             uint32_t ow, uint32_t oh, uint8_t* out);
/* Views under a projective map (llcomp_mi_codec_decode_perspective_views below: torchvision's RandomPerspective, PIL's
 * Image.transform(PERSPECTIVE)).  A PERSPECTIVE VIEW is a frame and eight numbers a[0..7]; view v of a group is byte for byte what
 *   PIL.Image.transform((ow, oh), Image.PERSPECTIVE, a, resample, fillcolor=fill)
 * gives on the decoded frame, for resample NEAREST, BILINEAR or BICUBIC, with independent bands as above (no alpha premultiplication).
 * THE RULE.  IEEE binary64, every operation rounded by itself, in the order written; the two divisions are true divisions (no
 * reciprocal).  Output pixel (x, y): xs = x + 0.5, ys = y + 0.5; den = (a6 xs + a7 ys) + 1; xin = ((a0 xs + a1 ys) + a2) / den;
 * yin = ((a3 xs + a4 ys) + a5) / den.
 *   BILINEAR and BICUBIC: from (xin, yin) on exactly the affine rule above -- the inside test, the tap origin and fractions, the taps.
 *   NEAREST (NOT the affine call's 16.16 path): xi = -1 if xin < 0, else xin truncated; yi likewise; the output is P[yi][xi] if
 *     0 <= xi < w and 0 <= yi < h, else fill.  With a6 = a7 = 0 this need not equal the affine call on a0..a5: it equals PIL's PERSPECTIVE.
 *   The mirror bit, the fill per channel, the output table and layout: as for the affine views.
 * LIMITS (BAD_ARGS): a coefficient that is not finite; a filter other than the three; an output side of 0; den, as the rule computes it,
 * not > 0 at one of the four corner pixels (the rounded den is monotone in x and in y, so its minimum sits at a corner: a map whose
 * denominator vanishes or changes sign inside the output is refused); |xin| or |yin| not below 2^30 at one of the four corner pixels.
 * A view with no pixel inside the image is NOT an error: its output is all fill. */
typedef struct llcomp_mi_perspective_view {
    uint32_t frame; /* the frame of the batch the view is taken from */
    uint32_t flags; /* as llcomp_mi_warp_view's: bit 0 mirrors the view's output, bits 4-6 hold the filter code; bits above 7 are ignored */
    double a[8];    /* output pixel -> source coordinate, as PIL's PERSPECTIVE data */
} llcomp_mi_perspective_view; /* 72 bytes */
typedef struct llcomp_mi_perspective_group {
    uint32_t struct_size;                    /* = sizeof(llcomp_mi_perspective_group); also the stride of an array of groups */
    uint32_t n_views;                        /* 1 .. 65535 */
    const llcomp_mi_perspective_view* views; /* HOST memory, read during the call only */
    uint32_t ow, oh;                         /* the output shape of every view of the group */
    const llcomp_mi_output_format* fmt;      /* NULL = U8 HWC; read during the call only */
    void* d_out;                             /* device memory, aligned to the format's element size (the plan does not read it) */
    const uint8_t* fill;                     /* c HOST bytes, NULL = zeros; read during the call only */
} llcomp_mi_perspective_group; /* 48 bytes on LP64 */
/* A rectangle rect = {x, y, rw, rh} of image pixels that CONTAINS every pixel the rule reads for the output pixels that lie inside the
 * image -- a bound, not the exact box: on no side more than one pixel beyond the taps of an inside pixel -- or *empty = 1 and four
 * zeros, exactly when no output pixel is inside.  Found from the first and last inside pixel of every output row (DESIGN.md "Perspective
 * views").  BAD_ARGS, outputs untouched: a NULL pointer, w or h 0, and the rule's limits.  Host-only. */
int llcomp_mi_perspective_source_rect(uint32_t w, uint32_t h, const double* a, uint32_t filter, uint32_t ow, uint32_t oh, uint32_t rect[4],
                                      uint32_t* empty);
/* llcomp_mi_warp_views_plan for perspective groups: the unions, windows and classes of llcomp_mi_views_plan on the views' source
 * rectangles (llcomp_mi_perspective_source_rect); the same BAD_ARGS cases.  Host-only. */
int llcomp_mi_perspective_views_plan(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t frames,
                                     const llcomp_mi_perspective_group* groups, uint32_t n_groups, uint32_t* unions, uint32_t* windows,
                                     uint32_t* n_used, uint32_t* n_classes);
/* The perspective rule on a host image, as llcomp_mi_warp_reference states the affine one: src [h][w][c] -> out [oh][ow][c], compiled
 * from the same functions as the GPU's kernel.  BAD_ARGS, out untouched: a NULL src, a or out, a side or c of 0, and the rule's limits.
 * Host-only. */
int llcomp_mi_perspective_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const double* a, uint32_t filter,
                                    const uint8_t* fill, uint32_t ow, uint32_t oh, uint8_t* out);
/* Photometric chains (llcomp_mi_codec_decode_photo_views / _photo_warped_views below: torchvision's ColorJitter with hue,
 * RandomGrayscale, PIL's GaussianBlur as the DINO and MoCo recipes apply it, and the colour ops of RandAugment / AutoAugment /
 * TrivialAugment, PIL backend).  A PHOTO CHAIN is 0 to
 * LLCOMP_MI_PHOTO_MAX_OPS ops {op, param}, applied in order to one view.
 * THE RULE.  The chain's input is what the call it extends writes for that view as U8 HWC: after the resample or the warp, and after the
 * mirror bit (every op commutes with the mirror: "mirror, then chain" is PIL's "flip, then jitter" and the reverse order alike).  The
 * output table (llcomp_mi_output_table) and the layout come after the chain, as they come last everywhere else.  Statistics are those of
 * the view's own oh x ow pixels as they stand when the op is reached, never those of the frame, the box or the group; n = oh * ow.
 *   L(r, g, b) = (19595 r + 38470 g + 7471 b + 0x8000) >> 16 for c = 3; L = v for c = 1.
 *   blend(d, v, a) is PIL's ImagingBlend, in IEEE binary32 with every operation rounded by itself, no fused multiply-add:
 *     t = (float)d + a * (float)(v - d); for 0 <= a <= 1 the result is t truncated toward zero; otherwise 0 for t <= 0, 255 for
 *     t >= 255, else t truncated.
 *   BRIGHTNESS  a  blend(0, v, a)                                           ImageEnhance.Brightness, adjust_brightness
 *   CONTRAST    a  m = (int)((double)sum of L / (double)n + 0.5) over the view, in binary64; then blend(m, v, a)
 *                                                                           ImageEnhance.Contrast, adjust_contrast
 *   COLOR       a  blend(L(pixel), v, a); identity for c = 1                ImageEnhance.Color, adjust_saturation
 *   GRAYSCALE   -  every channel becomes L(pixel); identity for c = 1       convert("L") replicated, RandomGrayscale
 *   INVERT      -  255 - v                                                  ImageOps.invert
 *   SOLARIZE    t  v if v < t, else 255 - v                                 ImageOps.solarize
 *   POSTERIZE   b  v & ~(2^(8 - b) - 1)                                     ImageOps.posterize
 *   AUTOCONTRAST -  per channel, from its histogram over the view: lo, hi = the lowest and highest value present; hi <= lo leaves the
 *                  channel unchanged; otherwise, in binary64, s = 255.0 / (hi - lo), o = -lo * s, lut[i] = clamp((int)(i * s + o), 0, 255),
 *                  the multiply and the add rounded separately, (int) truncating toward zero      ImageOps.autocontrast (cutoff 0)
 *   EQUALIZE    -  per channel, from its histogram h over the view: fewer than two values present leave the channel unchanged;
 *                  step = (n - h[last value present]) / 255 in integers, and step == 0 leaves it unchanged; otherwise acc = step / 2 and
 *                  for i = 0..255: lut[i] = min(255, acc / step), then acc += h[i]                ImageOps.equalize
 *   GAUSSIAN_BLUR radius  ImageFilter.GaussianBlur(radius): three box passes along every row, each reading the bytes the pass before
 *                  it wrote, then three along every column; every channel by itself; the window is symmetric, so the op commutes with
 *                  the mirror.  "f32": every operation rounded to binary32.
 *                  The box radius fr, f32: s2 = radius * radius / 3; L = (float)sqrt((double)(12 * s2 + 1)); l = floor((L - 1) / 2);
 *                    a = ((2l + 1) * (l * (l + 1) - 3 * s2)) / (6 * (s2 - (l + 1) * (l + 1))); fr = l + a
 *                    (radius 1 gives 0.25000003, radius 2 gives 1.375, radius 12 gives 11.479167).
 *                  The weights: r = (int)fr; ww = (uint32)((float)(1 << 24) / (fr * 2 + 1)), the division in f32;
 *                    fw = (uint32)((1 << 24) - (2r + 1) * ww) / 2, in wrapping uint32.
 *                  One pass over a line in[0..n-1], cl(i) = min(max(i, 0), n - 1): acc(x) = sum over k = -r..r of in[cl(x + k)];
 *                    far(x) = in[cl(x - r - 1)] + in[cl(x + r + 1)]; out[x] = (uint8)((acc * ww + far * fw + (1 << 23)) >> 24), in
 *                    wrapping uint32.  Radius 0 is the identity (r = 0, ww = 2^24, fw = 0).
 *   ADJUST_HUE  f  torchvision's adjust_hue(hue_factor = f), PIL backend; identity for c = 1.  shift = (uint8)(int32)((double)f * 255.0),
 *                  truncated toward zero, then mod 256; per pixel (H, S, V) = PIL's convert("HSV"), H = (H + shift) & 255, the pixel =
 *                  PIL's convert("RGB") of that.
 *                  RGB -> HSV: V = max; max == min gives H = S = 0; otherwise, f32: cr = max - min; s = cr / max;
 *                    rc, gc, bc = (max - r | g | b) / cr; h, in binary64 from these and then stored to f32: bc - gc where r is the max,
 *                    else (2.0 + rc) - bc where g is, else (4.0 + gc) - rc; h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
 *                    H = clip8((int)((double)h * 255.0)); S = clip8((int)((double)s * 255.0)).
 *                  HSV -> RGB: S == 0 gives r = g = b = V; otherwise, in binary64 on f32 values: hh = (double)(float)H * 6.0 / 255.0;
 *                    i = floor(hh); f = (float)(hh - (float)i); fs = (float)((float)S / 255.0); p = round(V * (1.0 - fs));
 *                    q = round(V * (1.0 - fs * f)); t = round(V * (1.0 - fs * (1.0 - f))), round C's (halves away from zero), each
 *                    clipped to 0..255; i % 6 selects (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q).  No fused multiply-add.
 *   ADJUST_SHARPNESS a  ImageEnhance.Sharpness(view).enhance(a) = Image.blend(view.filter(ImageFilter.SMOOTH), view, a), which is
 *                  torchvision's adjust_sharpness(img, a) on the PIL backend (RandomAdjustSharpness, the Sharpness op of RandAugment /
 *                  AutoAugment / TrivialAugmentWide); every channel by itself, c = 1 and c = 3; stated in integers:
 *                  d(x, y) = v(x, y) where x is 0 or ow - 1 or y is 0 or oh - 1 -- the outermost rows and columns, and so every
 *                    sample of a view with ow < 3 or oh < 3; otherwise d = (S + 6) / 13, floor division, with S = the sum of the nine
 *                    samples v(x - 1 .. x + 1, y - 1 .. y + 1) as they stand BEFORE the op, plus four times v(x, y).
 *                  The result is blend(d, v, a): a = 1 is the identity, a = 0 is SMOOTH itself, a > 1 sharpens.
 *                  (PIL sums the nine binary32 products of the kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 onto 0.5 and truncates; the exact
 *                  (S + 6.5) / 13 is never nearer than 1 / 26 to an integer and PIL's rounding error stays below 3e-4, so the integer
 *                  form is PIL's byte whatever the order of the sum.)  The window and the border rule are symmetric, so the op
 *                  commutes with the mirror.
 * LIMITS (BAD_ARGS): a factor a that is not finite or not within 0..256; a threshold t that is not an integer within 0..256; bits b
 * that are not an integer within 1..8; a radius that is not finite or not within 0..LLCOMP_MI_PHOTO_MAX_RADIUS; a hue factor that is not
 * finite or not within -0.5..0.5; an unknown op code (9..15 and 18 among them); more than LLCOMP_MI_PHOTO_MAX_OPS ops; and a chain that
 * is not empty on a codec whose c is neither 1 nor 3 (PIL's L and RGB).  The parameter of an op that takes none is ignored.  Views of
 * any width and height may blur and sharpen: there is no side limit.
 * NOT COVERED: torchvision's tensor-path GaussianBlur and adjust_sharpness (float convolutions: other rules), the other ImageFilter
 * kernels, alpha. */
#define LLCOMP_MI_PHOTO_MAX_OPS 8
#define LLCOMP_MI_PHOTO_MAX_RADIUS 32
enum {
    LLCOMP_MI_PHOTO_BRIGHTNESS = 0,
    LLCOMP_MI_PHOTO_CONTRAST = 1,
    LLCOMP_MI_PHOTO_COLOR = 2,
    LLCOMP_MI_PHOTO_GRAYSCALE = 3,
    LLCOMP_MI_PHOTO_INVERT = 4,
    LLCOMP_MI_PHOTO_SOLARIZE = 5,
    LLCOMP_MI_PHOTO_POSTERIZE = 6,
    LLCOMP_MI_PHOTO_AUTOCONTRAST = 7,
    LLCOMP_MI_PHOTO_EQUALIZE = 8,
    LLCOMP_MI_PHOTO_OP_COUNT = 9, /* the count of the pointwise family 0..8; codes 9..15 are no op */
    LLCOMP_MI_PHOTO_GAUSSIAN_BLUR = 16,
    LLCOMP_MI_PHOTO_ADJUST_HUE = 17,
    LLCOMP_MI_PHOTO_ADJUST_SHARPNESS = 19 /* code 18, like 9..15, is no op and stays refused */
};
typedef struct llcomp_mi_photo_op {
    uint32_t op; /* LLCOMP_MI_PHOTO_* */
    float param;
} llcomp_mi_photo_op;
typedef struct llcomp_mi_photo_chain {
    uint32_t n_ops; /* 0 .. LLCOMP_MI_PHOTO_MAX_OPS; 0 = the view as the extended call writes it */
    llcomp_mi_photo_op ops[LLCOMP_MI_PHOTO_MAX_OPS];
} llcomp_mi_photo_chain; /* 68 bytes */
typedef struct llcomp_mi_photo_group {
    uint32_t struct_size;                /* = sizeof(llcomp_mi_photo_group); also the stride of an array of them */
    const llcomp_mi_photo_chain* chains; /* one per view of the group it travels beside, HOST memory, read during the call only; NULL = none */
} llcomp_mi_photo_group; /* 16 bytes on LP64 */
/* The rule above on a host image, in place of a decode: src [h][w][c] -> out [h][w][c] (out may be src).  It is compiled from the same
 * functions as the GPU's kernels and states the rule as llcomp_mi_warp_reference does; it is not fast.  BAD_ARGS, out untouched: a NULL
 * src or out, a side of 0, a NULL ops with n_ops > 0, and the limits above (c other than 1 and 3 also with no op).  Host-only. */
int llcomp_mi_photo_reference(const uint8_t* src, uint32_t w, uint32_t h, uint32_t c, const llcomp_mi_photo_op* ops, uint32_t n_ops, uint8_t* out);
/* Batch mixing (llcomp_mi_codec_mix_batch below: torchvision's and timm's RandomErasing, MixUp and CutMix), in place on a dense batch
 * that a decode call has written: n samples of E = c * oh * ow elements of dtype U8, F16, BF16 or F32 (LLCOMP_MI_DTYPE_*) in layout HWC
 * [n][oh][ow][c] or CHW [n][c][oh][ow] (LLCOMP_MI_LAYOUT_*), aligned to the element's size and to nothing more.  Sample i has one record
 * (below); the call has erase_value, c floats (NULL = zeros).  The rule for the element at channel ch, row y, column x of sample i:
 *   1. Erase, per sample and ahead of the mix, as RandomErasing stands ahead of the collate in the recipes:
 *        e_i(ch, y, x) = erase_value[ch] converted to the dtype where (x, y) lies in erase_i, the element as it stood before the call
 *        elsewhere.  The conversion rounds to nearest even for F16 and BF16 (overflow to +-inf); U8 takes integers 0..255 only.
 *        (torch: img[..., y:y+h, x:x+w] = torch.tensor(value)[:, None, None])
 *   2. Mix, with p = partner_i:
 *        p == i:                      e_i
 *        else (x, y) in box_i:        e_p                                     (CutMix: out[..., y1:y2, x1:x2] = rolled[..., y1:y2, x1:x2])
 *        else with LLCOMP_MI_MIX_BLEND: rd(rd(e_i * w_own) + rd(e_p * w_partner))  (MixUp)
 *        else:                        e_i
 *      Both products and the sum are IEEE binary32 operations on the widened elements, each rounded by itself (no fused multiply-add);
 *      rd rounds to the dtype, to nearest even, and is the identity for F32.  With w_own = (float)lam and w_partner = (float)(1.0 - lam)
 *      for a double lam these are the bits of torchvision's inpt.roll(1, 0).mul(1.0 - lam).add_(inpt.mul(lam)) and of timm's
 *      x.mul_(lam).add_(x.flip(0).mul_(1 - lam)) as torch computes them on the CPU.  BLEND always computes, also for w_own = 1.  A blend
 *      whose result is a NaN writes the dtype's quiet NaN 0x7FC00000 / 0x7E00 / 0x7FC0, whatever the payloads were.
 * The partners form a permutation of 0..n-1 (roll: partner_i = (i + n - 1) % n; flip: n - 1 - i), so that the call runs in place.
 * NOT covered: RandomErasing(value="random"), which is normal noise per pixel; and the labels, which are n numbers the caller mixes
 * from lam and the boxes. */
#define LLCOMP_MI_MIX_BLEND 1u
typedef struct llcomp_mi_mix_sample {
    uint32_t partner;       /* the sample whose pixels are mixed in; == i: none */
    uint32_t flags;         /* bit 0 LLCOMP_MI_MIX_BLEND */
    float w_own, w_partner; /* BLEND's weights */
    uint32_t box[4];        /* x, y, w, h in output pixels: CutMix's box; w or h 0 = none */
    uint32_t erase[4];      /* x, y, w, h: RandomErasing's rectangle; w or h 0 = none */
} llcomp_mi_mix_sample;     /* 48 bytes */
/* What a call does with n records (DESIGN.md "Batch mixing"): the partner permutation cycle by cycle, every cycle of more than
 * llcomp_mi_mix_segment() samples cut into segments of at most that many.  order[n]: the samples, each cycle from its smallest sample
 * along the partners (order[j + 1] = partner of order[j] inside a cycle); seg_first[*n_segments + 1] (room for n + 1): where every
 * segment begins in order, the last entry n; *n_saved: the segments of the cycles that were cut -- the samples at their heads are copied
 * aside before anything is written.  order and seg_first may be NULL.  BAD_ARGS, outputs untouched: a NULL samples, n_segments or
 * n_saved, n = 0 or above 65535, a partner >= n, partners that are no permutation, flag bits above 0, a weight that is not finite.
 * Host-only. */
int llcomp_mi_mix_plan(uint32_t n, const llcomp_mi_mix_sample* samples, uint32_t* order, uint32_t* seg_first, uint32_t* n_segments,
                       uint32_t* n_saved);
uint32_t llcomp_mi_mix_segment(void);
/* The rule above on host memory: batch -> out, both n * c * oh * ow elements; out may be batch, and overlaps it in no other way.  It is
 * compiled from the same functions as the GPU's kernels; it is not fast.  BAD_ARGS, out untouched: a NULL batch, samples or out,
 * llcomp_mi_mix_plan's cases, a side or c of 0, an unknown dtype or layout, a box or erase rectangle that leaves ow x oh, BLEND on U8,
 * an erase value that is not finite, a U8 erase value that is no integer from 0 to 255.  Host-only. */
int llcomp_mi_mix_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                            const llcomp_mi_mix_sample* samples, const float* erase_value, void* out);
/* Batch orientation (llcomp_mi_codec_orient_batch below: RandomVerticalFlip, RandomHorizontalFlip on the finished batch, PIL's
 * Image.transpose, np.rot90), in place on a dense batch as the batch mixing takes it: n samples of c * oh * ow elements of dtype U8, F16,
 * BF16 or F32 in layout HWC [n][oh][ow][c] or CHW [n][c][oh][ow], aligned to the element's size and to nothing more.  Sample i has one
 * code, codes[i]: 0 for none, otherwise PIL's Image.Transpose value plus 1.  The rule for the pixel at row y, column x of sample i, all
 * c channels of a pixel alike:  out(x, y) = in(sx, sy)  with
 *   code  name              PIL method  (sx, sy)
 *   0     NONE              -           (x, y)
 *   1     FLIP_LEFT_RIGHT   0           (ow-1-x, y)
 *   2     FLIP_TOP_BOTTOM   1           (x, oh-1-y)
 *   3     ROTATE_90         2           (ow-1-y, x)          counter-clockwise, np.rot90(a, 1)
 *   4     ROTATE_180        3           (ow-1-x, oh-1-y)
 *   5     ROTATE_270        4           (y, oh-1-x)          np.rot90(a, 3)
 *   6     TRANSPOSE         5           (y, x)
 *   7     TRANSVERSE        6           (ow-1-y, oh-1-x)
 * Codes 3, 5, 6 and 7 would change the shape of a sample that is not square; the batch stays dense and the call runs in place, so they
 * take ow == oh only.  Elements are moved, never interpreted: NaN payloads, negative zeros and every other bit pattern survive, and only
 * the element's size tells the dtypes apart.  In CHW every plane of a sample is oriented alike; in HWC a pixel's c elements travel
 * together.
 * NOT covered: the transposing codes on outputs that are not square, and an out-of-place form (batch -> another buffer). */
enum {
    LLCOMP_MI_ORIENT_NONE = 0, LLCOMP_MI_ORIENT_FLIP_LEFT_RIGHT = 1, LLCOMP_MI_ORIENT_FLIP_TOP_BOTTOM = 2, LLCOMP_MI_ORIENT_ROTATE_90 = 3,
    LLCOMP_MI_ORIENT_ROTATE_180 = 4, LLCOMP_MI_ORIENT_ROTATE_270 = 5, LLCOMP_MI_ORIENT_TRANSPOSE = 6, LLCOMP_MI_ORIENT_TRANSVERSE = 7
};
/* The rule above on host memory: batch -> out, both n * c * oh * ow elements; out may be batch, and overlaps it in no other way.  It is
 * compiled from the same functions as the GPU's kernel; it is not fast.  BAD_ARGS, out untouched: a NULL batch, codes or out, n = 0 or
 * above 65535, a side or c of 0, an unknown dtype or layout, a code above 7, a transposing code (3, 5, 6, 7) with ow != oh.  Host-only. */
int llcomp_mi_orient_reference(const void* batch, uint32_t n, uint32_t c, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                               const uint8_t* codes, void* out);
/* The side, in pixels, of the tile of llcomp_mi_codec_orient_batch's kernel (DESIGN.md "Batch orientation"): a constant */
uint32_t llcomp_mi_orient_tile(void);
/* Batch composition (llcomp_mi_codec_compose_batch below: Mosaic, make_grid contact sheets, torchvision's batch_images collate,
 * RandomZoomOut on a batch, jigsaw shuffles, rectangle copy-paste, ResizeMix, CutMix between two batches, Cutout with several holes,
 * GridMask, Hide-and-Seek): rectangles of a source batch land at positions of a destination batch, the rest is a fill or stays.  Two
 * dense batches of the same c, dtype (U8, F16, BF16, F32) and layout (HWC or CHW), aligned to the element's size and to nothing more:
 * src, n_src samples of iw x ih, and dst, n_dst samples of ow x oh.  The call has a list of n_pieces records (below), fill_value (c
 * floats, NULL = zeros) and call flags.  The rule for the element at channel ch, row y, column x of dst sample d: take the LAST piece p
 * in list order with dst_p == d whose rectangle [dx, dx + w) x [dy, dy + h) holds (x, y) -- painter's order, later pieces win.
 *   p is a FILL piece:           fill_value[ch] converted to the dtype
 *   any other p:                 src(src_p, ch, sy_p + y - dy_p, sx_p + x - dx_p), moved as bits
 *   no such piece, KEEP set:     the element as it stood; it is not written
 *   no such piece, KEEP not set: fill_value[ch] converted
 * Elements are moved, never interpreted: NaN payloads and negative zeros survive, and only the element's size tells the dtypes apart.
 * The fill converts as the batch mixing's erase_value does: to nearest even for F16 and BF16, U8 takes integers 0..255 only, a value that
 * is not finite is refused.  Pieces come in any order of dst, may overlap and may be hidden entirely; a piece with w or h 0 is ignored
 * (but checked).  src may be NULL with n_src == 0 when every piece is a FILL piece (with KEEP: the in-place erase of many rectangles);
 * otherwise the byte ranges of the two batches must not overlap.
 * BAD_ARGS: a NULL pieces with n_pieces > 0; n_dst or n_src above 65535, n_dst == 0, n_pieces above 2^20; ow, oh or c of 0, iw or ih
 * of 0 with n_src > 0; a row of ow * c or iw * c elements or more than 2^31, a batch no address space holds; an unknown dtype or
 * layout; a piece with dst >= n_dst; a piece that is no FILL piece with src >= n_src or a source rectangle that leaves iw x ih; a piece
 * whose rectangle leaves ow x oh; a FILL piece with src, sx or sy not 0; flag or reserved bits that are not defined; a bad fill value;
 * more than llcomp_mi_compose_max_pieces_per_sample() = 1024 pieces with w and h above 0 on one dst sample.
 * NOT covered: pieces that resample or mirror (views do that at decode), and a src and dst that differ in dtype or layout.  Masks that
 * are not rectangles: "Batch copy-paste" below; the boxes of id maps: "Label boxes" below. */
#define LLCOMP_MI_COMPOSE_FILL 1u /* piece flag */
#define LLCOMP_MI_COMPOSE_KEEP 1u /* call flag: elements no piece covers keep their value and are not written */
typedef struct llcomp_mi_compose_piece {
    uint32_t dst, src;       /* sample of dst; sample of src (0 for a FILL piece) */
    uint32_t dx, dy, sx, sy; /* where the rectangle lands; where it is read (0, 0 for a FILL piece) */
    uint32_t w, h;           /* w or h 0: the piece is ignored */
    uint32_t flags;          /* bit 0 LLCOMP_MI_COMPOSE_FILL: the rectangle is the call's fill value, nothing is read */
    uint32_t reserved;       /* 0 */
} llcomp_mi_compose_piece;   /* 40 bytes */
/* The rule above on host memory.  out (n_dst samples) may be dst_in, and overlaps src in no way; dst_in is read only under KEEP and may
 * be NULL without it.  It is compiled from the same functions as the GPU's kernel; it is not fast.  BAD_ARGS, out untouched: the cases
 * above, a NULL out, a NULL dst_in under KEEP, a NULL src with n_src > 0.  Host-only. */
int llcomp_mi_compose_reference(const void* src, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow,
                                uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_compose_piece* pieces,
                                uint32_t n_pieces, const float* fill_value, uint32_t flags, void* out);
/* What a call does (DESIGN.md "Batch composition"): samples[*n_samples] (room for n_dst), the dst samples that get workgroups, ascending
 * -- all of them, or under KEEP those with a piece of w and h above 0; first[*n_samples + 1] (room for n_dst + 1) and order (room for
 * n_pieces): sample j's pieces are order[first[j] .. first[j + 1]), indices into pieces in the call's order, the ignored ones left out;
 * *n_workgroups: the workgroups of the call's one kernel, 0 for a call that queues nothing.  samples, first and order may be NULL.
 * BAD_ARGS, outputs untouched: the cases above, a NULL n_samples or n_workgroups.  Host-only. */
int llcomp_mi_compose_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, uint32_t flags, uint32_t* samples,
                           uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups);
/* The kernel's tile: llcomp_mi_compose_tile() pixels across (128) and llcomp_mi_compose_tile_rows(pixel_bytes) rows, where pixel_bytes
 * is the element's size in CHW and c elements in HWC: the power of two, at most 64, that keeps a tile within 16 KiB.  Constants. */
uint32_t llcomp_mi_compose_tile(void);
uint32_t llcomp_mi_compose_tile_rows(uint32_t pixel_bytes);
uint32_t llcomp_mi_compose_max_pieces_per_sample(void);
/* Batch copy-paste (llcomp_mi_codec_paste_batch below: Simple Copy-Paste of Ghiasi et al., torchvision's reference SimpleCopyPaste, the
 * paste of class maps, the renumbering of instances in id maps): the OBJECTS of one decoded sample land in another, chosen by the ids
 * of an id map.  Three dense batches: src, n_src samples of iw x ih, and dst, n_dst samples of ow x oh, of the same c, dtype (U8, F16,
 * BF16, F32) and layout (HWC or CHW), aligned to the element and to nothing more; and mask, n_src samples of ih x iw BYTES at any byte
 * address, mask[s] the id map of src[s]: mask(s, y, x) = mask[(s * ih + y) * iw + x].  The call has a list of n_pieces records (below),
 * in painter's order.  Piece p SELECTS (x, y) of dst sample d when dst_p == d, (x, y) lies in [dx, dx + w) x [dy, dy + h), and bit m of
 * ids_p is set for m = mask(src_p, sy + y - dy, sx + x - dx).  The element at channel ch, row y, column x of d takes the LAST piece of
 * the list that selects (x, y):
 *   p is a VALUE piece:  value_p converted to the dtype, the same for every channel
 *   any other p:         src(src_p, ch, sy_p + y - dy_p, sx_p + x - dx_p), moved as bits
 *   no such piece:       the element stays AND IS NOT WRITTEN -- the call is always in place on dst, there is no fill
 * The value converts as the composition's fill does: to nearest even for F16 and BF16, U8 takes integers 0..255 only, a value that is
 * not finite is refused.  A piece with w or h 0, or with no id bit set, is checked and ignored.  Elements are never interpreted: NaN
 * payloads and negative zeros survive.  dst must not overlap src or mask in bytes; src and mask may overlap or be the same buffer (for
 * c == 1 U8 the id maps are their own source: that is how a class map is pasted).  It covers binary masks (all bits but bit 0), one
 * instance or a drawn subset of instances per piece, and a VALUE piece per instance with the id it gets in the dst map -- the second
 * call of a Copy-Paste, on the maps.
 * BAD_ARGS: a dst or a src that is no dense batch (n above 65535 or 0, a side or c of 0, an unknown dtype or layout, a batch no address
 * space holds); n_src == 0 with n_pieces > 0; a NULL pieces with n_pieces > 0; n_pieces above 2^20; a row of ow * c or iw * c elements
 * of 2^31 elements or more; a piece with dst >= n_dst or src >= n_src, with a source rectangle that leaves iw x ih or a dst rectangle
 * that leaves ow x oh, with flag bits above bit 0, with a value that is not 0 without VALUE, or with a bad value under VALUE; more than
 * llcomp_mi_paste_max_pieces_per_sample() = 256 pieces with w and h above 0 on one dst sample.
 * Blended pastes under a per-pixel alpha: "Batch alpha paste" below.
 * NOT covered: Gaussian paste borders made from the ids, a src and dst of different dtype or layout, pieces that resample or mirror
 * (views do that at decode), a dst that overlaps its src, per-piece fills per channel.  More than 256 ids per map (16-bit id maps):
 * "Batch copy-paste by 16-bit ids" below. */
#define LLCOMP_MI_PASTE_VALUE 1u
typedef struct llcomp_mi_paste_piece {
    uint32_t dst, src;
    uint32_t dx, dy, sx, sy, w, h;
    uint32_t flags;        /* bit 0 LLCOMP_MI_PASTE_VALUE */
    float value;           /* VALUE's value; 0 without VALUE */
    uint32_t ids[8];       /* 256 bits: bit m set = mask byte m is selected */
} llcomp_mi_paste_piece;   /* 72 bytes */
/* The rule above on host memory.  out (n_dst samples) may be dst_in -- otherwise dst_in is copied into it first -- and overlaps src and
 * mask in no way.  It is compiled from the same functions as the GPU's kernel; it is not fast.  BAD_ARGS, out untouched: the cases
 * above, a NULL out or dst_in, a NULL src or mask with n_pieces > 0, src or out not aligned to the element.  Host-only. */
int llcomp_mi_paste_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                              uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece* pieces,
                              uint32_t n_pieces, void* out);
/* What a call does, as llcomp_mi_compose_plan: samples[*n_samples] (room for n_dst), the dst samples with a piece that is not ignored,
 * ascending; first[*n_samples + 1] and order (room for n_pieces): sample j's pieces are order[first[j] .. first[j + 1]), indices into
 * pieces in the call's order, the ignored ones left out; *n_workgroups: the workgroups of the call's one kernel (the composition's
 * tiles), 0 for a call that queues nothing.  samples, first and order may be NULL.  BAD_ARGS, outputs untouched: the cases above, a NULL
 * n_samples or n_workgroups.  Host-only. */
int llcomp_mi_paste_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                         uint32_t layout, const llcomp_mi_paste_piece* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first,
                         uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups);
uint32_t llcomp_mi_paste_max_pieces_per_sample(void);
/* Batch copy-paste by 16-bit ids (llcomp_mi_codec_paste_batch16 below): the rule of "Batch copy-paste" with a 16-bit mask, for the
 * instance and panoptic label sets with more than 256 ids per map (Cityscapes' class * 1000 + k, Mapillary Vistas' class * 256 + k,
 * ADE20K, KITTI-STEP, cell masks).  src, dst, painter's order, "the last piece that selects a pixel gives it" and "what no piece
 * selects stays and is not written" are unchanged.  mask is n_src samples of ih x iw little-endian uint16_t, dense, aligned to 2 bytes
 * and to nothing more: mask16(s, y, x).  A u16 map stored as a two-channel container (low byte in channel 0) decodes to one with the
 * nearest filter in U8 HWC.  Piece p selects (x, y) when its rectangle holds the pixel and, for m = mask16(src_p, sy + y - dy,
 * sx + x - dx), m - id_base < 256 holds in 32-bit unsigned arithmetic and bit m - id_base of ids is set.  A set of ids wider than 256
 * is several pieces over the same rectangle; the per-sample limit stays llcomp_mi_paste_max_pieces_per_sample() = 256 pieces.
 * id_base + 255 may pass 65535: those bits select nothing, and a piece with no other bit set is checked and ignored.  A VALUE piece's
 * value is given as BITS, value_bits, the element's bits in its low esize bytes, the same in every channel: a VALUE piece writes a new
 * 16-bit id into a dst map that is passed as a 2-byte dtype with c == 1 (elements are never interpreted, so F16 or BF16 serve) -- the
 * renumbering call of a Copy-Paste.  dst must not overlap src or mask in bytes; src and mask may be one buffer: for U8 HWC with c == 2,
 * and for a 2-byte dtype with c == 1, the id maps are their own source -- that is how a 16-bit class or instance map is pasted by id.
 * BAD_ARGS: the cases of "Batch copy-paste" (but for its value), an id_base above 65535, a value_bits that is not 0 without VALUE or
 * that has bits above the element.
 * Ids of 3 or 4 bytes (COCO panoptic's RGB ids): "Wide id maps" below.  NOT covered: maps at odd addresses, borders blended from the ids ("Batch alpha paste" below blends under an alpha batch), and what
 * "Batch copy-paste" does not cover. */
typedef struct llcomp_mi_paste_piece16 {
    uint32_t dst, src;
    uint32_t dx, dy, sx, sy, w, h;
    uint32_t flags;        /* bit 0 LLCOMP_MI_PASTE_VALUE */
    uint32_t value_bits;   /* VALUE: the element's bits in its low esize bytes, the same in every channel; 0 without VALUE */
    uint32_t id_base;      /* 0..65535 */
    uint32_t ids[8];       /* bit j set: id id_base + j is selected */
} llcomp_mi_paste_piece16; /* 76 bytes */
/* The rule above on host memory, as llcomp_mi_paste_reference.  BAD_ARGS, out untouched: the cases above, a NULL out or dst_in, a NULL
 * src or mask with n_pieces > 0, src or out not aligned to the element, a mask not aligned to 2 bytes.  Host-only. */
int llcomp_mi_paste16_reference(const void* src, const void* mask, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in, uint32_t n_dst,
                                uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece16* pieces,
                                uint32_t n_pieces, void* out);
/* What a call does: the outputs of llcomp_mi_paste_plan.  Host-only. */
int llcomp_mi_paste16_plan(uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                           uint32_t layout, const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, uint32_t* samples, uint32_t* first,
                           uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups);
/* Label boxes (llcomp_mi_codec_label_boxes below: torchvision's masks_to_boxes of every instance of an id map, with the areas): maps is
 * n samples of oh x ow bytes, dense, at any byte address -- an instance id or class id per pixel, as the containers of label images
 * decode, behind any crop, affine, perspective, flip, mosaic or paste.  The output is n * 256 records; for sample i and id m, record
 * i * 256 + m has count, the number of pixels equal to m, and [x0, x1) x [y0, y1), their bounding box; with count == 0 it is
 * {0, ow, oh, 0, 0}, the identities of min and max, so records of two maps merge by min, max and add.  masks_to_boxes of instance m is
 * (x0, y0, x1 - 1, y1 - 1), and count its area.  Every record is written: the caller initialises nothing.
 * BAD_ARGS: n of 0 or above 65535, ow or oh of 0, ow * oh of 2^32 or more, a batch no address space holds, a NULL pointer.
 * More than 256 ids per map (16-bit id maps): "Label boxes of listed ids" below. */
typedef struct llcomp_mi_label_box {
    uint32_t count, x0, y0, x1, y1;
} llcomp_mi_label_box;     /* 20 bytes */
/* The rule above on host memory: out holds n * 256 records.  Host-only. */
int llcomp_mi_label_boxes_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, llcomp_mi_label_box* out);
/* The rows of the band of a sample that a workgroup of llcomp_mi_codec_label_boxes takes (DESIGN.md "Label boxes"): a constant */
uint32_t llcomp_mi_label_boxes_rows(void);
/* Label boxes of listed ids (llcomp_mi_codec_label_boxes16 below: "Label boxes" above for the 16-bit id maps of instance and panoptic
 * label sets -- Cityscapes' class * 1000 + k, Mapillary Vistas' class * 256 + k, ADE20K, KITTI-STEP, cell masks): maps is n samples of
 * oh x ow little-endian uint16_t, dense, aligned to 2 bytes and to nothing more -- what a u16 map stored as a two-channel container
 * (low byte in channel 0) decodes to with the nearest filter in U8 HWC.  The caller NAMES the ids it wants: sample i lists
 * ids[first[i] .. first[i + 1]), strictly ascending, first[0] == 0, at most llcomp_mi_label_boxes16_max_ids() = 4096 ids per sample and
 * first[n] <= 2^20 in all.  The output is first[n] records of llcomp_mi_label_box: record first[i] + j is for id ids[first[i] + j] of
 * sample i, its pixel count and box, {0, ow, oh, 0, 0} without a pixel.  Every record is written.  Pixels whose id is not listed are
 * counted nowhere; a sample with an empty list costs nothing.
 * BAD_ARGS: the cases of "Label boxes", a NULL ids or first, first[0] != 0, a first that decreases, a list of more than 4096 ids, more
 * than 2^20 ids in all, a list that is not strictly ascending, maps not aligned to 2 bytes.
 * Ids of 3 or 4 bytes (COCO panoptic's RGB ids): "Wide id maps" below.  NOT covered: maps at odd addresses. */
int llcomp_mi_label_boxes16_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids, const uint32_t* first,
                                      llcomp_mi_label_box* out);
/* The most ids a sample lists: 22 bytes of a workgroup's LDS per listed id, one workgroup to a CU at the top capacity.  A constant. */
uint32_t llcomp_mi_label_boxes16_max_ids(void);
/* Label targets (llcomp_mi_codec_label_targets below: what a loss or a head takes from the id maps that the label boxes take -- a
 * class-index tensor for CrossEntropyLoss, one-hot planes for Dice, focal and smoothed losses, one binary mask per instance for Mask
 * R-CNN, Mask2Former and Copy-Paste's targets).  maps is n samples of P = oh * ow pixels, dense: map_bytes 1, bytes at any address, or
 * map_bytes 2, little-endian uint16_t aligned to 2 bytes.  Sample i lists ids[first[i] .. first[i + 1]), strictly ascending,
 * first[0] == 0, at most 4096 ids per sample and first[n] <= 2^20 in all as "Label boxes of listed ids", with one int32_t value per
 * listed id; for map_bytes 1 an id is at most 255.  The value of a pixel is
 *   v(i, p) = values[first[i] + j] if map(i, p) == ids[first[i] + j], else default_value;
 * several ids may share a value (the instances of a class).
 * INDEX: out[i * P + p] = v(i, p) as uint8_t, int32_t or int64_t (sign-extended): torch's lut[map.long()].  Every element is written,
 * those of a sample with an empty list too.
 * PLANES: sample i owns the planes plane_first[i] .. plane_first[i + 1]), K_i of them, at most llcomp_mi_label_targets_max_planes() =
 * 4096, plane_first[0] == 0; element (plane_first[i] + k) * P + p is on_bits where v(i, p) == k, else off_bits, in dtype
 * LLCOMP_MI_DTYPE_U8, _F16, _BF16 or _F32.  on_bits and off_bits are the element's bits in their low esize bytes (1 and 0; 0x3C00 and 0
 * for F16; label smoothing passes the bits of 1 - eps + eps / K and eps / K).  A value outside [0, K_i) selects no plane ("ignore").
 * Every element of every plane is written once.  One-hot planes [n][K][oh][ow] are plane_first[i] = i * K; the masks of the listed
 * instances are values 0, 1, 2, ... with default_value -1.
 * The output is dense and aligned to its element's size and to nothing more.
 * BAD_ARGS: the cases of "Label boxes of listed ids"; a NULL struct, values or (PLANES) plane_first; a struct_size below the struct's;
 * a map_bytes that is not 1 or 2, a kind or dtype that is none; an id above 255 with map_bytes 1; with INDEX U8 a value or default
 * outside 0..255; plane_first[0] != 0, a plane_first that decreases, more than 4096 planes of a sample; on_bits or off_bits with bits
 * above the element; an output of 2^62 bytes or more.
 * Ids of 3 or 4 bytes: llcomp_mi_label_targets32, "Wide id maps" below (map_bytes 3 or 4 stays BAD_ARGS here).
 * NOT covered: HWC one-hot ([n][oh][ow][K]), in-place conversion, 16-bit maps at odd addresses, a table kept on
 * the device across calls, targets as a job of the streaming pipeline, soft or blended mask borders, boxes or labels from the lists. */
enum { LLCOMP_MI_TARGET_INDEX = 0, LLCOMP_MI_TARGET_PLANES = 1 };
enum { LLCOMP_MI_TARGET_U8 = 0, LLCOMP_MI_TARGET_I32 = 1, LLCOMP_MI_TARGET_I64 = 2 };   /* INDEX dtypes */
typedef struct llcomp_mi_label_targets {
    uint32_t struct_size, map_bytes, kind, dtype;   /* dtype: LLCOMP_MI_TARGET_* for INDEX, LLCOMP_MI_DTYPE_* for PLANES */
    int32_t default_value;
    uint32_t on_bits, off_bits;                     /* PLANES */
    const uint16_t* ids;                            /* host arrays, read during the call */
    const int32_t* values;
    const uint32_t* first;                          /* first[n + 1] */
    const uint32_t* plane_first;                    /* PLANES: plane_first[n + 1] */
} llcomp_mi_label_targets;                          /* 64 bytes, ids at 32 */
/* The rule above on host memory: out holds llcomp_mi_label_targets_out_bytes bytes.  BAD_ARGS, out untouched: the cases above, a NULL
 * maps or out, maps (map_bytes 2) or out not aligned to their element.  Host-only. */
int llcomp_mi_label_targets_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* targets, void* out);
/* The bytes of a call's output: n * P elements for INDEX, plane_first[n] * P for PLANES; 0 for a bad call. */
uint64_t llcomp_mi_label_targets_out_bytes(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets* targets);
/* The pixels of the segment of a sample that a workgroup of llcomp_mi_codec_label_targets takes (DESIGN.md "Label targets"), and the
 * most planes of a sample: constants */
uint32_t llcomp_mi_label_targets_segment(void);
uint32_t llcomp_mi_label_targets_max_planes(void);
/* Wide id maps (llcomp_mi_codec_paste_batch32, llcomp_mi_codec_label_boxes32 and llcomp_mi_codec_label_targets32 below): "Batch
 * copy-paste by 16-bit ids", "Label boxes of listed ids" and "Label targets" for id maps of 3 or 4 bytes per pixel -- COCO panoptic's id = R + 256 * G + 65536 * B, and the int32 maps of class * 1000 +
 * instance sets whose ids pass 65535.  maps is n samples of oh x ow pixels, dense, of map_bytes little-endian bytes each:
 *   map_bytes 3: at ANY byte address, the id is b0 | b1 << 8 | b2 << 16 -- what a panoptic PNG stored as a three-channel container
 *                decodes to with the nearest filter in U8 HWC
 *   map_bytes 4: aligned to 4 bytes and to nothing more -- a four-channel container, or an int32 tensor
 * The map is never written, and no byte outside it is read.  The listed ids are uint32_t, every value of the map's width among them
 * (0, 0xFFFFFF, 0xFFFFFFFF); the lists' limits, the records, the values, the kinds and the output dtypes are those of the 16-bit calls.
 * BAD_ARGS: the 16-bit calls' cases; a map_bytes that is not 3 or 4; a listed id above 0xFFFFFF with map_bytes 3; a 4-byte map at an
 * address that is no multiple of 4.
 * NOT covered: 4-byte maps at addresses that are no multiples of 4, and what the 16-bit calls do not cover.  Batches of 2^32 bytes
 * and more, and samples of more than 2^31 pixels, are covered (the arithmetic is 64-bit; tests/test_gpu_large_wide_id_maps.py).
 * Batch copy-paste by wide ids (llcomp_mi_codec_paste_batch32 below) is "Batch copy-paste by 16-bit ids" word for word -- painter's
 * order, the last piece that selects a pixel gives it, what no piece selects stays and is not written, a dst element is written at
 * most once, 256 pieces per dst sample -- with mask the wide map above, map_bytes 3 or 4.  id_base is any 32-bit value (above 0xFFFFFF
 * with map_bytes 3: BAD_ARGS); a window that passes the top id selects nothing there, and a piece with no other bit set is checked and
 * ignored.  RGB ids are sparse, so a window is mostly ONE id per piece; the limit of 256 pieces still holds a COCO image's segments.
 * The maps may be their own source: map_bytes 3 as U8 HWC with c == 3; map_bytes 4 as U8 HWC with c == 4 or F32 with c == 1.
 * LLCOMP_MI_PASTE_VALUE_PIXEL (this call only; with VALUE; U8 HWC with c <= 4): channel ch of a selected pixel takes byte ch of
 * value_bits, whose bytes at and above c are 0 -- how a pasted segment gets a new 3-byte id in a dst map, the renumbering call of a
 * Copy-Paste.  BAD_ARGS: the 16-bit call's cases, a map_bytes that is not 3 or 4, VALUE_PIXEL without VALUE or on another dtype,
 * layout or c, value bytes at or above c, a 4-byte mask at an address that is no multiple of 4. */
#define LLCOMP_MI_PASTE_VALUE_PIXEL 2u
typedef struct llcomp_mi_paste_piece32 {
    uint32_t dst, src;
    uint32_t dx, dy, sx, sy, w, h;
    uint32_t flags;        /* bit 0 LLCOMP_MI_PASTE_VALUE, bit 1 LLCOMP_MI_PASTE_VALUE_PIXEL */
    uint32_t value_bits;
    uint32_t id_base;      /* any 32-bit value; map_bytes 3: at most 0xFFFFFF */
    uint32_t ids[8];       /* bit j set: id id_base + j is selected */
} llcomp_mi_paste_piece32; /* 76 bytes, the layout of llcomp_mi_paste_piece16 */
int llcomp_mi_paste32_reference(const void* src, const void* mask, uint32_t map_bytes, uint32_t n_src, uint32_t iw, uint32_t ih, const void* dst_in,
                                uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout,
                                const llcomp_mi_paste_piece32* pieces, uint32_t n_pieces, void* out);
int llcomp_mi_paste32_plan(uint32_t map_bytes, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c,
                           uint32_t dtype, uint32_t layout, const llcomp_mi_paste_piece32* pieces, uint32_t n_pieces, uint32_t* samples,
                           uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups);
int llcomp_mi_label_boxes32_reference(const void* maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh, const uint32_t* ids,
                                      const uint32_t* first, llcomp_mi_label_box* out);
typedef struct llcomp_mi_label_targets32 {
    uint32_t struct_size, map_bytes, kind, dtype;   /* map_bytes 3 or 4; the rest as llcomp_mi_label_targets */
    int32_t default_value;
    uint32_t on_bits, off_bits;
    const uint32_t* ids;
    const int32_t* values;
    const uint32_t* first;
    const uint32_t* plane_first;
} llcomp_mi_label_targets32;                        /* 64 bytes, ids at 32 */
int llcomp_mi_label_targets32_reference(const void* maps, uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* targets, void* out);
uint64_t llcomp_mi_label_targets32_out_bytes(uint32_t n, uint32_t ow, uint32_t oh, const llcomp_mi_label_targets32* targets);
/* Batch alpha paste (llcomp_mi_codec_alpha_paste_batch below): PIL's Image.paste(src, box, mask), Image.composite and
 * Image.alpha_composite on dense batches, byte for byte -- the step of a compositing pipeline that blends per pixel: a sprite or an
 * instance through a soft matte, a Copy-Paste with soft borders, a watermark.  src is n_src samples of iw x ih and dst n_dst samples of
 * ow x oh, both of c channels in one dtype (U8, F16, BF16, F32) and one layout, aligned to the element and to nothing more.  alpha is
 * n_src samples of ih x iw pixels of alpha_px_bytes (1..4) bytes each, dense, at ANY byte address; a pixel's alpha is byte alpha_byte
 * (< alpha_px_bytes) of it, a byte for every dtype of the batches: a plain matte has alpha_px_bytes 1; the A channel of a U8 HWC RGBA
 * batch, which may be src itself, alpha_px_bytes 4 and alpha_byte 3.  dst overlaps neither src nor alpha; neither is written.
 * A piece is a rectangle as in the paste calls, (sx, sy) addressing src AND alpha.  The pieces of a dst sample apply in the list's
 * order, each onto what the pieces before it left: painter's order forwards.  At most 256 pieces with w and h above 0 on one dst sample.
 *   LLCOMP_MI_ALPHA_VALUE        the source element is value_bits, the element's bits, in every channel (src may then be NULL when
 *                                no other piece reads it)
 *   LLCOMP_MI_ALPHA_VALUE_PIXEL  with VALUE, U8 HWC with c <= 4: channel ch takes byte ch of value_bits -- PIL's paste of a colour
 *   LLCOMP_MI_ALPHA_OVER         the OVER rule
 * The PASTE rule (the default), d and s the dst and src elements, m the pixel's alpha byte:
 *   m == 0: the element keeps its bits; m == 255: it takes s's bits, whatever d was;
 *   U8 otherwise: t = d * (255 - m) + s * m + 128, out = ((t >> 8) + t) >> 8  (PIL's paste with an L mask, Image.composite)
 *   F16, BF16, F32 otherwise: a = float(m) / 255.0f, out = rd(f32(d * (1.0f - a)) + f32(s * a)): every operation rounded in binary32
 *     by itself, no fused multiply-add, one rounding to the dtype, a NaN the dtype's one quiet NaN -- torch's
 *     (d * (1 - a) + s * a).to(dtype) with a = alpha.float() / 255 on the CPU
 * The OVER rule (Image.alpha_composite): U8 HWC with c == 4, src and dst aligned to 4 bytes; the alpha is src's own channel 3 and the
 * alpha argument is not read for such a piece; not with VALUE.  Per pixel with sa, da in 32-bit unsigned arithmetic: sa == 0: the
 * pixel stays; otherwise outa255 = sa * 255 + da * (255 - sa), coef1 = sa * 255 * 255 * 128 / outa255, coef2 = 255 * 128 - coef1; a
 * colour channel: t = s * coef1 + d * coef2 + (0x80 << 7), out = (((t >> 8) + t) >> 8) >> 7; alpha: t = outa255 + 0x80,
 * out = ((t >> 8) + t) >> 8.
 * BAD_ARGS: the paste calls' cases; alpha_px_bytes outside 1..4; alpha_byte >= alpha_px_bytes; unknown flag bits; OVER or VALUE_PIXEL
 * on a shape it does not take, OVER with VALUE, VALUE_PIXEL without it; value_bits with bytes at or above the element's size, for
 * VALUE_PIXEL at or above c, or without VALUE; a NULL alpha with a piece that is not OVER, a NULL src with one that is not VALUE.
 * NOT covered: a src with another channel count than dst (an RGBA sprite onto an RGB canvas in one call), float alpha maps, a
 * per-piece opacity, making a feathered matte from an id selection (the step towards Copy-Paste with Gaussian borders), Image.blend,
 * and PIL's special case of a COLOUR pasted onto an RGBA pixel whose alpha is 0 (there PIL replaces the colour channels whatever the
 * mask says; a VALUE_PIXEL piece follows the PASTE rule in every channel, which is PIL's result on L and RGB). */
#define LLCOMP_MI_ALPHA_VALUE 1u
#define LLCOMP_MI_ALPHA_VALUE_PIXEL 2u
#define LLCOMP_MI_ALPHA_OVER 4u
typedef struct llcomp_mi_alpha_piece {
    uint32_t dst, src;
    uint32_t dx, dy, sx, sy, w, h;
    uint32_t flags;        /* LLCOMP_MI_ALPHA_* */
    uint32_t value_bits;   /* with VALUE; otherwise 0 */
} llcomp_mi_alpha_piece;   /* 40 bytes */
/* The rule on host memory: out = dst_in with the pieces applied (out may be dst_in). */
int llcomp_mi_alpha_paste_reference(const void* src, const void* alpha, uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw,
                                    uint32_t ih, const void* dst_in, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t c, uint32_t dtype,
                                    uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, void* out);
/* What a call does, as llcomp_mi_paste32_plan: the dst samples with a piece that is not ignored, samples[*n_samples]; where every
 * sample's pieces begin, first[*n_samples + 1]; the pieces' indices by dst sample in the call's order, order[first[*n_samples]]; and
 * the workgroups of the kernel.  samples, first and order may be NULL. */
int llcomp_mi_alpha_paste_plan(uint32_t alpha_px_bytes, uint32_t alpha_byte, uint32_t n_src, uint32_t iw, uint32_t ih, uint32_t n_dst, uint32_t ow,
                               uint32_t oh, uint32_t c, uint32_t dtype, uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces,
                               uint32_t* samples, uint32_t* first, uint32_t* order, uint32_t* n_samples, uint64_t* n_workgroups);
uint32_t llcomp_mi_slice_count(uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar);
/* Slice width for one-row slices (tile_h = 1) when `frames` frames are coded per call: the widest slice (64..480 pixels) that
 * still keeps about four wavefronts per SIMD busy.  A call that codes few frames is latency-bound with wide slices; this
 * trades a little compression (fresh models per slice) for it.  Returns 0 for nonsense arguments. */
uint32_t llcomp_mi_suggest_tile_w(uint32_t frames, uint32_t w, uint32_t h, uint32_t c, uint32_t planar);
/* FNV-1a-64 of a byte range (the checksum tests/golden records containers in); seed 0 starts a hash, a previous result
 * continues it over the next piece (header, slice table and payload of a container that lies in three buffers).  A running
 * hash that happens to be 0 (probability 2^-64 per piece) cannot be told from "start" and would restart: good enough for a
 * checksum of test vectors, not a keyed or adversarial hash. */
uint64_t llcomp_mi_fnv1a64(const uint8_t* data, size_t len, uint64_t seed);
/* Concatenator for multi-GPU sharding: `bands` are SLICED containers of consecutive horizontal bands of one
 * image (same width/channels/tile/planar; every band but the last a multiple of tile_h rows, because slices
 * have slice-local borders a band's slices ARE the full image's slices).  Produces the container of the whole
 * image.  Inverse: llcomp_mi_split_band extracts tile rows [tile_row0, tile_row1). */
int llcomp_mi_merge_bands(const uint8_t* const* bands, const size_t* band_lens, uint32_t n_bands, uint8_t** out,
                          size_t* out_len);
int llcomp_mi_split_band(const uint8_t* data, size_t len, uint32_t tile_row0, uint32_t tile_row1, uint8_t** out,
                         size_t* out_len);
/* The work split of every multi-GPU path (device lists here, ranks in llcomp_amd/sharding.py -- ONE implementation): the tile rows of
 * an image of `height` pixel rows in consecutive chunks, chunk i owned by part i % n_parts; chunks are as even as the tile grid allows,
 * and with fewer tile rows than n_parts * chunks_per_part every chunk is one tile row.  Writes (tile_row0, tile_row1, owner) triples
 * to `triples` (room for cap_chunks of them; NULL = only count) and the number of chunks to *n_chunks.  OUTPUT_OVERFLOW when
 * cap_chunks is too small (*n_chunks says what it takes).  tile_h 0 or > height = the whole height; chunks_per_part 0 = 4. */
int llcomp_mi_plan_chunks(uint32_t height, uint32_t tile_h, uint32_t n_parts, uint32_t chunks_per_part, uint32_t* triples,
                          uint32_t cap_chunks, uint32_t* n_chunks);

/* ---- device-resident batch codec: buffers stay in HBM, work is enqueued on the caller's stream --------- */
/* One codec object = fixed geometry (frames x h x w x c, tiling) + its own workspace on one device.
 * `frames` images of identical shape are coded per call; every frame gets the slices of the SLICED format
 * (slice ids run frame-major).  All device pointers are hipMalloc'ed (or torch) memory on that device.
 *
 * Alignment of the device pointers.
 *   Any byte address: pixels in and out (d_px, d_rect), payloads in and out (d_payload, d_sub_payload, d_payload_out), and both byte
 *     ranges of llcomp_mi_device_copy_segments.  A frame of a batch, a payload inside a container in HBM (24 + 4n bytes in) or a piece
 *     of a receive buffer is passed as it lies.
 *   Natural alignment: d_slice_len, d_sub_len, d_slice_len_out, d_status and d_sym 4 bytes; d_total and d_sub_total 8 bytes; the u64
 *     tables of llcomp_mi_device_copy_segments / _range_sums 8 bytes (d_vals 4); a float output of the _ex calls its element size.
 *     A pointer of this kind that is not aligned is LLCOMP_MI_BAD_ARGS before anything is launched or written.
 *   Bounds: a call reads nothing outside [d_payload, d_payload + payload_bytes) and the frames*h*w*c bytes of its pixels, and writes
 *     nothing outside [d_payload, d_payload + payload_cap) and the frames*rh*rw*c (h*w*c, oh*ow*c) bytes of its output. */
typedef struct llcomp_mi_codec llcomp_mi_codec;
int llcomp_mi_codec_create(llcomp_mi_codec** codec, int32_t device, uint32_t frames, uint32_t w, uint32_t h,
                           uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar);
/* flags: LLCOMP_MI_FLAG_SMALL_MODEL */
int llcomp_mi_codec_create_ex(llcomp_mi_codec** codec, int32_t device, uint32_t frames, uint32_t w, uint32_t h,
                              uint32_t c, uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t flags);
/* Does not wait for the device: the workspace is parked behind an event recorded on the stream of the codec's LAST encode /
 * decode (whether that call succeeded or not) and is handed out again only after it.  (One exception, microseconds in practice: a
 * codec destroyed right behind a 2-D decode waits for that call's 16-byte feedback copy, whose pinned mailbox it is about to free.)  That stream should outlive the work
 * queued on it; if it is destroyed earlier (legal HIP: hipStreamDestroy drains it in the background) the library notices the
 * dead event when the blocks are taken out again and drains the whole device instead. */
void llcomp_mi_codec_destroy(llcomp_mi_codec* codec);
uint32_t llcomp_mi_codec_slices(const llcomp_mi_codec* codec);        /* total = frames * slices per frame */
/* Diagnostic: which kernel family the codec's geometry selected when it was created -- bit 0 one-row slices (states on chip),
 * bit 1 one slice per wavefront (state table in LDS), bit 2 forced replay (test hook), bit 3 small model, bit 4 the encoder's state
 * snapshot pass, bit 5 the 2-D decoder's bank cache in LDS; bits 8..15 log2 of the lane-group width, bits 16..23 slices per
 * wavefront.  No effect on any output byte: tests use it to make sure they run the family they mean to. */
uint32_t llcomp_mi_codec_kernel_family(const llcomp_mi_codec* codec);
/* Device bytes the codec can hold at most.  The per-slice state tables (decoding 2-D slices; 63 KB per slice) and the snapshot
 * arrays of the 2-D encoder (22 B per sample; 28 B and the coder's parking records of 64 B per slice where slices are above 4096
 * samples) are allocated by the first call that needs them, so an encode-only or decode-only codec stays below this figure; that
 * first call can return LLCOMP_MI_NOMEM. */
uint64_t llcomp_mi_codec_workspace_bytes(const llcomp_mi_codec* codec);
/* Diagnostic: the device bytes the codec holds right now (what the calls so far have allocated; never above
 * llcomp_mi_codec_workspace_bytes, except through a resized regions decode to an output larger than the image, or a views decode of
 * more views than frames: llcomp_mi_codec_views_workspace_bytes; the padded, warped and photometric calls have bounds of their own). */
uint64_t llcomp_mi_codec_allocated_bytes(const llcomp_mi_codec* codec);
/* Allocates NOW what the first encode (LLCOMP_MI_PREPARE_ENCODE: the 2-D encoder's snapshot arrays with their parking records, or its state tables) and / or
 * the first decode (LLCOMP_MI_PREPARE_DECODE: the state tables of 2-D slices) would otherwise allocate inside the call -- for callers
 * that need the first call to be like every other one (no hipMalloc behind work already queued on their stream, no NOMEM in the
 * middle of a pipeline).  Idempotent; LLCOMP_MI_NOMEM when the device cannot give the memory. */
#define LLCOMP_MI_PREPARE_ENCODE 1u
#define LLCOMP_MI_PREPARE_DECODE 2u
#define LLCOMP_MI_PREPARE_REGION 8u /* the region decode's two arrays (12 B per slice), and state tables if a region may need them (bit 2 stays unused) */
#define LLCOMP_MI_PREPARE_REGIONS 16u /* ... and the per-frame table of a regions decode (32 B per frame in HBM, a pinned staging ring) */
#define LLCOMP_MI_PREPARE_RESIZED 32u /* ... and the boxes and the horizontal pass's rows of a resized regions decode (frames * w * h * c bytes each) */
#define LLCOMP_MI_PREPARE_UPDATE 64u /* ... and a region update's offset arrays (8 B per slice) and its box pixel buffer (frames * w * h * c bytes) */
#define LLCOMP_MI_PREPARE_VIEWS 128u /* ... what LLCOMP_MI_PREPARE_RESIZED allocates, and the staging buffer for the tables of a views decode
                                        from HBM of up to `frames` views (a _host call's staged payload and more views grow it) */
int llcomp_mi_codec_prepare(llcomp_mi_codec* codec, uint32_t what);
/* Upper bound on the packed payload bytes the codec can emit for any input (13 B per sample + slack). */
uint64_t llcomp_mi_codec_max_payload_bytes(const llcomp_mi_codec* codec);
/* encode: d_px [frames][h][w][c] u8 -> d_payload (slice payloads packed back to back, slice order),
 * d_slice_len u32[slices], d_total u64[1] (= sum of lengths).  payload_cap = bytes available at d_payload; if
 * the packed size exceeds it nothing past the capacity is written and the status word reports OVERFLOW.
 * Asynchronous on `stream` (a hipStream_t, NULL = default stream).  d_status: u32[1], LLCOMP_MI_OK or an error,
 * valid once the stream has drained. */
int llcomp_mi_codec_encode(llcomp_mi_codec* codec, const void* d_px, void* d_payload, uint64_t payload_cap,
                           void* d_slice_len, void* d_total, void* d_status, void* stream);
/* decode: inverse.  d_payload/d_slice_len as produced by encode (payload_bytes = total), d_px out. */
int llcomp_mi_codec_decode(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes,
                           const void* d_slice_len, void* d_px, void* d_status, void* stream);
/* Region decode of a batch: the rectangle (x, y, rw, rh) of every frame (one rectangle for all frames of the call) -> d_px
 * [frames][rh][rw][c].  d_payload / payload_bytes / d_slice_len are the FULL batch's, as for llcomp_mi_codec_decode; only the covered
 * slices' table entries and payload bytes are read (semantics and verdicts: llcomp_mi_decode_region).  The decoder runs on the geometry
 * of the covered sub-image inside the codec's own workspace.  Asynchronous on `stream` like a decode; profile slots 4, 5, 6 (and 7).
 * The first region call allocates 12 B per slice (LLCOMP_MI_PREPARE_REGION does it ahead) and can return LLCOMP_MI_NOMEM. */
int llcomp_mi_codec_decode_region(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                  uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, void* d_px, void* d_status, void* stream);
/* Diagnostic: the kernel family (encoding of llcomp_mi_codec_kernel_family) a region decode of this rectangle runs -- the sub-image's
 * geometry may select another one than the codec's (a 1-row remainder of 2-row tiles runs the row kernels).  0 for a bad rectangle. */
uint32_t llcomp_mi_codec_region_family(const llcomp_mi_codec* codec, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh);
/* Region update of a batch, the write side of llcomp_mi_codec_decode_region: the rectangle (x, y, rw, rh) of every frame (one rectangle
 * for all frames of the call) is replaced by d_rect [frames][rh][rw][c], and only the slices of the tiles it touches are coded again.
 * Because every slice is the reference stream of its own crop, the result is byte for byte what llcomp_mi_codec_encode gives for the
 * modified frames.  Both calls are asynchronous on `stream`, run in the codec's workspace on the geometry of the covered box
 * (llcomp_mi_codec_region_family reports its kernel family) and write d_status like an encode.
 *   encode_region: -> d_sub_payload (the covered slices' new streams back to back, capacity sub_payload_cap, OVERFLOW as for an encode),
 *     d_sub_len u32[covered slices of all frames], d_sub_total u64[1]; order: frame, tile row, tile column, plane -- per frame what
 *     llcomp_mi_replace_slices takes.
 *   update_region: the same work, then the splice in HBM: -> d_payload_out (capacity payload_cap; a slice that would end past it is
 *     not written and the status is OVERFLOW), d_slice_len_out u32[slices], d_total u64[1], as llcomp_mi_codec_encode would
 *     write them for the modified frames.  The outputs must not overlap d_payload / d_slice_len: both are read to the end of the call.
 * A rectangle that is exactly its box's pixels (tile-aligned, or reaching the image edge) needs nothing of the old covered slices: the
 * encoder reads d_rect itself, no decoder runs (n_decode of llcomp_mi_codec_get_profile does not move), and d_payload / d_slice_len may
 * be NULL for encode_region.  Otherwise the box is decoded first (the chain of llcomp_mi_codec_decode_region, whole box), the rectangle is
 * pasted into it and the box is encoded: BAD_EXPONENT and TRUNCATED then come from the covered slices, through the status word, and
 * what the call has written is not to be used.  Slices outside the box are never decoded: damage there is carried over verbatim; an
 * uncovered slice whose table entry runs past payload_bytes is TRUNCATED (update_region; nothing is read past the payload).  BAD_ARGS,
 * before anything is launched or written: a NULL pointer, a rectangle empty or outside the image.  HIP_ERROR, likewise, if the
 * sub-geometry's arrays would not fit the workspace (never with default tuning).  The first call allocates what LLCOMP_MI_PREPARE_UPDATE
 * | LLCOMP_MI_PREPARE_ENCODE allocate ahead, and the state tables or snapshot arrays a sub-geometry needs where the codec's own family
 * does not (llcomp_mi_codec_workspace_bytes counts them); it can return LLCOMP_MI_NOMEM. */
int llcomp_mi_codec_encode_region(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                                  uint32_t y, uint32_t rw, uint32_t rh, const void* d_rect, void* d_sub_payload, uint64_t sub_payload_cap,
                                  void* d_sub_len, void* d_sub_total, void* d_status, void* stream);
int llcomp_mi_codec_update_region(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len, uint32_t x,
                                  uint32_t y, uint32_t rw, uint32_t rh, const void* d_rect, void* d_payload_out, uint64_t payload_cap,
                                  void* d_slice_len_out, void* d_total, void* d_status, void* stream);
/* Regions decode of a batch: frame f's rectangle (xy[2f], xy[2f + 1], rw, rh) -> d_px[f] of [frames][rh][rw][c], dense, in frame order:
 * byte for byte full_decode[f, y_f : y_f + rh, x_f : x_f + rw].  xy is HOST memory, 2 * frames values, read during the call and never
 * after it returns.  d_payload / payload_bytes / d_slice_len are the full batch's, as for llcomp_mi_codec_decode.  Each frame decodes
 * its window of tiles (llcomp_mi_regions_plan); each class of windows is one sub-geometry and one launch chain, the classes run in
 * order on `stream`, and the call is asynchronous like a decode.  Verdicts (BAD_EXPONENT, TRUNCATED) come from the slices of the
 * decoded WINDOWS: damage in a window tile outside the rectangle IS reported (unlike llcomp_mi_codec_decode_region, which reads the
 * covered box only), damage outside every window is never seen.  Any rectangle outside the image is BAD_ARGS, and nothing is launched
 * or written.  Profile slots 4-7 and the counters accumulate as for a region decode; each class takes a state generation of its own.
 * The first call allocates what LLCOMP_MI_PREPARE_REGIONS allocates ahead and can return LLCOMP_MI_NOMEM.  The per-frame table reaches
 * the GPU from a small pinned ring: a call waits only for the table copy of the call four before it on that codec. */
int llcomp_mi_codec_decode_regions(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                   const uint32_t* xy, uint32_t rw, uint32_t rh, void* d_px, void* d_status, void* stream);
/* Diagnostic: the kernel family (encoding of llcomp_mi_codec_kernel_family) of every class a regions decode of these rectangles runs,
 * in class order (bit 0 = partial last tile column, bit 1 = partial last tile row), the first `cap` of them to fam.  Returns the
 * number of classes; 0 for bad arguments. */
uint32_t llcomp_mi_codec_regions_family(const llcomp_mi_codec* codec, const uint32_t* xy, uint32_t rw, uint32_t rh, uint32_t* fam,
                                        uint32_t cap);
/* The same regions decode from HOST containers: data[f] / lens[f] are the frames' single-frame SLICED containers (f < frames; the codec's
 * shape, tiling, planar setting and model), and only their windows' bytes cross PCIe.  d_px and the status word get the same bytes as
 * llcomp_mi_codec_decode_regions on the payload and table of the same containers packed back to back, for every input whose slice
 * tables fit their containers.  The call runs llcomp_mi_regions_gather into a slot of the codec's pinned ring (with the per-frame table
 * and every window slice's offset) and queues ONE host-to-device copy of it into a staging buffer of the codec; the decode then runs as
 * for llcomp_mi_codec_decode_regions, class by class on `stream`.  The containers and xy are read during the call only: the caller may
 * free or overwrite them as soon as it returns.  A gather error (llcomp_mi_regions_gather; BAD_ARGS also for containers that do not match
 * the codec) is returned before anything is queued, and d_px / d_status stay untouched.  The pinned slots and the staging buffer grow
 * geometrically when a call needs more (never per call; llcomp_mi_codec_workspace_bytes counts the buffer's upper bound): such a call can
 * return LLCOMP_MI_NOMEM.  A call waits only for the copy of the call four before it on that codec.  LLCOMP_MI_CTR_HOST_STAGED_BYTES
 * counts the payload bytes staged.  Profile slots as for a regions decode. */
int llcomp_mi_codec_decode_regions_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens, const uint32_t* xy, uint32_t rw,
                                        uint32_t rh, void* d_px, void* d_status, void* stream);
/* Regions decode with a rectangle of its own size per frame, every rectangle resampled to one output shape (torchvision's
 * RandomResizedCrop, and RandomHorizontalFlip through flags): rects = {x, y, rw, rh} per frame (4 * frames, HOST memory), flags = one
 * byte per frame (HOST memory, NULL = none; bit 0 mirrors the frame's output horizontally after resampling, bits 4-6 choose the frame's
 * filter, LLCOMP_MI_FLAG_FILTER(LLCOMP_MI_FILTER_*): a batch may mix filters, e.g. pictures and their label images) -> d_px
 * [frames][oh][ow][c], dense: byte for byte the rule of llcomp_mi_resize_filter_weights applied to full_decode[f, y_f : y_f + rh_f, x_f : x_f + rw_f].  rects and
 * flags are read during the call only.  Every frame decodes a window of tiles sized for the batch's largest rectangle
 * (llcomp_mi_resized_regions_plan): a frame with a small rectangle decodes as much as one with the largest.  The classes run as in
 * llcomp_mi_codec_decode_regions and crop every frame's BOX (the largest rectangle's size, containing the frame's rectangle) into a buffer
 * of the codec; two resample kernels then write d_px.  Asynchronous on `stream`; verdicts as for llcomp_mi_codec_decode_regions (from the
 * decoded windows' slices).  BAD_ARGS, before anything is launched or written: a NULL pointer, ow or oh 0, a rectangle empty or outside the
 * image, a filter code of 6 or 7, or a downscale above the frame's filter's limit on either axis (R * rw_f > 64 * ow or R * rh_f > 64 * oh;
 * R = 1, BICUBIC 2, LANCZOS 3).  Profile slots as for a regions decode; the resample
 * is timed in slot 6 with the crops.  The boxes (frames * rw_max * rh_max * c bytes) and the horizontal pass's rows (frames * rh_max * ow *
 * c) are buffers of the codec that grow geometrically, never per call, and never past frames * w * h * c each but where a call needs
 * more (LLCOMP_MI_PREPARE_RESIZED allocates both at that size).  llcomp_mi_codec_workspace_bytes counts both at that size and the tables
 * and weights the staging buffer carries, for outputs no larger than the image (ow <= w, oh <= h); a larger output can take the rows'
 * buffer and the staging buffer beyond it.  A call that grows a buffer waits for the codec's last call and can return LLCOMP_MI_NOMEM.  The regions table, the per-frame resample table and every
 * frame's weights reach the GPU in ONE copy from the pinned ring of llcomp_mi_codec_decode_regions. */
int llcomp_mi_codec_decode_resized_regions(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                           const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh, void* d_px, void* d_status,
                                           void* stream);
/* ... from HOST containers, as llcomp_mi_codec_decode_regions_host is to llcomp_mi_codec_decode_regions: only the windows' bytes cross
 * PCIe (in the same one copy as the tables and weights), the containers, rects and flags may be reused as soon as the call returns, a
 * gather error is returned before anything is queued, LLCOMP_MI_CTR_HOST_STAGED_BYTES counts the staged payload bytes. */
int llcomp_mi_codec_decode_resized_regions_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens, const uint32_t* rects,
                                                const uint8_t* flags, uint32_t ow, uint32_t oh, void* d_px, void* d_status, void* stream);
/* The two calls above with an output format (llcomp_mi_output_format; NULL = U8 HWC, the calls above exactly): d_out receives
 * frames * oh * ow * c elements of fmt's dtype in its layout, element [f][ch][y][x] (CHW) or [f][y][x][ch] (HWC) = the table of
 * llcomp_mi_output_table at [ch][v], v the u8 call's byte for (f, y, x, ch).  The table travels in the call's one copy, behind the
 * weights.  BAD_ARGS, before anything is queued or written (d_status untouched): every case of the calls above, every case of the
 * table's, and a d_out not aligned to the element size.  fmt, mean and std are read during the call only. */
int llcomp_mi_codec_decode_resized_regions_ex(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                              const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                                              const llcomp_mi_output_format* fmt, void* d_out, void* d_status, void* stream);
int llcomp_mi_codec_decode_resized_regions_host_ex(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens, const uint32_t* rects,
                                                   const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_output_format* fmt,
                                                   void* d_out, void* d_status, void* stream);
/* Several views of each frame, each frame decoded ONCE (llcomp_mi_view / llcomp_mi_view_group / llcomp_mi_views_plan above): every
 * used frame decodes the window of its views' union rectangle -- the classes of llcomp_mi_codec_decode_resized_regions, unchanged, over the
 * used frames only, sized for the largest union, each cutting its frame's box into a buffer of the codec; a frame without a view has no
 * table entry and none of its slices is read.  Then, group by group, the two resample kernels read every view's rectangle from ITS
 * FRAME's box and write the group's d_out: view v of a group gets byte for byte what llcomp_mi_codec_decode_resized_regions_ex writes for
 * that rectangle of that frame with the view's flags and the group's ow, oh and fmt (a view's bytes do not depend on the box it is read
 * from: no tap leaves the rectangle).  d_payload / payload_bytes / d_slice_len are the full batch's.  Asynchronous on `stream`; d_status
 * and the verdicts as for llcomp_mi_codec_decode_resized_regions on the union rectangles of the used frames (damage outside every
 * window, and anywhere in an unused frame, is never seen).  BAD_ARGS, before anything is queued or written (d_status untouched): a NULL
 * codec, payload, table or status, a misaligned d_slice_len or d_status, every case of llcomp_mi_views_plan, a bad output format
 * (llcomp_mi_output_table), and a group's d_out NULL or not aligned to its element size.  The regions table, every group's view table,
 * the weights (an axis that several views share is computed and sent once per call) and the output tables cross in the call's ONE copy
 * from the pinned ring.  Memory: the boxes take used frames * union_w_max * union_h_max * c bytes, never above frames * w * h * c; the
 * horizontal pass's rows of a group take n_views * rh_max * ow * c bytes (rh_max: the group's largest view height), and where that passes
 * frames * w * h * c the group is resampled in chunks of views, so the rows' buffer never grows past that bound for ow <= w (one view
 * always fits).  Profile slots and n_decode as for one resized regions decode. */
int llcomp_mi_codec_decode_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                 const llcomp_mi_view_group* groups, uint32_t n_groups, void* d_status, void* stream);
/* ... from HOST containers, as llcomp_mi_codec_decode_resized_regions_host: data[f] / lens[f] for f < frames, and only the union windows'
 * bytes cross PCIe, in the same one copy as the tables (LLCOMP_MI_CTR_HOST_STAGED_BYTES counts them: what the resized call stages for the
 * union rectangles).  data[f] of a frame without a view may be NULL and is never read; a NULL container of a used frame is BAD_ARGS.  Same
 * bytes and status as the call above on the same containers packed back to back. */
int llcomp_mi_codec_decode_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens, const llcomp_mi_view_group* groups,
                                      uint32_t n_groups, void* d_status, void* stream);
/* llcomp_mi_codec_workspace_bytes for calls of up to total_views views: it bounds llcomp_mi_codec_allocated_bytes for outputs no larger
 * than the image (ow <= w, oh <= h) and at most 1 + max(total_views - frames, 0) groups with an output format.  The staged tables grow
 * with the views: every view beyond `frames` adds 48 + 40 * (w + h) + 16 + 1024 * c bytes (its table entry, its weights at their upper
 * bound, and an output table); for total_views <= frames this is llcomp_mi_codec_workspace_bytes. */
uint64_t llcomp_mi_codec_views_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
/* The _ex resized calls with rectangles that may leave the image (llcomp_mi_pad above): rects = {x, y, rw, rh} per frame, x and y signed;
 * fmt NULL = U8 HWC.  Every frame decodes the window of its SOURCE rectangle -- the classes, the gather and the one copy of
 * llcomp_mi_codec_decode_resized_regions_ex on the source rectangles, unchanged -- and the resample kernels run the folded weights on
 * it: no pass over padded pixels and no padded copy in HBM.  Frame f gets byte for byte the _ex call's output for np.pad(frame, mode)
 * cut at the rectangle; a rectangle inside the image gives the _ex call's bytes for it.  Only CONSTANT with a fill other than 0 on a
 * rectangle that leaves the image needs what the unpadded kernels do not have: the bias forms of the three resample kernels, which start
 * every accumulator at bias * fill[ch]; a launch uses them when an entry of its chunk has a bias that is not 0
 * (LLCOMP_MI_CTR_BIAS_LAUNCHES counts those launches) and the parent's kernels otherwise.  d_status and the verdicts as for the _ex call
 * on the source rectangles.  BAD_ARGS, before anything is queued or written (d_status untouched): every case of the _ex call, a NULL pad, a
 * struct_size below the struct's, a mode above 3, a size below 1, a pad above the mode's limit, a rectangle with no image pixel on an
 * axis. */
int llcomp_mi_codec_decode_padded_regions(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                          const int32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_pad* pad,
                                          const llcomp_mi_output_format* fmt, void* d_out, void* d_status, void* stream);
int llcomp_mi_codec_decode_padded_regions_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens, const int32_t* rects,
                                               const uint8_t* flags, uint32_t ow, uint32_t oh, const llcomp_mi_pad* pad,
                                               const llcomp_mi_output_format* fmt, void* d_out, void* d_status, void* stream);
/* llcomp_mi_codec_decode_views(_host) with views that may leave the image: the same group and view structs, a view's x and y read as
 * two's-complement int32, one pad for the call.  A frame decodes the bounding box of its views' SOURCE rectangles; view v of a group gets
 * byte for byte what llcomp_mi_codec_decode_padded_regions writes for that rectangle.  BAD_ARGS: every case of the views call (on the
 * source rectangles) and of the pad, as above. */
int llcomp_mi_codec_decode_padded_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                        const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad, void* d_status,
                                        void* stream);
int llcomp_mi_codec_decode_padded_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                             const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad, void* d_status,
                                             void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes for padded calls of up to total_views views (a padded resized call: `frames`) with
 * ow <= w, oh <= h.  The boxes and the horizontal pass's rows shrink or stay -- source rectangles lie inside the image -- but the staged
 * tables grow: r reaches 3 n, so an axis takes out * (K' + 1) int32 of weights and `out` of bias with K' <= K <= 6 * max(r / out, 1) + 3,
 * at most 6 * max(r, out) + 5 * out <= 23 * side against the unpadded 10 * side, and the call adds c int32 of fill values.  So this is
 * llcomp_mi_codec_views_workspace_bytes(total_views) + max(total_views, frames) * 52 * (w + h) + 4 * c: every view beyond `frames` adds
 * 48 + 92 * (w + h) + 16 + 1024 * c bytes.  llcomp_mi_codec_workspace_bytes and _views_workspace_bytes keep their values. */
uint64_t llcomp_mi_codec_padded_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
/* llcomp_mi_codec_decode_views(_host) with views that are affine maps (llcomp_mi_warp_view / llcomp_mi_warp_group / the rule above).
 * Every used frame decodes ONCE, and only the window of the bounding box of the source pixels its views read (llcomp_mi_warp_views_plan):
 * the windows, classes, boxes, the gather of a host source and the one copy are those of a views call on the source rectangles,
 * unchanged.  Then one gather kernel per group -- one thread per output pixel, no intermediate buffer -- reads every view from ITS
 * FRAME's box and writes the group's d_out, dense in view order as the views call does: view v gets byte for byte the rule's output
 * for its frame, mirrored if bit 0 of its flags is set, through the group's output format.  Each view's entry (its matrix, or the six
 * fixed-point integers, or the offsets of its xi / yi tables for the pure-scale form, which the host computes), the groups' fill values
 * and the output tables cross in the call's ONE copy.  d_status and the verdicts are those of the views call on the unions (damage outside
 * every window, and anywhere in an unused frame, is never seen); with no used frame the call decodes nothing and the status is OK.
 * BAD_ARGS, before anything is queued or written (d_status untouched): a NULL codec, payload, table or status, a misaligned d_slice_len
 * or d_status, every case of llcomp_mi_warp_views_plan, a bad output format, a group's d_out NULL or not aligned to its element size.
 * _host: data[f] / lens[f] for f < frames; only the union windows' bytes cross PCIe (LLCOMP_MI_CTR_HOST_STAGED_BYTES: what
 * llcomp_mi_codec_decode_views_host stages for the unions); data[f] of an unused frame may be NULL and is never read.  Same bytes and
 * status as the device form on the same containers packed back to back.  Profile slots and n_decode as for one views decode. */
int llcomp_mi_codec_decode_warped_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                        const llcomp_mi_warp_group* groups, uint32_t n_groups, void* d_status, void* stream);
int llcomp_mi_codec_decode_warped_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                             const llcomp_mi_warp_group* groups, uint32_t n_groups, void* d_status, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes for warped views calls of up to total_views views with ow <= w, oh <= h: the boxes stay
 * within frames * w * h * c and there are no rows in between, but the staged block takes, per view, 64 bytes of entry, 4 * (w + h) of
 * index tables, c fill bytes and an output table (16 + 1024 * c): llcomp_mi_codec_workspace_bytes + 48 + max(total_views, 1) * (64 +
 * 4 * (w + h) + c + 16 + 1024 * c). */
uint64_t llcomp_mi_codec_warp_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
/* llcomp_mi_codec_decode_padded_views(_host) and llcomp_mi_codec_decode_warped_views(_host) with a photometric chain per view
 * (llcomp_mi_photo_chain / llcomp_mi_photo_group / the rule above).  photo: n_groups entries, photo[i].chains the n_views chains of
 * groups[i]; a NULL photo, a NULL chains and a group whose chains are all empty mean no chain: such a group takes the extended call's path
 * untouched, and with no chain at all the call writes exactly the bytes and the status of the call it extends.  pad (the padded form):
 * NULL = plain views, llcomp_mi_codec_decode_views exactly.
 * A group with a chain is resampled or warped by the extended call's kernels, unchanged, as U8 HWC into a staging buffer of the codec,
 * `chunk` views at a time where the group's n_views * oh * ow * c bytes would pass frames * w * h * c -- the buffer never grows past that
 * for ow <= w, oh <= h (one view always fits).  Then the chunk's views run their chains together, step by step on the stream, views with
 * shorter chains sitting out: a statistics pass where some view's op of that step needs one (per view, c histograms of 256 u32 and the sum
 * of L as u64, summed with integer atomics: the result does not depend on the order), one table [c][256] per view built from the
 * parameter and the statistics for every op but COLOR and GRAYSCALE, and a per-pixel pass in place.  A view's last step writes through the
 * group's output table and layout to d_out; a view with an empty chain in such a group is written by the first step, byte for byte as
 * the extended call writes it.  The chains cross in the call's ONE copy, behind the tail's block; nothing goes back to the host between
 * the steps.  d_status and the verdicts are the extended call's.  BAD_ARGS, before anything is queued or written (d_status untouched):
 * every case of the extended call, a photo[i].struct_size that is not the struct's, and the rule's limits.
 * _host: as the extended calls' _host forms; LLCOMP_MI_CTR_HOST_STAGED_BYTES counts what they count. */
int llcomp_mi_codec_decode_photo_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                       const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                                       const llcomp_mi_photo_group* photo, void* d_status, void* stream);
int llcomp_mi_codec_decode_photo_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                            const llcomp_mi_view_group* groups, uint32_t n_groups, const llcomp_mi_pad* pad,
                                            const llcomp_mi_photo_group* photo, void* d_status, void* stream);
int llcomp_mi_codec_decode_photo_warped_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                              const llcomp_mi_warp_group* groups, uint32_t n_groups, const llcomp_mi_photo_group* photo,
                                              void* d_status, void* stream);
int llcomp_mi_codec_decode_photo_warped_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                                   const llcomp_mi_warp_group* groups, uint32_t n_groups, const llcomp_mi_photo_group* photo,
                                                   void* d_status, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes for the four calls above with up to total_views views and ow <= w, oh <= h: the larger of
 * llcomp_mi_codec_padded_workspace_bytes and llcomp_mi_codec_warp_workspace_bytes for them, plus the staging buffer (frames * w * h * c),
 * and per view its statistics and table (8 + 1024 * c + 256 * c bytes) and its chain in the staged block (68 bytes, and 16 of alignment
 * per call). */
uint64_t llcomp_mi_codec_photo_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
/* llcomp_mi_codec_decode_warped_views(_host) with views that are projective maps (llcomp_mi_perspective_view /
 * llcomp_mi_perspective_group / the rule above): the same plan on the views' source rectangles (llcomp_mi_perspective_views_plan), the
 * same windows, classes, boxes, gather of a host source and ONE copy, and one gather kernel per group of 16 x 16 output pixels of one
 * view per workgroup, which computes the two quotients per pixel and reads the view straight from its frame's box.  A view's entry is
 * its eight coefficients (80 bytes with the box's origin); there are no index tables.  d_status, the verdicts, the BAD_ARGS cases (with
 * llcomp_mi_perspective_views_plan's) and the _host form: as for the warped views.  _photo_: with a photometric chain per view, as
 * llcomp_mi_codec_decode_photo_warped_views. */
int llcomp_mi_codec_decode_perspective_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes, const void* d_slice_len,
                                             const llcomp_mi_perspective_group* groups, uint32_t n_groups, void* d_status, void* stream);
int llcomp_mi_codec_decode_perspective_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                                  const llcomp_mi_perspective_group* groups, uint32_t n_groups, void* d_status, void* stream);
int llcomp_mi_codec_decode_photo_perspective_views(llcomp_mi_codec* codec, const void* d_payload, uint64_t payload_bytes,
                                                   const void* d_slice_len, const llcomp_mi_perspective_group* groups, uint32_t n_groups,
                                                   const llcomp_mi_photo_group* photo, void* d_status, void* stream);
int llcomp_mi_codec_decode_photo_perspective_views_host(llcomp_mi_codec* codec, const uint8_t* const* data, const size_t* lens,
                                                        const llcomp_mi_perspective_group* groups, uint32_t n_groups,
                                                        const llcomp_mi_photo_group* photo, void* d_status, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes for perspective views calls of up to total_views views with ow <= w, oh <= h:
 * llcomp_mi_codec_warp_workspace_bytes + 16 * max(total_views, 1), the longer entry.  With chains (the _photo_ calls):
 * llcomp_mi_codec_photo_workspace_bytes + 16 * max(total_views, 1) -- a form of its own, because taking this bound into
 * llcomp_mi_codec_photo_workspace_bytes' maximum would raise that function's value for its present callers. */
uint64_t llcomp_mi_codec_perspective_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
uint64_t llcomp_mi_codec_photo_perspective_workspace_bytes(const llcomp_mi_codec* codec, uint64_t total_views);
/* Batch mixing (the rule: "Batch mixing" above) in place on d_batch, n samples of the codec's c channels and ow x oh pixels in device
 * memory, asynchronously on `stream` -- behind the decode call that wrote the batch when that ran on the same stream.  One read and one
 * write per element at most: a sample that is its own partner writes its erase rectangle and nothing else, an element that keeps its
 * value is not written.  samples (n records) and erase_value (c floats or NULL) are HOST memory, read during the call only: they travel
 * with the plan in ONE copy from the codec's pinned ring into a device buffer of this call's own.  The heads of the segments of cut cycles
 * (llcomp_mi_mix_plan) are copied into a buffer of the codec's first.  BAD_ARGS, nothing queued: a NULL codec, d_batch or samples, a
 * d_batch that is not aligned to the element, and llcomp_mi_mix_reference's cases. */
int llcomp_mi_codec_mix_batch(llcomp_mi_codec* codec, void* d_batch, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                              const llcomp_mi_mix_sample* samples, const float* erase_value, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n samples of ow x oh among the codec's calls:
 * llcomp_mi_codec_workspace_bytes, the table (68 bytes per sample and 4 * c per call) and the saved heads: for n above
 * llcomp_mi_mix_segment(), 2 * n / (llcomp_mi_mix_segment() + 1) slots, each c * oh * ow elements rounded up to 16 bytes and 16 more.
 * 0 for a NULL codec or an unknown dtype. */
uint64_t llcomp_mi_codec_mix_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype);
/* Batch orientation (the rule: "Batch orientation" above) in place on d_batch, n samples of the codec's c channels and ow x oh pixels
 * in device memory, asynchronously on `stream` -- behind the decode call that wrote the batch when that ran on the same stream, and
 * ahead of llcomp_mi_codec_mix_batch.  No scratch in device memory: a workgroup reads the orbits of its pixels into LDS and writes
 * them back, so every element of an oriented sample is read once and written once at most; an element that is its own image is not
 * touched (the middle column of a mirror of odd width, the centre of an odd square) or, on the diagonal of a transposition, written
 * with the value it held; a sample with code 0 costs no workgroup.  codes (n bytes) is HOST memory, read during the call only: the oriented samples and their codes travel in ONE copy from
 * the codec's pinned ring into a device buffer of this call's own.  A call whose codes are all 0 queues nothing.  BAD_ARGS, nothing
 * queued: a NULL codec, d_batch or codes, a d_batch that is not aligned to the element, and llcomp_mi_orient_reference's cases. */
int llcomp_mi_codec_orient_batch(llcomp_mi_codec* codec, void* d_batch, uint32_t n, uint32_t ow, uint32_t oh, uint32_t dtype,
                                 uint32_t layout, const uint8_t* codes, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n samples among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 8 * n, the table of a call that orients every sample (8 bytes per oriented sample).  0 for a NULL
 * codec. */
uint64_t llcomp_mi_codec_orient_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n);
/* Batch composition (the rule: "Batch composition" above): rectangles of d_src, n_src samples of the codec's c channels and iw x ih
 * pixels, into d_dst, n_dst samples of ow x oh, both in device memory, asynchronously on `stream` -- behind the decode call that wrote
 * src when that ran on the same stream.  One kernel, no scratch in device memory: every dst element is written at most once (exactly
 * once without KEEP), in aligned 16-byte stores wherever a whole 16-byte unit of dst memory comes from one piece or from the fill; no
 * byte outside either batch is read or written.  Under KEEP a dst sample without pieces costs no workgroup, and a call with no piece of
 * w and h above 0 queues nothing.  pieces and fill_value are HOST memory, read during the call only: they travel with the plan in ONE
 * copy from the codec's pinned ring into a device buffer of this call's own.  d_src may be NULL with n_src == 0.  BAD_ARGS, nothing
 * queued: a NULL codec or d_dst, a NULL d_src with n_src > 0, a pointer that is not aligned to the element, byte ranges of the two
 * batches that overlap, and llcomp_mi_compose_plan's cases. */
int llcomp_mi_codec_compose_batch(llcomp_mi_codec* codec, const void* d_src, uint32_t n_src, uint32_t iw, uint32_t ih, void* d_dst,
                                  uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                  const llcomp_mi_compose_piece* pieces, uint32_t n_pieces, const float* fill_value, uint32_t flags,
                                  void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n_dst dst samples and n_pieces pieces among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 12 * n_dst + 32 * n_pieces + 4 * c, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_compose_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n_dst, uint32_t n_pieces);
/* Batch copy-paste (the rule: "Batch copy-paste" above): the pieces of d_src, n_src samples of the codec's c channels and iw x ih
 * pixels, that the id maps d_mask select, into d_dst, n_dst samples of ow x oh, all in device memory, asynchronously on `stream` --
 * behind the decode calls that wrote them when those ran on the same stream.  One kernel, no scratch in device memory: a dst element is
 * written at most once, and only if a piece selects it; no byte outside the three batches is read, none outside dst is written.  A dst
 * sample without a piece that is not ignored costs no workgroup, and a call without one queues nothing.  pieces is HOST memory, read
 * during the call only: the records travel with the plan in ONE copy from the codec's pinned ring into a device buffer of this call's
 * own.  BAD_ARGS, nothing queued: a NULL codec or d_dst, a NULL d_src or d_mask with n_pieces > 0, d_src or d_dst not aligned to the
 * element, a dst whose bytes overlap src's or mask's, and llcomp_mi_paste_plan's cases. */
int llcomp_mi_codec_paste_batch(llcomp_mi_codec* codec, const void* d_src, const void* d_mask, uint32_t n_src, uint32_t iw, uint32_t ih,
                                void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                const llcomp_mi_paste_piece* pieces, uint32_t n_pieces, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n_dst dst samples and n_pieces pieces among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 12 * n_dst + 68 * n_pieces, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_paste_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n_dst, uint32_t n_pieces);
/* Batch copy-paste by 16-bit ids (the rule: "Batch copy-paste by 16-bit ids" above): llcomp_mi_codec_paste_batch with d_mask the 16-bit
 * id maps, n_src x ih x iw uint16_t aligned to 2 bytes, and pieces of llcomp_mi_paste_piece16.  One kernel on the composition's tiles
 * and 16-byte units of dst memory; a unit's mask pixels come as shifted copies of the one to three aligned units of mask memory that
 * hold them.  BAD_ARGS, nothing queued: llcomp_mi_codec_paste_batch's cases, a d_mask not aligned to 2 bytes, and
 * llcomp_mi_paste16_plan's cases. */
int llcomp_mi_codec_paste_batch16(llcomp_mi_codec* codec, const void* d_src, const void* d_mask, uint32_t n_src, uint32_t iw, uint32_t ih,
                                  void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                  const llcomp_mi_paste_piece16* pieces, uint32_t n_pieces, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n_dst dst samples and n_pieces pieces among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 12 * n_dst + 72 * n_pieces, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_paste16_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n_dst, uint32_t n_pieces);
/* Label boxes (the rule: "Label boxes" above): the 256 records of each of the n id maps at d_maps, oh x ow bytes each whatever the
 * codec's c, into d_boxes, n * 256 records in device memory, asynchronously on `stream`.  The codec gives the device and nothing else:
 * no table, no workspace.  Two kernels: one writes the identities, one has a workgroup per band of llcomp_mi_label_boxes_rows() rows of
 * a sample, which merges its records into d_boxes with integer atomics, so the result does not depend on order.  BAD_ARGS, nothing
 * queued: a NULL codec, the reference's cases, d_boxes not aligned to 4, d_boxes overlapping the maps. */
int llcomp_mi_codec_label_boxes(llcomp_mi_codec* codec, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, void* d_boxes, void* stream);
/* Label boxes of listed ids (the rule: "Label boxes of listed ids" above): the first[n] records of the ids listed for the n 16-bit id
 * maps at d_maps, oh x ow uint16_t each whatever the codec's c, into d_boxes in device memory, asynchronously on `stream`.  ids and
 * first are HOST memory, read during the call only: they travel in ONE copy from the codec's pinned ring into a device buffer of this
 * call's own.  Two kernels: one writes the identities, one has a workgroup per band of llcomp_mi_label_boxes_rows() rows of a LISTED
 * sample, which holds the sample's list and records in LDS (capacities of 256, 1024 and 4096 ids: the call runs the smallest that
 * holds its longest list), finds every run's id by binary search, and merges into d_boxes with integer atomics, so the result does
 * not depend on order.  A call with first[n] == 0 queues nothing.  BAD_ARGS, nothing queued and nothing written: a NULL codec, the
 * reference's cases, d_boxes not aligned to 4, records that overlap the maps. */
int llcomp_mi_codec_label_boxes16(llcomp_mi_codec* codec, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh, const uint16_t* ids,
                                  const uint32_t* first, void* d_boxes, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n samples and total_ids listed ids among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 4 * (2 * n + 1) + 2 * total_ids, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_label_boxes16_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n, uint32_t total_ids);
/* Label targets (the rule: "Label targets" above): the index tensor or the planes of the n id maps at d_maps, oh x ow pixels each
 * whatever the codec's c, into d_out in device memory, asynchronously on `stream`.  The arrays of `targets` are HOST memory, read
 * during the call only: first, the samples that get workgroups, plane_first, the values and the ids travel in ONE copy from the
 * codec's pinned ring into a device buffer of this call's own.  One kernel: a workgroup per segment of
 * llcomp_mi_label_targets_segment() pixels of a sample (PLANES: and per chunk of 32 of its planes) holds the sample's table in LDS (a
 * dense table of 256 values for map_bytes 1; the list and its values at capacities of 256, 1024 and 4096 ids for map_bytes 2), reads
 * the segment's map pixels once in aligned 16-byte units, leaves their values in LDS, and writes the aligned 16-byte units of output
 * memory that the segment covers with one 16-byte store each; a unit covered in part gets exactly its own elements.  INDEX: every
 * sample gets workgroups; PLANES: a sample without planes costs none, a call without planes queues nothing.
 * BAD_ARGS, nothing queued and nothing written: a NULL codec, d_maps or d_out, the reference's cases, an output that overlaps the maps. */
int llcomp_mi_codec_label_targets(llcomp_mi_codec* codec, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh,
                                  const llcomp_mi_label_targets* targets, void* d_out, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n samples and total_ids listed ids among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 4 * (3 * n + 2) + 6 * total_ids, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_label_targets_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n, uint32_t total_ids);
/* Wide id maps (the rule: "Wide id maps" above): llcomp_mi_codec_label_boxes16 and llcomp_mi_codec_label_targets for maps of 3 or 4
 * bytes per pixel, with the same kernels' bands, segments, capacities and merges.  A listed id takes 24 bytes of a workgroup's LDS for
 * the boxes (96 KiB at 4096 ids: still one workgroup to a CU) and 8 for the targets.  A thread takes the aligned 16-byte units of map
 * memory as before; a 3-byte pixel belongs to the unit that holds its first byte, and the thread reads the last bytes of a pixel that
 * straddles, at most two, from the next unit -- five or six pixels to a unit.  The tables travel in the 16-bit calls' buffers.
 * BAD_ARGS, nothing queued and nothing written: the 16-bit calls' cases and the references'. */
/* ... and llcomp_mi_codec_paste_batch16 for them: k_paste<3|4, ES> on the composition's tiles and units; a unit's npx mask pixels are
 * map_bytes * npx bytes, one to four (3) or one to five (4) aligned mask units; the table travels in the 16-bit call's buffer, and the
 * bound is llcomp_mi_codec_paste16_workspace_bytes's. */
int llcomp_mi_codec_paste_batch32(llcomp_mi_codec* codec, const void* d_src, const void* d_mask, uint32_t map_bytes, uint32_t n_src, uint32_t iw,
                                  uint32_t ih, void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype, uint32_t layout,
                                  const llcomp_mi_paste_piece32* pieces, uint32_t n_pieces, void* stream);
uint64_t llcomp_mi_codec_paste32_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n_dst, uint32_t n_pieces);
int llcomp_mi_codec_label_boxes32(llcomp_mi_codec* codec, const void* d_maps, uint32_t map_bytes, uint32_t n, uint32_t ow, uint32_t oh,
                                  const uint32_t* ids, const uint32_t* first, void* d_boxes, void* stream);
/* llcomp_mi_codec_workspace_bytes + 4 * (2 * n + 1) + 4 * total_ids, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_label_boxes32_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n, uint32_t total_ids);
int llcomp_mi_codec_label_targets32(llcomp_mi_codec* codec, const void* d_maps, uint32_t n, uint32_t ow, uint32_t oh,
                                    const llcomp_mi_label_targets32* targets, void* d_out, void* stream);
/* llcomp_mi_codec_workspace_bytes + 4 * (3 * n + 2) + 8 * total_ids, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_label_targets32_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n, uint32_t total_ids);
/* Batch alpha paste (the rule: "Batch alpha paste" above) on device memory, in place on d_dst, asynchronous on `stream`, in ONE kernel
 * with no scratch in device memory: k_alpha_paste<AB, DT> on the composition's tiles and 16-byte units of dst memory.  A workgroup
 * filters its sample's pieces against its tile into a short list in LDS (36-byte records, 9 KiB, and the 256 weights); a thread loads
 * its unit of dst once, walks the list forwards -- per piece the alpha bytes of the unit's pixels as shifted copies of the aligned
 * alpha units that hold them, the src unit as one shifted copy, the blend -- and stores the unit once: 16 bytes where the pieces
 * reach all of its elements, the reached elements one by one otherwise.  No byte outside dst is written, none outside src or alpha
 * read; a dst element that no piece reaches is not written, one whose alphas are all 0 keeps its bits.  Calls with an OVER piece run an
 * instantiation of their own, so that the division costs the others no register.  The table travels in a buffer of its own, allocated
 * by the first such call.  A call without a piece that has w and h queues nothing.
 * BAD_ARGS, nothing queued and nothing written: a NULL codec or d_dst, the reference's cases.  NOMEM before anything is queued. */
int llcomp_mi_codec_alpha_paste_batch(llcomp_mi_codec* codec, const void* d_src, const void* d_alpha, uint32_t alpha_px_bytes, uint32_t alpha_byte,
                                      uint32_t n_src, uint32_t iw, uint32_t ih, void* d_dst, uint32_t n_dst, uint32_t ow, uint32_t oh, uint32_t dtype,
                                      uint32_t layout, const llcomp_mi_alpha_piece* pieces, uint32_t n_pieces, void* stream);
/* The bound on llcomp_mi_codec_allocated_bytes with such calls of up to n_dst dst samples and n_pieces pieces among the codec's calls:
 * llcomp_mi_codec_workspace_bytes + 12 * n_dst + 36 * n_pieces, the table of a call.  0 for a NULL codec. */
uint64_t llcomp_mi_codec_alpha_paste_workspace_bytes(const llcomp_mi_codec* codec, uint32_t n_dst, uint32_t n_pieces);
/* Stage-A only (context + prediction model), for tests and profiling: d_sym u32[frames*h*w*c],
 * low 16 bits = folded context (0..7925), high 16 bits = folded residual (two's complement). */
int llcomp_mi_codec_model(llcomp_mi_codec* codec, const void* d_px, void* d_sym, void* stream);
/* Device-side concatenator (multi-GPU sharding: the gathering rank interleaves the ranks' packed payloads into image
 * order): copies n_seg byte ranges src[src_off[i] .. +len[i]) -> dst[dst_off[i] .. +len[i]) in one launch.  All five
 * pointers are device memory (offsets / lengths: u64[n_seg], computed on the GPU, 8-byte aligned); the byte ranges have any alignment
 * and must not overlap.  max_len = an upper bound of the lengths (sizes the grid only: the bytes copied do not depend on it);
 * n_seg <= 65535 (0: nothing is done; more: BAD_ARGS, nothing is launched).  Asynchronous on `stream`. */
int llcomp_mi_device_copy_segments(const void* d_src, void* d_dst, const void* d_src_off, const void* d_dst_off,
                                   const void* d_len, uint32_t n_seg, uint64_t max_len, void* stream);
/* Sums over ranges of a u32 table in HBM: d_out[i] (u64) = sum of min(d_vals[j], cap) for j in [d_start[i], d_start[i] + d_count[i])
 * (d_start, d_count: u64[n] in HBM).  The multi-GPU path derives the byte counts of its (image, chunk) segments from the
 * slice-length tables with it.  Asynchronous on `stream`. */
int llcomp_mi_device_range_sums(const void* d_vals, const void* d_start, const void* d_count, void* d_out, uint32_t n, uint32_t cap,
                                void* stream);
/* The u32 status word written by encode/decode holds bit flags (1 overflow, 2 bad exponent, 4 truncated);
 * this maps it to an llcomp_mi_status. */
uint32_t llcomp_mi_status_from_bits(uint32_t bits);
/* Event counters of a codec object: what the rare and the adaptive paths of its kernels actually did, cumulative since creation (or
 * the last reset).  The kernels add to them with one atomic per wavefront -- and only wavefronts that have something to report -- so
 * they cost nothing measurable and are always on.  Tests use them to prove that a branch ran (parity passes either way); a caller can
 * watch the bank cache's hit rate on its content.  get_counters waits for the codec's last call (its own event, not the device),
 * writes the first n (<= LLCOMP_MI_CTR_COUNT) counters and clears all of them when reset != 0. */
enum {
    LLCOMP_MI_CTR_DEC_CACHED_WAVES = 0,    /* 2-D decoder (state tables in HBM): wavefronts that started with the bank cache in LDS */
    LLCOMP_MI_CTR_DEC_BYPASSED_WAVES = 1,  /* ... of those, the ones that gave it up (fewer than one hit in eight over four rows) */
    LLCOMP_MI_CTR_CACHE_LOOKUPS = 2,       /* state-bank look-ups in the cache (one per decoded sample while the cache is in use) */
    LLCOMP_MI_CTR_CACHE_MISSES = 3,        /* ... that missed: a 64-byte line fill from the table in HBM */
    LLCOMP_MI_CTR_CACHE_WRITEBACKS = 4,    /* victims written back to the table (one 32-byte sector each) */
    LLCOMP_MI_CTR_DEC_REPLAYS = 5,         /* decoded samples that ran out of window bytes (or saw an invalid exponent) on the fast path
                                              and went through rollback + checked replay (llcomp.hpp:219-247 is the checked form) */
    LLCOMP_MI_CTR_ENC_CARRY_BACKS = 6,     /* encoder: carries into a held 0xFF byte that went on into bytes already stored to HBM
                                              (the reference's outstanding_count run, llcomp.hpp:40-57, resolved eagerly) */
    LLCOMP_MI_CTR_GENERATION_WRAPS = 7,    /* state tables cleared because the 8-bit generation tag ran out (every 255 calls) */
    LLCOMP_MI_CTR_DEC_LAUNCHES_CACHED = 8, /* 2-D decode launches that ran with the bank cache */
    LLCOMP_MI_CTR_DEC_LAUNCHES_PLAIN = 9,  /* ... and without it, because (nearly) every wavefront of the last cached launch had given
                                              it up: the plain kernel holds no LDS for a cache nobody uses; re-probed every 16th call */
    LLCOMP_MI_CTR_HOST_STAGED_BYTES = 10,  /* payload bytes llcomp_mi_codec_decode_regions_host copied to the GPU (host-side count) */
    LLCOMP_MI_CTR_BIAS_LAUNCHES = 11,      /* resample launches of the padded calls that ran the kernels' bias forms: a chunk with an entry
                                              whose constant fill other than 0 has weight (host-side count) */
    LLCOMP_MI_CTR_COUNT = 16
};
int llcomp_mi_codec_get_counters(llcomp_mi_codec* codec, uint64_t* out, uint32_t n, int reset);
/* Per-kernel timing with hipEvents recorded on the caller's stream around each launch (bench.py's roofline leg).
 * get_profile drains the stream, adds up the milliseconds since the last call and resets:
 *   ms[0] state-table clear -- or, where the 2-D encoder replays its states ahead of the coder (slices of several rows and
 *         at most 4096 samples), the state snapshot pass that replaces the tables: k_snap_sort + _walk + _unperm
 *   ms[1] stage A (k_model_*)  ms[2] k_encode_slices  ms[3] k_scan_groups + k_pack_payload
 *   ms[4] k_group_sums + k_scan_groups + k_stage_streams (decode)  ms[5] k_decode_slices  ms[6] stage A inverse
 *   ms[7] state-table clear (decode) */
int llcomp_mi_codec_set_profiling(llcomp_mi_codec* codec, int enable);
int llcomp_mi_codec_get_profile(llcomp_mi_codec* codec, double* ms8, uint32_t* n_encode, uint32_t* n_decode);

/* ---- streaming pipeline: frames of one shape, host -> GPU -> host, several jobs in flight (BASELINE config 5) ------- */
/* The reference codes one image in RAM per call (llcompc.cpp:25-41, llcompd.cpp:17-31); this is the same operation as a
 * pipeline.  `depth` slots (1..16), each with its own codec object, HIP stream, HBM buffers and a pinned output buffer;
 * a job is one frame (SLICED container).  submit_* returns at once: LLCOMP_MI_OK, or LLCOMP_MI_BUSY when every slot is
 * occupied (back-pressure: take a result and release it).  `px` / `data` must stay valid until the job's result has
 * been returned by llcomp_mi_stream_wait (except for llcomp_mi_stream_submit_decode_regions, which reads them during the call only); pinned memory (llcomp_mi_host_alloc, or the `data` of an earlier result that
 * has not been released) is copied by DMA while other jobs compute.  Results come back in submission order.  A
 * container that needs more than 2x the raw size fails with OUTPUT_OVERFLOW (llcomp_mi_encode handles such a frame).
 * One object is driven by one thread at a time (calls are serialised internally). */
typedef struct llcomp_mi_stream llcomp_mi_stream;
enum { LLCOMP_MI_JOB_ENCODE = 0, LLCOMP_MI_JOB_DECODE = 1, LLCOMP_MI_JOB_DECODE_REGIONS = 2, LLCOMP_MI_JOB_DECODE_RESIZED_REGIONS = 3 };
typedef struct llcomp_mi_stream_result {
    uint32_t slot;       /* hand back with llcomp_mi_stream_release when `data` is no longer needed */
    uint32_t kind;       /* LLCOMP_MI_JOB_ENCODE: data = container, LLCOMP_MI_JOB_DECODE: data = h*w*c pixels,
                            LLCOMP_MI_JOB_DECODE_REGIONS: data = frames_per_job crops of rh*rw*c pixels,
                            LLCOMP_MI_JOB_DECODE_RESIZED_REGIONS: data = frames_per_job outputs of oh*ow*c pixels */
    int32_t status;      /* llcomp_mi_status of this job */
    uint32_t reserved;
    uint64_t tag;        /* the caller's tag from submit */
    const uint8_t* data; /* pinned host memory owned by the stream object; NULL when status != OK */
    uint64_t len;
} llcomp_mi_stream_result;
int llcomp_mi_stream_create(llcomp_mi_stream** stream, int32_t device, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w,
                            uint32_t tile_h, uint32_t planar, uint32_t depth);
/* Jobs of `frames_per_job` (1..64) frames: larger launches for the GPU, larger copies for the link.  submit_encode then
 * takes frames_per_job frames back to back, llcomp_mi_stream_submit_decode_batch that many containers; a result describes
 * the whole job (encode: all containers back to back, decode: all frames back to back) and llcomp_mi_stream_result_part
 * hands out container / frame f of a result that has been returned by wait and not yet released. */
int llcomp_mi_stream_create_ex(llcomp_mi_stream** stream, int32_t device, uint32_t w, uint32_t h, uint32_t c, uint32_t tile_w,
                               uint32_t tile_h, uint32_t planar, uint32_t depth, uint32_t frames_per_job);
/* The same pipeline over a device list (BASELINE config 5 "round-robin over the GPUs"): one pipeline of `depth` slots PER
 * DEVICE behind one object; jobs are dealt round-robin (a device whose slots are all occupied is skipped; BUSY when all are), results
 * still come back in submission order, every other call of this section works on the object unchanged (`slot` values are opaque).
 * An ordinal may repeat.  1 <= n_devices <= LLCOMP_MI_MAX_DEVICES.  A device that cannot be set up fails the call with
 * LLCOMP_MI_DEVICE_FAILED (llcomp_mi_last_device_error). */
int llcomp_mi_stream_create_multi(llcomp_mi_stream** stream, const int32_t* devices, uint32_t n_devices, uint32_t w, uint32_t h, uint32_t c,
                                  uint32_t tile_w, uint32_t tile_h, uint32_t planar, uint32_t depth, uint32_t frames_per_job);
uint32_t llcomp_mi_stream_devices(const llcomp_mi_stream* stream); /* pipelines behind the object (1 for a plain stream) */
uint32_t llcomp_mi_stream_frames_per_job(const llcomp_mi_stream* stream);
int llcomp_mi_stream_submit_decode_batch(llcomp_mi_stream* stream, const uint8_t* const* data, const size_t* lens, uint64_t tag);
int llcomp_mi_stream_result_part(llcomp_mi_stream* stream, uint32_t slot, uint32_t frame, const uint8_t** data, uint64_t* len);
void llcomp_mi_stream_destroy(llcomp_mi_stream* stream);
uint64_t llcomp_mi_stream_container_capacity(const llcomp_mi_stream* stream); /* largest container a slot can return */
int llcomp_mi_stream_submit_encode(llcomp_mi_stream* stream, const uint8_t* px, uint64_t tag);
int llcomp_mi_stream_submit_decode(llcomp_mi_stream* stream, const uint8_t* data, size_t len, uint64_t tag);
/* A job of crops: frames_per_job containers (data[f], lens[f]) and frame f's rectangle (xy[2f], xy[2f + 1], rw, rh).  The slot's codec
 * runs llcomp_mi_codec_decode_regions_host on the slot's stream (only the windows' bytes cross PCIe), then the crops come back:
 * kind = LLCOMP_MI_JOB_DECODE_REGIONS, len = frames_per_job * rw * rh * c, dense [frames][rh][rw][c], and llcomp_mi_stream_result_part
 * hands out crop f.  UNLIKE the other submits, the containers and xy are read during the call only: they may be reused as soon as it
 * returns.  A gather error is the call's return value (nothing is queued).  Region jobs and whole-frame jobs mix in one object. */
int llcomp_mi_stream_submit_decode_regions(llcomp_mi_stream* stream, const uint8_t* const* data, const size_t* lens, const uint32_t* xy,
                                           uint32_t rw, uint32_t rh, uint64_t tag);
/* A job of resized crops: frames_per_job containers, frame f's rectangle rects[4f .. 4f + 3] = {x, y, rw, rh} and flags[f] (NULL = none),
 * resampled to ow x oh (llcomp_mi_codec_decode_resized_regions_host on the slot's codec and stream): kind =
 * LLCOMP_MI_JOB_DECODE_RESIZED_REGIONS, len = frames_per_job * oh * ow * c, and llcomp_mi_stream_result_part hands out frame f.  The
 * output has to fit a slot: a job of more than frames_per_job * w * h * c bytes (llcomp_mi_stream_container_capacity bounds the slot's
 * pinned buffer) is BAD_ARGS at submit.  Containers, rects and flags are read during the call only, as for
 * llcomp_mi_stream_submit_decode_regions. */
int llcomp_mi_stream_submit_decode_resized_regions(llcomp_mi_stream* stream, const uint8_t* const* data, const size_t* lens, const uint32_t* rects,
                                                   const uint8_t* flags, uint32_t ow, uint32_t oh, uint64_t tag);
/* ... with an output format (NULL = the call above exactly): len = frames_per_job * oh * ow * c * the dtype's size, in fmt's layout, and
 * a job of more than frames_per_job * w * h * c bytes is BAD_ARGS at submit.  fmt, mean and std are read during the call only. */
int llcomp_mi_stream_submit_decode_resized_regions_ex(llcomp_mi_stream* stream, const uint8_t* const* data, const size_t* lens,
                                                      const uint32_t* rects, const uint8_t* flags, uint32_t ow, uint32_t oh,
                                                      const llcomp_mi_output_format* fmt, uint64_t tag);
int llcomp_mi_stream_pending(llcomp_mi_stream* stream); /* jobs submitted and not yet returned by wait */
/* LLCOMP_MI_OK when llcomp_mi_stream_wait would not block (or nothing is pending), LLCOMP_MI_BUSY otherwise. */
int llcomp_mi_stream_poll(llcomp_mi_stream* stream);
/* Blocks until the OLDEST pending job has finished and describes it; BAD_ARGS when nothing is pending.  Single consumer:
 * wait / release / destroy of one pipeline object come from one thread (submits may come from another); the object's lock
 * is released while wait blocks. */
int llcomp_mi_stream_wait(llcomp_mi_stream* stream, llcomp_mi_stream_result* result);
int llcomp_mi_stream_release(llcomp_mi_stream* stream, uint32_t slot);

#ifdef __cplusplus
}
#endif
#endif
