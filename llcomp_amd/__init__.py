"""llcomp_amd -- host-side mirror (Python, for tests / bench / scripting) of the MI355X-native llcomp coding path.

The product is libllcomp_mi.so (hand-written HIP kernels for gfx950 behind the C ABI of include/llcomp_mi.h);
include/llcomp_mi.hpp is the C++ drop-in with the reference's own signatures.  This module binds the same C ABI
with ctypes and keeps the reference's names and error behaviour:

    compress_image(rgb, width, height, channels)  <->  llcomp::compressImage    (/root/reference/llcomp.hpp:358)
    decompress_image(data) -> RawImage            <->  llcomp::decompressImage  (/root/reference/llcomp.hpp:461)
    decompress_region(data, x, y, w, h)           <->  llcomp::decompressRegion (include/llcomp_mi.hpp: one rectangle, covered slices only)
    update_region(data, x, y, patch)              <->  llcomp::updateRegion     (the write side: only the covered tiles are coded again)
    replace_slices / Codec.encode_region / Codec.update_region  (the host-only splice, and the update of a batch in HBM)
    regions_plan(w, h, c, tw, th, planar, rw, rh, xy) / Codec.decode_regions  (a rectangle per frame of a batch; pack_batch feeds it)
    regions_gather / Codec.decode_regions_host / Stream.submit_decode_regions  (the same from host containers: only the windows cross)
    resize_weights / resized_regions_plan / Codec.decode_resized_regions(_host) / Stream.submit_decode_resized_regions  (a rectangle of
        its own size per frame, resampled to one output shape with an optional mirror: RandomResizedCrop + RandomHorizontalFlip;
        filter= chooses PIL's bilinear, box, hamming, bicubic or lanczos, or nearest for label images, for the call or per frame)
    output_table / dtype=, layout=, scale=, mean=, std= of the three resized calls  (their output as a model takes it: float32, float16
        or bfloat16, CHW or HWC, ToTensor() + Normalize(mean, std) -- the _ex calls and llcomp_mi_output_format)
    views_plan / ViewGroup / Codec.decode_views(_host) / Codec.views_workspace_bytes  (several views of each frame in one call, each
        frame decoded once: a view = (frame, x, y, rw, rh, flags), a group = views that share one output shape, format and buffer --
        multi-crop (2 x 224 + 8 x 96) and two-view training; a frame decodes the bounding box of its views)
    PAD_* / pad_axis / padded_weights / padded_regions_plan / pad_mode=, fill= of Codec.decode_resized_regions(_host) and
        Codec.decode_views(_host) / Codec.padded_workspace_bytes  (crops that leave the image -- RandomCrop(padding=...), pad_if_needed, a
        CenterCrop larger than the picture, a translate: rectangles and view origins may be negative, the outside is np.pad's
        "constant" (with fill), "edge", "reflect" or "symmetric", and only the part inside the image is decoded)
    WarpGroup / warp_source_rect / warp_views_plan / warp_reference / rotate_matrix / Codec.decode_warped_views(_host) /
        Codec.warp_workspace_bytes  (views under an affine map: a view = (frame, m0..m5[, flags]), byte for byte PIL's
        Image.transform(AFFINE) -- Image.rotate, RandomRotation, RandomAffine -- under nearest, bilinear or bicubic; a frame decodes
        the bounding box of the source pixels its views read)
    PerspectiveGroup / perspective_source_rect / perspective_views_plan / perspective_reference / perspective_coeffs /
        Codec.decode_perspective_views(_host) / Codec.perspective_workspace_bytes  (views under a projective map: a view =
        (frame, a0..a7[, flags]), byte for byte PIL's Image.transform(PERSPECTIVE) -- RandomPerspective -- under the same three filters)
    mix_samples / mix_plan / mix_reference / Codec.mix_batch / Codec.mix_workspace_bytes  (RandomErasing, MixUp and CutMix in place on
        the float batch a decode call wrote, bit for bit torch's expressions on the CPU)
    ORIENT_* / orient_code / orient_reference / Codec.orient_batch / Codec.orient_workspace_bytes  (a flip, quarter turn or transposition
        per sample, in place on the batch a decode call wrote: RandomVerticalFlip, PIL's Image.transpose, np.rot90)
    COMPOSE_FILL / COMPOSE_KEEP / compose_pieces / compose_plan / compose_tile / compose_reference / grid_pieces / mosaic_pieces /
        Codec.compose_batch / Codec.compose_workspace_bytes  (rectangles of one decoded batch into the canvases of another, the rest a
        fill or kept: Mosaic, make_grid, batch_images, Cutout with several holes, GridMask)
    PASTE_VALUE / paste_pieces / paste_plan / paste_reference / paste_max_pieces_per_sample / Codec.paste_batch /
        Codec.paste_workspace_bytes  (the objects of one decoded sample into another, chosen by the ids of an id map: Simple Copy-Paste)
    PastePiece16 / paste_pieces16 / paste16_plan / paste16_reference / Codec.paste_batch16 / Codec.paste16_workspace_bytes  (the same
        selected by a 16-bit id map, a piece a window of 256 ids from id_base on: Cityscapes, Mapillary Vistas, ADE20K instance ids)
    LABEL_BOX_DTYPE / label_boxes_reference / label_boxes_rows / Codec.label_boxes  (the pixel count and bounding box of each of the 256
        ids of every id map of a batch: torchvision's masks_to_boxes)
    label_boxes16_reference / label_boxes16_max_ids / Codec.label_boxes16 / Codec.label_boxes16_workspace_bytes  (the same for the ids
        the caller lists per sample, in 16-bit id maps: Cityscapes, Mapillary Vistas, ADE20K instance ids)
    PastePiece32 / PASTE_VALUE_PIXEL / paste_pieces32 / paste32_plan / paste32_reference / Codec.paste_batch32 /
        Codec.paste32_workspace_bytes  (the copy-paste selected by id maps of 3 or 4 bytes per pixel; VALUE_PIXEL writes a 3-byte id)
    AlphaPiece / ALPHA_VALUE / ALPHA_VALUE_PIXEL / ALPHA_OVER / alpha_pieces / alpha_paste_plan / alpha_paste_reference /
        Codec.alpha_paste_batch / Codec.alpha_paste_workspace_bytes  (pieces blended under a per-pixel alpha byte: PIL's paste with a
        mask, Image.composite and Image.alpha_composite, byte for byte; floats as torch's d * (1 - a) + s * a)
    label_boxes32_reference / label_targets32_reference / Codec.label_boxes32 / Codec.label_targets32 / their _workspace_bytes  (both
        for id maps of 3 or 4 bytes per pixel: COCO panoptic's RGB ids, int32 class * 1000 + instance maps)
    TARGET_* / label_targets_reference / label_targets_segment / label_targets_max_planes / Codec.label_targets /
        Codec.label_targets_workspace_bytes  (what a loss takes from the id maps: lut[map] as a class-index tensor, one-hot planes with
        label smoothing, one binary mask per listed instance)
    RawImage(pixels, width, height, channels)     <->  llcomp::RawImage         (/root/reference/llcomp.hpp:454-459)
    EXT = ".llcomp"                               <->  llcomp::ext              (/root/reference/llcomp.hpp:18)

Errors: the reference throws std::runtime_error("Invalid magic number") / ("Invalid exponent"); here LlcompError
carries the same message text plus the C status code.  There is no CPU fallback anywhere in this package.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import Info, Opts, OutputFormat
from ._lib import Pad as _Pad
from ._lib import View as _View, ViewGroup as _ViewGroup
from ._lib import WarpView as _WarpView, WarpGroup as _WarpGroup
from ._lib import PerspectiveView as _PerspectiveView, PerspectiveGroup as _PerspectiveGroup
from ._lib import PhotoOp as _PhotoOp, PhotoChain as _PhotoChain, PhotoGroup as _PhotoGroup
from ._lib import ComposePiece as _ComposePiece
from ._lib import PastePiece as _PastePiece
from ._lib import PastePiece16, PastePiece32
from ._lib import AlphaPiece
from ._lib import MixSample as _MixSample

EXT = ".llcomp"
FORMAT_LEGACY, FORMAT_SLICED = 0, 1
(OK, BAD_MAGIC, BAD_EXPONENT, TRUNCATED, BAD_ARGS, OUT_OF_RANGE, OUTPUT_OVERFLOW, HIP_ERROR, NO_DEVICE, NOMEM, BUSY, DEVICE_FAILED) = range(12)
JOB_ENCODE, JOB_DECODE, JOB_DECODE_REGIONS, JOB_DECODE_RESIZED_REGIONS = 0, 1, 2, 3
DTYPE_U8, DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2, 3
LAYOUT_HWC, LAYOUT_CHW = 0, 1
# the resampling filters of the resized calls (LLCOMP_MI_FILTER_*): PIL's, and NEAREST for label images
FILTER_BILINEAR, FILTER_NEAREST, FILTER_BOX, FILTER_HAMMING, FILTER_BICUBIC, FILTER_LANCZOS = range(6)
FILTER_NAMES = ("bilinear", "nearest", "box", "hamming", "bicubic", "lanczos")
FLAG_MIRROR, FLAG_FILTER_SHIFT = 1, 4
# what stands outside the image in a padded call (LLCOMP_MI_PAD_*): numpy's np.pad modes and torchvision's padding_mode of these names
PAD_CONSTANT, PAD_EDGE, PAD_REFLECT, PAD_SYMMETRIC = range(4)
PAD_NAMES = ("constant", "edge", "reflect", "symmetric")
# photometric ops (LLCOMP_MI_PHOTO_*; include/llcomp_mi.h "Photometric chains")
(PHOTO_BRIGHTNESS, PHOTO_CONTRAST, PHOTO_COLOR, PHOTO_GRAYSCALE, PHOTO_INVERT, PHOTO_SOLARIZE, PHOTO_POSTERIZE, PHOTO_AUTOCONTRAST,
 PHOTO_EQUALIZE) = range(9)
PHOTO_MAX_OPS = 8
PHOTO_NAMES = ("brightness", "contrast", "color", "grayscale", "invert", "solarize", "posterize", "autocontrast", "equalize")
# the two ops outside the pointwise family 0..8, under torchvision's functional names: PIL's ImageFilter.GaussianBlur(radius) and
# adjust_hue(hue_factor); and adjust_sharpness(sharpness_factor), PIL's ImageEnhance.Sharpness (code 18 is no op)
PHOTO_GAUSSIAN_BLUR, PHOTO_ADJUST_HUE = 16, 17
PHOTO_ADJUST_SHARPNESS = 19
PHOTO_MAX_RADIUS = 32
PHOTO_MORE_NAMES = {"gaussian_blur": PHOTO_GAUSSIAN_BLUR, "adjust_hue": PHOTO_ADJUST_HUE, "adjust_sharpness": PHOTO_ADJUST_SHARPNESS}

RawImage = namedtuple("RawImage", "pixels width height channels")


class LlcompError(RuntimeError):
    def __init__(self, status, detail=None):
        self.status = int(status)
        msg = _lib.load().llcomp_mi_strerror(int(status)).decode()
        # a call over a device list: (HIP ordinal, position in the list, that device's own status)
        self.device_error = last_device_error() if self.status == DEVICE_FAILED else None
        super().__init__(msg if not detail else f"{msg} ({detail})")


def _check(rc):
    if rc != OK:
        raise LlcompError(rc)


def last_device_error():
    """(HIP ordinal, position in the device list, that device's own status) behind this thread's last DEVICE_FAILED, else None"""
    dev, idx, st = C.c_int32(), C.c_uint32(), C.c_int()
    if not _lib.load().llcomp_mi_last_device_error(C.byref(dev), C.byref(idx), C.byref(st)):
        return None
    return dev.value, idx.value, st.value


def _opts(format, tile_w, tile_h, planar, device, small_model, devices=None, chunks_per_device=0):
    """llcomp_mi_opts (+ the int32 array its `devices` points at: keep it alive for the call)"""
    o = Opts(C.sizeof(Opts), format, tile_w, tile_h, int(bool(planar)), device, int(bool(small_model)), 0, None, int(chunks_per_device), 0)
    arr = None
    if devices is not None:
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        o.n_devices, o.devices = len(devices), C.cast(arr, C.POINTER(C.c_int32))
    return o, arr


def plan_chunks(height, tile_h, n_parts, chunks_per_part=4):
    """[(tile_row0, tile_row1, owner)] -- llcomp_mi_plan_chunks, the one work split of every multi-GPU path (device lists in the
    library, ranks in llcomp_amd.sharding)"""
    L = _lib.load()
    n = C.c_uint32()
    _check(L.llcomp_mi_plan_chunks(height, max(0, tile_h), n_parts, max(1, chunks_per_part), None, 0, C.byref(n)))
    tri = (C.c_uint32 * (3 * n.value))()
    _check(L.llcomp_mi_plan_chunks(height, max(0, tile_h), n_parts, max(1, chunks_per_part), tri, n.value, C.byref(n)))
    return [(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2]) for i in range(n.value)]


def device_count():
    return _lib.load().llcomp_mi_device_count()


def compress_image(rgb, width, height, channels, *, format=FORMAT_LEGACY, tile_w=0, tile_h=0, planar=False, device=-1, small_model=False,
                   devices=None, chunks_per_device=0):
    """bytes of an llcomp stream.  Default = the reference's own whole-image format (magic 0x79), byte-identical to
    llcomp::compressImage; format=FORMAT_SLICED produces the parallel container (magic 0x9C).  small_model=True codes like
    a reference built with LargeModel = false (llcomp.hpp:21); a legacy stream does not record that, so it must be passed
    to decompress_image as well.  devices=[ordinals]: the image's tile rows are dealt over these GPUs inside this process
    (llcomp_mi_opts.devices; the container is byte-identical to the one-device container)."""
    L = _lib.load()
    buf = np.ascontiguousarray(np.frombuffer(rgb, dtype=np.uint8) if isinstance(rgb, (bytes, bytearray, memoryview)) else rgb, dtype=np.uint8).reshape(-1)
    if buf.size != width * height * channels:  # the reference only asserts this (llcomp.hpp:361)
        raise LlcompError(BAD_ARGS)
    o, _keep = _opts(format, tile_w, tile_h, planar, device, small_model, devices, chunks_per_device)
    out, n = _lib.u8p(), C.c_size_t()
    _check(L.llcomp_mi_encode(buf.ctypes.data_as(_lib.u8p), width, height, channels, C.byref(o), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        L.llcomp_mi_free(out)


def decompress_image(data, *, device=-1, small_model=False, devices=None, chunks_per_device=0):
    """RawImage(pixels: np.uint8[h,w,c], width, height, channels) from either wire format.  devices=[ordinals]: decoded over
    these GPUs inside this process (llcomp_mi_decode_devices)."""
    L = _lib.load()
    data = bytes(data)  # no copy when it already is bytes
    src = C.cast(C.c_char_p(data or b"\0"), _lib.u8p)  # borrows the bytes object's buffer for the call
    px, w, h, c = _lib.u8p(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    if devices is not None:
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        _check(L.llcomp_mi_decode_devices(src, len(data), arr, len(devices), int(chunks_per_device), 1 if small_model else 0, C.byref(px), C.byref(w),
                                          C.byref(h), C.byref(c)))
    else:
        _check(L.llcomp_mi_decode_flags(src, len(data), device, 1 if small_model else 0, C.byref(px), C.byref(w), C.byref(h), C.byref(c)))
    try:
        n = w.value * h.value * c.value
        pixels = np.ctypeslib.as_array(px, shape=(max(n, 1),))[:n].copy().reshape(h.value, w.value, c.value)
    finally:
        L.llcomp_mi_free(px)
    return RawImage(pixels, w.value, h.value, c.value)


def region_plan(w, h, c, tile_w, tile_h, planar, x, y, rw, rh):
    """((tx0, ty0, tx1, ty1), covered slices per frame) of the rectangle (x, y, rw, rh) -- llcomp_mi_region_plan, host only.  tile_w /
    tile_h 0 = the whole width / height.  LlcompError(BAD_ARGS) for an empty rectangle or one outside the image."""
    box, n = (C.c_uint32 * 4)(), C.c_uint32()
    _check(_lib.load().llcomp_mi_region_plan(w, h, c, tile_w, tile_h, int(bool(planar)), x, y, rw, rh, box, C.byref(n)))
    return tuple(box), n.value


def _xy_table(xy, n=None):
    """a sequence of (x, y) pairs or an int / uint32 array of shape [n, 2] -> (ctypes u32 array of 2n values, n); BAD_ARGS otherwise"""
    a = np.asarray(xy)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or (n is not None and a.shape[0] != n) or not np.issubdtype(a.dtype, np.integer) \
            or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
        raise LlcompError(BAD_ARGS, f"xy must be {n if n is not None else 'n'} x 2 non-negative integers, got shape {a.shape} {a.dtype}")
    flat = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return (C.c_uint32 * flat.size)(*flat.tolist()), a.shape[0]


def regions_plan(w, h, c, tile_w, tile_h, planar, rw, rh, xy):
    """(windows, n_classes) of a rectangle of size (rw, rh) at every offset of `xy` ([n, 2]) -- llcomp_mi_regions_plan, host only.
    windows = [n, 4] uint32 array of (wx0, wy0, wx1, wy1) tile windows.  LlcompError(BAD_ARGS) for a rectangle outside the image."""
    tab, n = _xy_table(xy)
    win, k = (C.c_uint32 * (4 * n))(), C.c_uint32()
    _check(_lib.load().llcomp_mi_regions_plan(w, h, c, tile_w, tile_h, int(bool(planar)), rw, rh, tab, n, win, C.byref(k)))
    return np.array(win, dtype=np.uint32).reshape(n, 4), k.value


def _rects_table(rects, n=None):
    """a sequence of (x, y, rw, rh) or an int array of shape [n, 4] -> (ctypes u32 array of 4n values, n); BAD_ARGS otherwise"""
    a = np.asarray(rects)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1 or (n is not None and a.shape[0] != n) or not np.issubdtype(a.dtype, np.integer) \
            or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
        raise LlcompError(BAD_ARGS, f"rects must be {n if n is not None else 'n'} x 4 non-negative integers, got shape {a.shape} {a.dtype}")
    flat = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return (C.c_uint32 * flat.size)(*flat.tolist()), a.shape[0]


def _signed_rects_table(rects, n=None):
    """a sequence of (x, y, rw, rh) with x and y of either sign -> (ctypes i32 array of 4n values, n); BAD_ARGS otherwise"""
    a = np.asarray(rects)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1 or (n is not None and a.shape[0] != n) or not np.issubdtype(a.dtype, np.integer) \
            or (a.size and (a.min() < -0x80000000 or a.max() > 0x7FFFFFFF)):
        raise LlcompError(BAD_ARGS, f"rects must be {n if n is not None else 'n'} x 4 integers of 32 bits, got shape {a.shape} {a.dtype}")
    flat = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return (C.c_int32 * flat.size)(*flat.tolist()), a.shape[0]


def pad_code(pad_mode):
    """PAD_* of a code (0..3) or a name ("constant", "edge", "reflect", "symmetric"); BAD_ARGS for anything else"""
    if isinstance(pad_mode, str) and pad_mode.lower() in PAD_NAMES:
        return PAD_NAMES.index(pad_mode.lower())
    if isinstance(pad_mode, (int, np.integer)) and not isinstance(pad_mode, bool) and 0 <= int(pad_mode) < len(PAD_NAMES):
        return int(pad_mode)
    raise LlcompError(BAD_ARGS, f"pad_mode must be one of {PAD_NAMES} or its code 0..{len(PAD_NAMES) - 1}, got {pad_mode!r}")


def _pad(c, pad_mode, fill=None):
    """(llcomp_mi_pad, what must stay alive during the call).  pad_mode None with a fill is "constant"; fill: one value or c values in 0..255"""
    mode = PAD_CONSTANT if pad_mode is None else pad_code(pad_mode)
    arr = None
    if fill is not None:
        a = np.asarray(fill).reshape(-1)
        if a.size == 1:
            a = np.full(c, a[0])
        if a.size != c or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
            raise LlcompError(BAD_ARGS, f"fill takes one or {c} integers in 0..255, got {fill!r}")
        arr = (C.c_uint8 * c)(*[int(v) for v in a.tolist()])
    pad = _Pad(C.sizeof(_Pad), mode, C.cast(arr, _lib.u8p) if arr is not None else None)
    return pad, (pad, arr)


def pad_axis(pad_mode, n, x, r):
    """(s0, s_len): the source interval of the rectangle [x, x + r) of an axis of side n under pad_mode (llcomp_mi_pad_axis, host only) --
    the image pixels the padded rectangle is made of.  LlcompError(BAD_ARGS) for a rectangle with no image pixel or a pad above the mode's
    limit (n - 1 for "reflect", else n)."""
    if not (-0x80000000 <= int(x) <= 0x7FFFFFFF and 0 <= int(n) <= 0xFFFFFFFF and 0 <= int(r) <= 0xFFFFFFFF):
        raise LlcompError(BAD_ARGS, f"no rectangle [{x}, {x} + {r}) of an axis of {n}")
    s0, sl = C.c_uint32(), C.c_uint32()
    _check(_lib.load().llcomp_mi_pad_axis(pad_code(pad_mode), n, x, r, C.byref(s0), C.byref(sl)))
    return s0.value, sl.value


def padded_weights(filter, pad_mode, n, x, r, out_len):
    """(s0, lo np.uint32[out_len], q np.int32[out_len, K'], bias np.int32[out_len]) of one axis of a padded call
    (llcomp_mi_padded_filter_weights, host only): output i = clamp((sum_j q[i, j] * src[s0 + lo[i] + j] + bias[i] * fill + 2^21) >> 22) --
    resize_weights(r, out_len, filter) with every tap on a padded index folded onto the source pixel it stands for, or into the bias for
    "constant".  LlcompError(BAD_ARGS) for what pad_axis or resize_weights refuse."""
    L = _lib.load()
    code = int(filter) if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 0xFFFFFFFF else filter_code(filter)
    mode = pad_code(pad_mode)
    if not (-0x80000000 <= int(x) <= 0x7FFFFFFF and 0 <= int(n) <= 0xFFFFFFFF and 0 <= int(r) <= 0xFFFFFFFF and 0 <= int(out_len) <= 0xFFFFFFFF):
        raise LlcompError(BAD_ARGS, f"no resampling of [{x}, {x} + {r}) of an axis of {n} to {out_len}")
    s0 = C.c_uint32()
    k = L.llcomp_mi_padded_filter_weights(code, mode, n, x, r, out_len, C.byref(s0), None, None, None)
    if not k:
        raise LlcompError(BAD_ARGS, f"no resampling of [{x}, {x} + {r}) of an axis of {n} to {out_len} with filter {filter!r}, pad {pad_mode!r}")
    lo, q, bias = np.zeros(out_len, np.uint32), np.zeros((out_len, k), np.int32), np.zeros(out_len, np.int32)
    L.llcomp_mi_padded_filter_weights(code, mode, n, x, r, out_len, C.byref(s0), lo.ctypes.data, q.ctypes.data, bias.ctypes.data)
    return s0.value, lo, q, bias


def padded_regions_plan(w, h, rects, pad_mode):
    """every rectangle's SOURCE rectangle [n, 4] of (x, y, rw, rh) inside the image (llcomp_mi_padded_regions_plan, host only): what a padded
    call decodes is what the unpadded calls decode for these -- resized_regions_plan of them gives its windows, views_plan of the views'
    source rectangles its unions.  LlcompError(BAD_ARGS) for a rectangle with no image pixel on an axis or a pad above the mode's limit."""
    tab, n = _signed_rects_table(rects)
    pad, _keep = _pad(1, pad_mode)
    src = np.zeros((n, 4), np.uint32)
    _check(_lib.load().llcomp_mi_padded_regions_plan(w, h, tab, n, C.byref(pad), src.ctypes.data_as(C.POINTER(C.c_uint32))))
    return src


def filter_code(filter):
    """FILTER_* of a code (0..5) or a name ("bilinear", "nearest", "box", "hamming", "bicubic", "lanczos"); BAD_ARGS for anything else"""
    if isinstance(filter, str) and filter.lower() in FILTER_NAMES:
        return FILTER_NAMES.index(filter.lower())
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) < len(FILTER_NAMES):
        return int(filter)
    raise LlcompError(BAD_ARGS, f"filter must be one of {FILTER_NAMES} or its code 0..{len(FILTER_NAMES) - 1}, got {filter!r}")


def _flags_table(flags, n, filter=None):
    """None, or n per-frame flags (bit 0: mirror horizontally, bits 4-6: the frame's filter) -> (ctypes u8 array or None).  filter: one
    code or name for every frame, or a sequence of n; it is OR-ed into bits 4-6."""
    if flags is None and filter is None:
        return None
    a = np.zeros(n, np.int64) if flags is None else np.asarray(flags)
    if a.shape != (n,) or (a.size and (a.min() < 0 or a.max() > 255)):
        raise LlcompError(BAD_ARGS, f"flags must be {n} values in 0..255, got shape {a.shape}")
    vals = [int(v) for v in a.tolist()]
    if filter is not None:
        per_frame = [filter] * n if isinstance(filter, (str, int, np.integer)) else list(filter)
        if len(per_frame) != n:
            raise LlcompError(BAD_ARGS, f"filter must be one filter or {n} of them, got {len(per_frame)}")
        vals = [v | (filter_code(f) << FLAG_FILTER_SHIFT) for v, f in zip(vals, per_frame)]
    return (C.c_uint8 * n)(*vals)


_DTYPES = {"uint8": DTYPE_U8, "u8": DTYPE_U8, "float32": DTYPE_F32, "float": DTYPE_F32, "f32": DTYPE_F32, "float16": DTYPE_F16,
           "half": DTYPE_F16, "f16": DTYPE_F16, "bfloat16": DTYPE_BF16, "bf16": DTYPE_BF16}
# numpy type of each dtype's elements (bfloat16: its bit patterns, numpy has no bfloat16)
_NP_OF_DTYPE = {DTYPE_U8: np.uint8, DTYPE_F32: np.float32, DTYPE_F16: np.float16, DTYPE_BF16: np.uint16}


def _dtype_code(dtype):
    """None / "float32" / np.float16 / torch.bfloat16 / ... -> DTYPE_*; BAD_ARGS for anything else"""
    if dtype is None:
        return DTYPE_U8
    if isinstance(dtype, (int, np.integer)) and not isinstance(dtype, bool) and int(dtype) in _NP_OF_DTYPE:
        return int(dtype)
    name = str(dtype).replace("torch.", "")
    if name not in _DTYPES:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            pass
    if name not in _DTYPES:
        raise LlcompError(BAD_ARGS, f"dtype must be uint8, float32, float16 or bfloat16, got {dtype!r}")
    return _DTYPES[name]


def _output_format(c, dtype=None, layout="hwc", scale=False, mean=None, std=None):
    """(OutputFormat, numpy element type, what must stay alive during the call); the format is None where every argument is its
    default (the u8 calls exactly).  mean / std: c values (one value is used for every channel); the library checks them."""
    code = _dtype_code(dtype)
    lay = {"hwc": LAYOUT_HWC, "chw": LAYOUT_CHW}.get(str(layout).lower()) if not isinstance(layout, int) else layout
    if lay is None:
        raise LlcompError(BAD_ARGS, f"layout must be 'hwc' or 'chw', got {layout!r}")
    if dtype is None and lay == LAYOUT_HWC and not scale and mean is None and std is None:
        return None, np.uint8, ()
    keep = []

    def vec(v):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32).reshape(-1)
        if a.size == 1:
            a = np.full(c, a[0], np.float32)
        if a.size != c:
            raise LlcompError(BAD_ARGS, f"mean / std take {c} values, got {a.size}")
        arr = (C.c_float * c)(*a.tolist())
        keep.append(arr)
        return C.cast(arr, C.POINTER(C.c_float))

    fmt = OutputFormat(C.sizeof(OutputFormat), code, lay, int(bool(scale)), vec(mean), vec(std))
    return fmt, _NP_OF_DTYPE[code], (fmt, keep)


def output_table(c, dtype, scale=False, mean=None, std=None):
    """The output rule of the resized calls as a table [c, 256] (llcomp_mi_output_table, host only): entry [ch, v] is what an output in
    this format holds where the u8 call writes v in channel ch -- float32, float16, uint8, or uint16 holding the bfloat16 bits.
    LlcompError(BAD_ARGS) for a format the calls refuse (U8 with scale / mean / std, a mean not finite, a std 0 or not finite)."""
    fmt, np_t, keep = _output_format(c, dtype, "hwc", scale, mean, std)
    if fmt is None:
        fmt, np_t, keep = _output_format(c, DTYPE_U8, "chw")
    out = np.zeros((c, 256), np_t)
    _check(_lib.load().llcomp_mi_output_table(C.byref(fmt), c, out.ctypes.data))
    return out


def resize_weights(in_len, out_len, filter=0):
    """(lo np.uint32[out_len], q np.int32[out_len, K]) of the resampling rule of one axis under `filter` (a FILTER_* code or its name;
    llcomp_mi_resize_filter_weights, host only): PIL's filter in Q22, exactly what the GPU runs.  LlcompError(BAD_ARGS) for a side of
    0, an unknown filter, or a downscale above the filter's limit (64x; bicubic 32x; Lanczos 64/3)."""
    L = _lib.load()
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 0xFFFFFFFF:
        code = int(filter)  # (an unknown code is the library's to refuse)
    else:
        code = filter_code(filter)
    if not (0 <= int(in_len) <= 0xFFFFFFFF and 0 <= int(out_len) <= 0xFFFFFFFF):
        raise LlcompError(BAD_ARGS, f"no resampling {in_len} -> {out_len}")
    k = L.llcomp_mi_resize_filter_weights(code, in_len, out_len, None, None)
    if not k:
        raise LlcompError(BAD_ARGS, f"no resampling {in_len} -> {out_len} with filter {filter!r}")
    lo, q = np.zeros(out_len, np.uint32), np.zeros((out_len, k), np.int32)
    L.llcomp_mi_resize_filter_weights(code, in_len, out_len, lo.ctypes.data, q.ctypes.data)
    return lo, q


def resized_regions_plan(w, h, c, tile_w, tile_h, planar, rects):
    """(windows, n_classes) of a rectangle of its own size per frame (rects [n, 4] of (x, y, rw, rh)), every window sized for the largest
    one -- llcomp_mi_resized_regions_plan, host only.  LlcompError(BAD_ARGS) for a rectangle empty or outside the image."""
    tab, n = _rects_table(rects)
    win, k = (C.c_uint32 * (4 * n))(), C.c_uint32()
    _check(_lib.load().llcomp_mi_resized_regions_plan(w, h, c, tile_w, tile_h, int(bool(planar)), tab, n, win, C.byref(k)))
    return np.array(win, dtype=np.uint32).reshape(n, 4), k.value


class ViewGroup:
    """Views that share one output (llcomp_mi_view_group): views = a sequence of (frame, x, y, rw, rh) or (frame, x, y, rw, rh, flags) or
    an int array [n, 5 or 6]; the output is [n][oh][ow][c] at device address d_out (layout="chw": [n][c][oh][ow]) in the format that
    dtype, layout, scale, mean and std give (as Codec.decode_resized_regions takes them); filter: one name or FILTER_* code for every view
    of the group, or one per view, OR-ed into bits 4-6 of the views' flags.  A plain tuple (views, ow, oh, d_out) is a group too.
    photo: a photometric chain for every view of the group -- a list of (op, param) or (name, param) pairs or bare names, such as
    [("brightness", 1.2), ("adjust_hue", 0.05), "grayscale", ("gaussian_blur", 1.5)] -- or a list of one chain per view (photo_chain);
    None: none."""

    def __init__(self, views, ow, oh, d_out=0, dtype=None, layout="hwc", scale=False, mean=None, std=None, filter=None, photo=None):
        self.views, self.ow, self.oh, self.d_out = views, ow, oh, d_out
        self.format = dict(dtype=dtype, layout=layout, scale=scale, mean=mean, std=std)
        self.filter = filter
        self.photo = photo


def photo_code(op):
    """PHOTO_* code of an op given by name ("brightness", "contrast", "color" or "saturation", "grayscale", "invert", "solarize",
    "posterize", "autocontrast", "equalize", "gaussian_blur", "adjust_hue", "adjust_sharpness") or by code"""
    if isinstance(op, str):
        name = "color" if op.lower() == "saturation" else op.lower()
        if name in PHOTO_MORE_NAMES:
            return PHOTO_MORE_NAMES[name]
        if name not in PHOTO_NAMES:
            raise LlcompError(BAD_ARGS, f"no photometric op {op!r}: one of {PHOTO_NAMES + tuple(PHOTO_MORE_NAMES)}")
        return PHOTO_NAMES.index(name)
    code = int(op)
    if not 0 <= code <= 0xFFFFFFFF:
        raise LlcompError(BAD_ARGS, f"no photometric op {op!r}")
    return code


def photo_chain(ops):
    """a chain -- a sequence of (op, param) pairs, (op,) tuples, names or codes -- as a list of (code, float32 param); the limits are the
    library's to check, but for the length: a chain holds at most PHOTO_MAX_OPS ops"""
    out = []
    for o in ops if ops is not None else ():
        if isinstance(o, (str, int, np.integer)):
            o = (o,)
        o = tuple(o)
        if not 1 <= len(o) <= 2:
            raise LlcompError(BAD_ARGS, f"an op is (op, param) or (op,), got {o!r}")
        out.append((photo_code(o[0]), float(np.float32(o[1] if len(o) == 2 and o[1] is not None else 0.0))))
    if len(out) > PHOTO_MAX_OPS:
        raise LlcompError(BAD_ARGS, f"a chain holds at most {PHOTO_MAX_OPS} ops, got {len(out)}")
    return out


def _is_op(o):
    """whether an element of a photo= list is ONE op -- a name, a code, an (op, param) pair with a number for param, or a 1-tuple (op,) --
    and not a view's chain (a list of ops)"""
    if isinstance(o, (str, int, np.integer)):
        return True
    if not isinstance(o, (tuple, list)) or not o or not isinstance(o[0], (str, int, np.integer)):
        return False
    if len(o) == 1:
        return isinstance(o, tuple)
    return len(o) == 2 and (o[1] is None or isinstance(o[1], (int, float, np.integer, np.floating)))


def _photo_groups(groups, n_views):
    """the photo= of every group -> (ctypes array of llcomp_mi_photo_group or None when no group has one, keep-alive list); n_views: the
    groups' view counts"""
    specs = [getattr(gr, "photo", None) for gr in groups]
    if all(p is None for p in specs):
        return None, []
    arr, keep = (_PhotoGroup * max(1, len(groups)))(), []
    for i, spec in enumerate(specs):
        arr[i] = _PhotoGroup(C.sizeof(_PhotoGroup), None)
        if spec is None:
            continue
        spec = list(spec)
        if all(_is_op(o) for o in spec):  # one chain for all views (an empty list: the empty chain)
            chains = [photo_chain(spec)] * n_views[i]
        else:
            if len(spec) != n_views[i]:
                raise LlcompError(BAD_ARGS, f"group {i}: photo takes one chain, or one per view ({n_views[i]}), got {len(spec)}")
            chains = [photo_chain(ch) for ch in spec]
        carr = (_PhotoChain * max(1, len(chains)))()
        for j, ch in enumerate(chains):
            carr[j].n_ops = len(ch)
            for k, (op, param) in enumerate(ch):
                carr[j].ops[k] = _PhotoOp(op, param)
        keep.append(carr)
        arr[i] = _PhotoGroup(C.sizeof(_PhotoGroup), C.cast(carr, C.POINTER(_PhotoChain)))
    return arr, keep


def photo_reference(frame, ops):
    """The rule of the photometric chains on a host image (llcomp_mi_photo_reference): frame [h, w] or [h, w, c] uint8 with c = 1 or 3,
    ops a chain as photo_chain takes it -> the image after the chain, byte for byte PIL's ImageEnhance / ImageOps / ImageFilter.GaussianBlur
    / ImageEnhance.Sharpness and torchvision's adjust_hue applied in order."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    if a.ndim not in (2, 3) or not a.size:
        raise LlcompError(BAD_ARGS, f"a frame is [h, w] or [h, w, c], got shape {a.shape}")
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    ch = list(ops if ops is not None else ())
    raw = []
    for o in ch:  # (the length is the library's to refuse here: no PHOTO_MAX_OPS check on this side)
        raw += photo_chain([o])
    arr = (_PhotoOp * max(1, len(raw)))(*[_PhotoOp(op, p) for op, p in raw])
    out = np.zeros_like(a)
    _check(_lib.load().llcomp_mi_photo_reference(a.ctypes.data, w, h, c, arr, len(raw), out.ctypes.data))
    return out


MIX_BLEND = 1


def _layout_code(layout):
    lay = {"hwc": LAYOUT_HWC, "chw": LAYOUT_CHW}.get(str(layout).lower()) if not isinstance(layout, int) else layout
    if lay is None:
        raise LlcompError(BAD_ARGS, f"layout must be 'hwc' or 'chw', got {layout!r}")
    return lay


def _mix_rects(r, n, what):
    """None / one (x, y, w, h) for every sample / n of them, each (x, y, w, h) or None -> n tuples"""
    if r is None:
        return [(0, 0, 0, 0)] * n
    r = list(r)
    if len(r) == 4 and all(isinstance(v, (int, np.integer)) for v in r):
        r = [r] * n
    if len(r) != n:
        raise LlcompError(BAD_ARGS, f"{what} must be one (x, y, w, h) or {n} of them, got {len(r)}")
    out = []
    for q in r:
        q = (0, 0, 0, 0) if q is None else tuple(int(v) for v in q)
        if len(q) != 4 or min(q) < 0 or max(q) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"{what}: a rectangle is (x, y, w, h) of unsigned values, got {q!r}")
        out.append(q)
    return out


def mix_samples(n, partner=None, lam=None, boxes=None, erase=None):
    """The records of a mix_batch call (llcomp_mi_mix_sample), n of them as a ctypes array.  partner: None (every sample by itself),
    "roll" (torchvision's inpt.roll(1, 0): sample i mixes with i - 1), "flip" (timm's x.flip(0): with n - 1 - i) or n indices, a
    permutation.  lam: None, one value or n of them (None: that sample does not blend): MixUp's weight of the sample itself -- the
    record takes w_own = float32(lam) and w_partner = float32(1.0 - lam), lam a double, which is what torch's mul(lam) and
    mul(1.0 - lam) compute with.  boxes: CutMix's box, None, one (x, y, w, h) or n of them (None: none).  erase: RandomErasing's
    rectangle, the same way.  The library checks the records."""
    n = int(n)
    if n <= 0:
        raise LlcompError(BAD_ARGS, f"n must be positive, got {n}")
    if partner is None:
        part = list(range(n))
    elif isinstance(partner, str):
        if partner not in ("roll", "flip"):
            raise LlcompError(BAD_ARGS, f"partner must be None, 'roll', 'flip' or {n} indices, got {partner!r}")
        part = [(i + n - 1) % n for i in range(n)] if partner == "roll" else [n - 1 - i for i in range(n)]
    else:
        part = [int(v) for v in partner]
        if len(part) != n or min(part) < 0 or max(part) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"partner must be {n} indices, got {len(part)}")
    if lam is None or isinstance(lam, (int, float, np.integer, np.floating)):
        lams = [lam] * n
    else:
        lams = list(lam)
        if len(lams) != n:
            raise LlcompError(BAD_ARGS, f"lam must be one value or {n} of them, got {len(lams)}")
    bx, er = _mix_rects(boxes, n, "boxes"), _mix_rects(erase, n, "erase")
    arr = (_MixSample * n)()
    for i in range(n):
        s = arr[i]
        s.partner = part[i]
        if lams[i] is not None:
            lam_i = float(lams[i])
            s.flags = MIX_BLEND
            s.w_own, s.w_partner = float(np.float32(lam_i)), float(np.float32(1.0 - lam_i))
        s.box[:] = bx[i]
        s.erase[:] = er[i]
    return arr


def _mix_records(samples, n=None):
    if not isinstance(samples, C.Array) or samples._type_ is not _MixSample:
        raise LlcompError(BAD_ARGS, "samples must come from mix_samples()")
    if n is not None and len(samples) != int(n):
        raise LlcompError(BAD_ARGS, f"{n} samples take {n} records, got {len(samples)}")
    return samples


def mix_segment():
    """the samples one thread of the mixing kernel walks: a longer cycle of partners is cut (llcomp_mi_mix_segment)"""
    return int(_lib.load().llcomp_mi_mix_segment())


def mix_plan(samples):
    """What a mix_batch call does with these records (llcomp_mi_mix_plan, host only) -> (order, seg_first, n_saved): the samples cycle
    by cycle along their partners, where every segment begins in that order (one more entry: n), and how many segment heads are saved
    first.  LlcompError(BAD_ARGS) for records the calls refuse by themselves."""
    samples = _mix_records(samples)
    n = len(samples)
    order, seg = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
    ns, nv = C.c_uint32(0), C.c_uint32(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_mix_plan(n, samples, order.ctypes.data_as(u32p), seg.ctypes.data_as(u32p), C.byref(ns), C.byref(nv)))
    return order, seg[:ns.value + 1].copy(), int(nv.value)


def _per_channel(values, c, what):
    """one value or c of them (None: the library's zeros) -> a ctypes float array for the batch calls, or None"""
    if values is None:
        return None
    a = np.asarray(values, dtype=np.float32).reshape(-1)
    if a.size == 1:
        a = np.full(c, a[0], np.float32)
    if a.size != c:
        raise LlcompError(BAD_ARGS, f"{what} takes {c} values, got {a.size}")
    return (C.c_float * c)(*a.tolist())


def _batch_array(batch, dtype, layout):
    """a host batch [n, c, h, w] ("chw") or [n, h, w, c] ("hwc") for the references of the batch calls -> (the contiguous array, dtype
    code, layout code, n, c, h, w)"""
    a = np.ascontiguousarray(batch)
    code = _dtype_code(a.dtype if dtype is None else dtype)
    if a.ndim != 4 or not a.size or a.dtype != _NP_OF_DTYPE[code]:
        raise LlcompError(BAD_ARGS, f"a batch is 4-D {_NP_OF_DTYPE[code].__name__}, got {a.dtype} of shape {a.shape}")
    lay = _layout_code(layout)
    c, h, w = a.shape[1:] if lay == LAYOUT_CHW else (a.shape[3], a.shape[1], a.shape[2])
    return a, code, lay, a.shape[0], c, h, w


def mix_reference(batch, samples, layout="chw", erase_value=None, dtype=None):
    """The rule of the batch mixing on a host array (llcomp_mi_mix_reference): batch [n, c, oh, ow] (layout "chw") or [n, oh, ow, c]
    ("hwc") of uint8, float32, float16, or uint16 holding bfloat16 bits with dtype="bfloat16" -> the mixed batch, a new array."""
    a, code, lay, n, c, oh, ow = _batch_array(batch, dtype, layout)
    ev = _per_channel(erase_value, c, "erase_value")
    out = np.empty_like(a)
    _check(_lib.load().llcomp_mi_mix_reference(a.ctypes.data, n, c, ow, oh, code, lay, _mix_records(samples, n), ev, out.ctypes.data))
    return out


# the orientations of Codec.orient_batch (LLCOMP_MI_ORIENT_*): 0 for none, otherwise PIL's Image.Transpose value plus 1
(ORIENT_NONE, ORIENT_FLIP_LEFT_RIGHT, ORIENT_FLIP_TOP_BOTTOM, ORIENT_ROTATE_90, ORIENT_ROTATE_180, ORIENT_ROTATE_270, ORIENT_TRANSPOSE,
 ORIENT_TRANSVERSE) = range(8)
ORIENT_NAMES = ("none", "flip_left_right", "flip_top_bottom", "rotate_90", "rotate_180", "rotate_270", "transpose", "transverse")


def orient_code(orientation):
    """ORIENT_* of a code (0..7), of None, or of a name in any letter case: "none" or PIL's Image.Transpose names ("FLIP_LEFT_RIGHT",
    "FLIP_TOP_BOTTOM", "ROTATE_90", "ROTATE_180", "ROTATE_270", "TRANSPOSE", "TRANSVERSE"); BAD_ARGS for anything else"""
    if orientation is None:
        return ORIENT_NONE
    if isinstance(orientation, str) and orientation.lower() in ORIENT_NAMES:
        return ORIENT_NAMES.index(orientation.lower())
    if isinstance(orientation, (int, np.integer)) and not isinstance(orientation, bool) and 0 <= int(orientation) < len(ORIENT_NAMES):
        return int(orientation)
    raise LlcompError(BAD_ARGS, f"an orientation is None, one of {ORIENT_NAMES} or its code 0..{len(ORIENT_NAMES) - 1}, got {orientation!r}")


def _orient_codes(codes, n):
    """n orientations (codes, names or None), or one for every sample -> a ctypes u8 array; a code the library would refuse (above 7)
    is passed on for it to refuse"""
    per_sample = [codes] * n if codes is None or isinstance(codes, (str, int, np.integer)) else list(codes)
    if len(per_sample) != n:
        raise LlcompError(BAD_ARGS, f"{n} samples take {n} orientations, got {len(per_sample)}")
    vals = []
    for v in per_sample:
        if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) <= 255:
            vals.append(int(v))
        else:
            vals.append(orient_code(v))
    return (C.c_uint8 * max(1, n))(*vals)


def orient_tile():
    """the side, in pixels, of the orientation kernel's tile (llcomp_mi_orient_tile)"""
    return int(_lib.load().llcomp_mi_orient_tile())


def orient_reference(batch, codes, layout="chw", dtype=None):
    """The rule of the batch orientation on a host array (llcomp_mi_orient_reference): batch [n, c, oh, ow] (layout "chw") or
    [n, oh, ow, c] ("hwc") of uint8, float32, float16, or uint16 holding bfloat16 bits with dtype="bfloat16"; codes: n orientations
    (orient_code) or one for every sample -> the oriented batch, a new array of the same shape (the transposing codes take squares)."""
    a, code, lay, n, c, oh, ow = _batch_array(batch, dtype, layout)
    out = np.empty_like(a)
    _check(_lib.load().llcomp_mi_orient_reference(a.ctypes.data, n, c, ow, oh, code, lay, _orient_codes(codes, n), out.ctypes.data))
    return out


# Codec.compose_batch (LLCOMP_MI_COMPOSE_*): a piece's flag, and the call's
COMPOSE_FILL = 1
COMPOSE_KEEP = 1
_COMPOSE_FIELDS = ("dst", "src", "dx", "dy", "sx", "sy", "w", "h", "flags")


def compose_pieces(records):
    """The pieces of a compose_batch call (llcomp_mi_compose_piece) as a ctypes array: every record a tuple (dst, src, dx, dy, sx, sy,
    w, h[, flags]) or a dict of those names (what it leaves out is 0).  A FILL piece has flags=COMPOSE_FILL and src, sx, sy 0.  The
    library checks the records."""
    if isinstance(records, C.Array) and records._type_ is _ComposePiece:
        return records
    records = list(records)
    arr = (_ComposePiece * len(records))()
    for i, r in enumerate(records):
        if isinstance(r, dict):
            if set(r) - set(_COMPOSE_FIELDS):
                raise LlcompError(BAD_ARGS, f"a piece has {_COMPOSE_FIELDS}, got {sorted(set(r) - set(_COMPOSE_FIELDS))}")
            vals = [r.get(name, 0) for name in _COMPOSE_FIELDS]
        else:
            vals = list(r)
            if len(vals) not in (8, 9):
                raise LlcompError(BAD_ARGS, f"a piece is (dst, src, dx, dy, sx, sy, w, h[, flags]), got {r!r}")
            vals += [0] * (9 - len(vals))
        vals = [int(v) for v in vals]
        if min(vals) < 0 or max(vals) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"a piece takes unsigned values, got {r!r}")
        for name, v in zip(_COMPOSE_FIELDS, vals):
            setattr(arr[i], name, v)
    return arr


def compose_tile(pixel_bytes=None):
    """the kernel's tile: its width in pixels (llcomp_mi_compose_tile), or with pixel_bytes -- the element's size in CHW, c elements in
    HWC -- its rows (llcomp_mi_compose_tile_rows)"""
    L = _lib.load()
    return int(L.llcomp_mi_compose_tile()) if pixel_bytes is None else int(L.llcomp_mi_compose_tile_rows(int(pixel_bytes)))


def compose_max_pieces_per_sample():
    """the most pieces with w and h above 0 on one dst sample (llcomp_mi_compose_max_pieces_per_sample)"""
    return int(_lib.load().llcomp_mi_compose_max_pieces_per_sample())


def compose_plan(n_src, iw, ih, n_dst, ow, oh, c, pieces, dtype="float32", layout="chw", keep=False):
    """What a compose_batch call does (llcomp_mi_compose_plan, host only) -> (samples, first, order, n_workgroups): the dst samples that
    get workgroups, where every sample's pieces begin in order (one more entry: their number), the pieces' indices by dst sample, each
    sample's in the call's order without the empty ones, and the workgroups of the kernel.  LlcompError(BAD_ARGS) for a call that is
    refused by itself."""
    recs = compose_pieces(pieces)
    n_dst = int(n_dst)
    samples, first, order = np.zeros(max(n_dst, 1), np.uint32), np.zeros(max(n_dst, 1) + 1, np.uint32), np.zeros(max(len(recs), 1), np.uint32)
    ns, nw = C.c_uint32(0), C.c_uint64(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_compose_plan(int(n_src), int(iw), int(ih), n_dst, int(ow), int(oh), int(c), _dtype_code(dtype), _layout_code(layout),
                                              recs, len(recs), COMPOSE_KEEP if keep else 0, samples.ctypes.data_as(u32p),
                                              first.ctypes.data_as(u32p), order.ctypes.data_as(u32p), C.byref(ns), C.byref(nw)))
    n = ns.value
    return samples[:n].copy(), first[:n + 1].copy(), order[:int(first[n])].copy(), int(nw.value)


def compose_reference(src, dst, pieces, layout="chw", fill=None, keep=False, dtype=None):
    """The rule of the batch composition on host arrays (llcomp_mi_compose_reference): src [n_src, c, ih, iw] (layout "chw") or
    [n_src, ih, iw, c] ("hwc"), or None when every piece is a FILL piece; dst the same way -- its values matter under keep only; both of
    uint8, float32, float16, or uint16 holding bfloat16 bits with dtype="bfloat16" -> the composed dst batch, a new array."""
    d, code, lay, n_dst, c, oh, ow = _batch_array(dst, dtype, layout)
    n_src = iw = ih = 0
    s = None
    if src is not None:
        s = np.ascontiguousarray(src)
        if s.ndim != 4 or s.dtype != d.dtype or (s.shape[1] if lay == LAYOUT_CHW else s.shape[3]) != c:
            raise LlcompError(BAD_ARGS, f"src is a 4-D batch of dst's type and channels, got {s.dtype} of shape {s.shape}")
        n_src = s.shape[0]
        ih, iw = s.shape[2:] if lay == LAYOUT_CHW else s.shape[1:3]
    recs = compose_pieces(pieces)
    out = np.empty_like(d)
    _check(_lib.load().llcomp_mi_compose_reference(s.ctypes.data if n_src else None, n_src, iw, ih, d.ctypes.data, n_dst, ow, oh, c, code, lay,
                                                   recs, len(recs), _per_channel(fill, c, "fill"), COMPOSE_KEEP if keep else 0, out.ctypes.data))
    return out


def grid_pieces(n, iw, ih, nrow=8, padding=2):
    """The pieces that lay n samples of iw x ih out as torchvision.utils.make_grid(nrow=, padding=) does, on ONE canvas (dst sample 0)
    -> (pieces, ow, oh); the canvas's fill is make_grid's pad_value.  (make_grid returns a single picture as it is; this lays it
    out with its border like the others.)"""
    n, iw, ih, nrow, padding = int(n), int(iw), int(ih), int(nrow), int(padding)
    if n <= 0 or iw <= 0 or ih <= 0 or nrow <= 0 or padding < 0:
        raise LlcompError(BAD_ARGS, "grid_pieces takes n, iw, ih, nrow above 0 and a padding of 0 or more")
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    cw, ch = iw + padding, ih + padding
    recs = [(0, k, (k % xmaps) * cw + padding, (k // xmaps) * ch + padding, 0, 0, iw, ih) for k in range(n)]
    return compose_pieces(recs), cw * xmaps + padding, ch * ymaps + padding


def mosaic_pieces(centres, iw, ih, s):
    """The pieces of YOLO's 4-picture mosaic as Ultralytics' load_mosaic places them: canvas i, 2s x 2s, takes src samples 4i .. 4i + 3
    of iw x ih around centres[i] = (xc, yc) -- top left, top right, bottom left, bottom right, each clipped to its quadrant and read
    from the corner of its picture that touches the centre.  The canvas's fill is 114 there.  -> the pieces"""
    iw, ih, s = int(iw), int(ih), int(s)
    recs = []
    for i, (xc, yc) in enumerate(centres):
        xc, yc = int(xc), int(yc)
        if not (0 <= xc <= 2 * s and 0 <= yc <= 2 * s):
            raise LlcompError(BAD_ARGS, f"a mosaic centre lies in the canvas of {2 * s} x {2 * s}, got {(xc, yc)}")
        boxes = (
            (max(xc - iw, 0), max(yc - ih, 0), xc, yc, "br"),
            (xc, max(yc - ih, 0), min(xc + iw, 2 * s), yc, "bl"),
            (max(xc - iw, 0), yc, xc, min(2 * s, yc + ih), "tr"),
            (xc, yc, min(xc + iw, 2 * s), min(2 * s, yc + ih), "tl"),
        )
        for k, (x1, y1, x2, y2, corner) in enumerate(boxes):
            w, h = x2 - x1, y2 - y1
            sx = iw - w if corner in ("br", "tr") else 0
            sy = ih - h if corner in ("br", "bl") else 0
            recs.append((i, 4 * i + k, x1, y1, sx, sy, w, h))
    return compose_pieces(recs)


# Codec.paste_batch (LLCOMP_MI_PASTE_VALUE): a piece's flag
PASTE_VALUE = 1


def paste_pieces(records):
    """The pieces of a paste_batch call (llcomp_mi_paste_piece) as a ctypes array: every record a tuple (dst, src, dx, dy, sx, sy, w, h,
    ids[, value]).  ids: an iterable of ints 0..255, the mask bytes the piece selects, or "nonzero" for all of them but 0 (a binary
    mask).  A value makes a VALUE piece: the selected pixels take the value in every channel, not src's.  The library checks the rest."""
    if isinstance(records, C.Array) and records._type_ is _PastePiece:
        return records
    records = list(records)
    arr = (_PastePiece * len(records))()
    for i, r in enumerate(records):
        vals = list(r) if isinstance(r, (tuple, list)) else []
        if len(vals) not in (9, 10):
            raise LlcompError(BAD_ARGS, f"a piece is (dst, src, dx, dy, sx, sy, w, h, ids[, value]), got {r!r}")
        nums = [int(v) for v in vals[:8]]
        if min(nums) < 0 or max(nums) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"a piece takes unsigned values, got {r!r}")
        for name, v in zip(("dst", "src", "dx", "dy", "sx", "sy", "w", "h"), nums):
            setattr(arr[i], name, v)
        ids = vals[8]
        if isinstance(ids, str):
            if ids != "nonzero":
                raise LlcompError(BAD_ARGS, f'ids are ints 0..255 or "nonzero", got {ids!r}')
            ids = range(1, 256)
        for m in ids:
            m = int(m)
            if not 0 <= m <= 255:
                raise LlcompError(BAD_ARGS, f"an id is 0..255, got {m}")
            arr[i].ids[m >> 5] |= 1 << (m & 31)
        if len(vals) == 10 and vals[9] is not None:
            arr[i].flags, arr[i].value = PASTE_VALUE, float(vals[9])
    return arr


def paste_max_pieces_per_sample():
    """the most pieces with w and h above 0 on one dst sample (llcomp_mi_paste_max_pieces_per_sample)"""
    return int(_lib.load().llcomp_mi_paste_max_pieces_per_sample())


def paste_plan(n_src, iw, ih, n_dst, ow, oh, c, pieces, dtype="float32", layout="chw"):
    """What a paste_batch call does (llcomp_mi_paste_plan, host only) -> (samples, first, order, n_workgroups), as compose_plan: the dst
    samples with a piece that is not ignored, where every sample's pieces begin in order, the pieces' indices by dst sample without the
    ignored ones (w or h 0, no id), and the workgroups of the kernel."""
    recs = paste_pieces(pieces)
    n_dst = int(n_dst)
    samples, first, order = np.zeros(max(n_dst, 1), np.uint32), np.zeros(max(n_dst, 1) + 1, np.uint32), np.zeros(max(len(recs), 1), np.uint32)
    ns, nw = C.c_uint32(0), C.c_uint64(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_paste_plan(int(n_src), int(iw), int(ih), n_dst, int(ow), int(oh), int(c), _dtype_code(dtype), _layout_code(layout),
                                            recs, len(recs), samples.ctypes.data_as(u32p), first.ctypes.data_as(u32p), order.ctypes.data_as(u32p),
                                            C.byref(ns), C.byref(nw)))
    n = ns.value
    return samples[:n].copy(), first[:n + 1].copy(), order[:int(first[n])].copy(), int(nw.value)


def paste_reference(src, mask, dst, pieces, layout="chw", dtype=None):
    """The rule of the batch copy-paste on host arrays (llcomp_mi_paste_reference): src [n_src, c, ih, iw] (layout "chw") or
    [n_src, ih, iw, c] ("hwc"), mask [n_src, ih, iw] uint8 (it may be src itself for c = 1 uint8), dst as src; both of uint8, float32,
    float16, or uint16 holding bfloat16 bits with dtype="bfloat16" -> the pasted dst batch, a new array."""
    d, code, lay, n_dst, c, oh, ow = _batch_array(dst, dtype, layout)
    s = np.ascontiguousarray(src)
    if s.ndim != 4 or s.dtype != d.dtype or (s.shape[1] if lay == LAYOUT_CHW else s.shape[3]) != c:
        raise LlcompError(BAD_ARGS, f"src is a 4-D batch of dst's type and channels, got {s.dtype} of shape {s.shape}")
    n_src = s.shape[0]
    ih, iw = s.shape[2:] if lay == LAYOUT_CHW else s.shape[1:3]
    m = s if mask is src else np.ascontiguousarray(mask)
    if m.dtype != np.uint8 or m.size != n_src * ih * iw:
        raise LlcompError(BAD_ARGS, f"mask is uint8 [n_src, ih, iw], got {m.dtype} of shape {m.shape}")
    recs = paste_pieces(pieces)
    out = np.empty_like(d)
    _check(_lib.load().llcomp_mi_paste_reference(s.ctypes.data, m.ctypes.data, n_src, iw, ih, d.ctypes.data, n_dst, ow, oh, c, code, lay, recs,
                                                 len(recs), out.ctypes.data))
    return out


def paste_pieces16(records):
    """The pieces of a paste_batch16 call (llcomp_mi_paste_piece16) as a ctypes array: every record a tuple (dst, src, dx, dy, sx, sy, w,
    h, ids[, value_bits]).  ids: an iterable of ints 0..65535, the ids of the 16-bit mask the record selects, or "nonzero" for all of
    them but 0.  A record becomes one piece per window of 256 ids that holds one of its ids, windows ascending, in the records' order:
    a window begins at its lowest id.  value_bits makes VALUE pieces: the selected pixels take these bits as their element in every
    channel, not src's.  A record without an id gives one piece that selects nothing.  The library checks the rest."""
    if isinstance(records, C.Array) and records._type_ is PastePiece16:
        return records
    out = []
    for r in list(records):
        vals = list(r) if isinstance(r, (tuple, list)) else []
        if len(vals) not in (9, 10):
            raise LlcompError(BAD_ARGS, f"a piece is (dst, src, dx, dy, sx, sy, w, h, ids[, value_bits]), got {r!r}")
        nums = [int(v) for v in vals[:8]]
        if min(nums) < 0 or max(nums) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"a piece takes unsigned values, got {r!r}")
        ids = vals[8]
        if isinstance(ids, str):
            if ids != "nonzero":
                raise LlcompError(BAD_ARGS, f'ids are ints 0..65535 or "nonzero", got {ids!r}')
            ids = range(1, 65536)
        ids = np.unique(np.asarray(list(ids), np.int64).reshape(-1))
        if ids.size and (ids[0] < 0 or ids[-1] > 0xFFFF):
            raise LlcompError(BAD_ARGS, f"an id is 0..65535, got {int(ids[0] if ids[0] < 0 else ids[-1])}")
        value = None
        if len(vals) == 10 and vals[9] is not None:
            value = int(vals[9])
            if not 0 <= value <= 0xFFFFFFFF:
                raise LlcompError(BAD_ARGS, f"value_bits are the element's bits, got {vals[9]!r}")
        at = 0
        while True:
            p = PastePiece16()
            for name, v in zip(("dst", "src", "dx", "dy", "sx", "sy", "w", "h"), nums):
                setattr(p, name, v)
            if value is not None:
                p.flags, p.value_bits = PASTE_VALUE, value
            if ids.size:
                p.id_base = int(ids[at])
                end = int(np.searchsorted(ids, p.id_base + 256))
                for m in ids[at:end]:
                    d = int(m) - p.id_base
                    p.ids[d >> 5] |= 1 << (d & 31)
                at = end
            out.append(p)
            if at >= ids.size:
                break
    arr = (PastePiece16 * len(out))()
    for i, p in enumerate(out):
        arr[i] = p
    return arr


PASTE_VALUE_PIXEL = 2


def paste_pieces32(records, map_bytes):
    """The pieces of a paste_batch32 call (llcomp_mi_paste_piece32) as a ctypes array, as paste_pieces16: every record a tuple (dst,
    src, dx, dy, sx, sy, w, h, ids[, value_bits[, pixel]]), ids an iterable of ints up to 0xFFFFFF (map_bytes 3) or 0xFFFFFFFF (4); one
    piece per window of 256 ids that holds one of its ids -- RGB ids are sparse, so mostly one piece per id.  pixel=True with
    value_bits makes VALUE_PIXEL pieces (uint8 "hwc", c <= 4): channel ch of a selected pixel takes byte ch of value_bits, which is how
    a pasted segment gets a new 3-byte id in a dst map.  "nonzero" is not offered: a binary mask is no list of windows."""
    if isinstance(records, C.Array) and records._type_ is PastePiece32:
        return records
    if int(map_bytes) not in (3, 4):
        raise LlcompError(BAD_ARGS, f"map_bytes of a wide id map is 3 or 4, got {map_bytes!r}")
    top = (1 << (8 * int(map_bytes))) - 1
    out = []
    for r in list(records):
        vals = list(r) if isinstance(r, (tuple, list)) else []
        if len(vals) not in (9, 10, 11):
            raise LlcompError(BAD_ARGS, f"a piece is (dst, src, dx, dy, sx, sy, w, h, ids[, value_bits[, pixel]]), got {r!r}")
        nums = [int(v) for v in vals[:8]]
        if min(nums) < 0 or max(nums) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"a piece takes unsigned values, got {r!r}")
        if isinstance(vals[8], str):
            raise LlcompError(BAD_ARGS, f"ids are ints 0..{top}, got {vals[8]!r}")
        ids = np.unique(np.asarray(list(vals[8]), np.int64).reshape(-1))
        if ids.size and (ids[0] < 0 or ids[-1] > top):
            raise LlcompError(BAD_ARGS, f"an id is 0..{top}, got {int(ids[0] if ids[0] < 0 else ids[-1])}")
        value = None
        if len(vals) >= 10 and vals[9] is not None:
            value = int(vals[9])
            if not 0 <= value <= 0xFFFFFFFF:
                raise LlcompError(BAD_ARGS, f"value_bits are the element's bits, got {vals[9]!r}")
        pixel = len(vals) == 11 and bool(vals[10])
        if pixel and value is None:
            raise LlcompError(BAD_ARGS, "pixel=True needs value_bits")
        at = 0
        while True:
            p = PastePiece32()
            for name, v in zip(("dst", "src", "dx", "dy", "sx", "sy", "w", "h"), nums):
                setattr(p, name, v)
            if value is not None:
                p.flags, p.value_bits = PASTE_VALUE | (PASTE_VALUE_PIXEL if pixel else 0), value
            if ids.size:
                p.id_base = int(ids[at])
                end = int(np.searchsorted(ids, p.id_base + 256))
                for m in ids[at:end]:
                    d = int(m) - p.id_base
                    p.ids[d >> 5] |= 1 << (d & 31)
                at = end
            out.append(p)
            if at >= ids.size:
                break
    arr = (PastePiece32 * len(out))()
    for i, p in enumerate(out):
        arr[i] = p
    return arr


def paste32_plan(map_bytes, n_src, iw, ih, n_dst, ow, oh, c, pieces, dtype="float32", layout="chw"):
    """What a paste_batch32 call does (llcomp_mi_paste32_plan, host only) -> (samples, first, order, n_workgroups), as paste16_plan."""
    recs = paste_pieces32(pieces, map_bytes)
    n_dst = int(n_dst)
    samples, first, order = np.zeros(max(n_dst, 1), np.uint32), np.zeros(max(n_dst, 1) + 1, np.uint32), np.zeros(max(len(recs), 1), np.uint32)
    ns, nw = C.c_uint32(0), C.c_uint64(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_paste32_plan(int(map_bytes), int(n_src), int(iw), int(ih), n_dst, int(ow), int(oh), int(c), _dtype_code(dtype),
                                              _layout_code(layout), recs, len(recs), samples.ctypes.data_as(u32p), first.ctypes.data_as(u32p),
                                              order.ctypes.data_as(u32p), C.byref(ns), C.byref(nw)))
    n = ns.value
    return samples[:n].copy(), first[:n + 1].copy(), order[:int(first[n])].copy(), int(nw.value)


def paste32_reference(src, mask, dst, pieces, layout="chw", dtype=None):
    """The rule of the batch copy-paste by wide ids on host arrays (llcomp_mi_paste32_reference): src and dst as paste_reference's, mask
    [n_src, ih, iw, 3] uint8 or [n_src, ih, iw] uint32 -- or src itself where src IS the id maps: uint8 "hwc" with c = 3 (map_bytes 3)
    or c = 4, or float32 with c = 1 (map_bytes 4) -> the pasted dst batch, a new array."""
    d, code, lay, n_dst, c, oh, ow = _batch_array(dst, dtype, layout)
    s = np.ascontiguousarray(src)
    if s.ndim != 4 or s.dtype != d.dtype or (s.shape[1] if lay == LAYOUT_CHW else s.shape[3]) != c:
        raise LlcompError(BAD_ARGS, f"src is a 4-D batch of dst's type and channels, got {s.dtype} of shape {s.shape}")
    n_src = s.shape[0]
    ih, iw = s.shape[2:] if lay == LAYOUT_CHW else s.shape[1:3]
    if mask is src:
        m, mb = s, s.nbytes // max(n_src * ih * iw, 1)
    else:
        m, mb = _wide_maps(mask)[:2]
    if mb not in (3, 4) or m.nbytes != mb * n_src * ih * iw:
        raise LlcompError(BAD_ARGS, f"mask is uint8 [n_src, ih, iw, 3] or uint32 [n_src, ih, iw], got {m.dtype} of shape {m.shape}")
    recs = paste_pieces32(pieces, mb)
    out = np.empty_like(d)
    _check(_lib.load().llcomp_mi_paste32_reference(s.ctypes.data, m.ctypes.data, mb, n_src, iw, ih, d.ctypes.data, n_dst, ow, oh, c, code, lay, recs,
                                                   len(recs), out.ctypes.data))
    return out


# Codec.alpha_paste_batch (LLCOMP_MI_ALPHA_*): a piece's flags
ALPHA_VALUE = 1
ALPHA_VALUE_PIXEL = 2
ALPHA_OVER = 4


def alpha_pieces(records):
    """The pieces of an alpha_paste_batch call (llcomp_mi_alpha_piece) as a ctypes array: every record a tuple (dst, src, dx, dy, sx,
    sy, w, h[, flags[, value_bits]]).  flags: 0 for PIL's paste under the alpha, ALPHA_VALUE for value_bits (the element's bits) as the
    source in every channel, ALPHA_VALUE | ALPHA_VALUE_PIXEL for byte ch of value_bits in channel ch (uint8 "hwc", c <= 4: PIL's paste
    of a colour), ALPHA_OVER for Image.alpha_composite.  The pieces apply in order.  The library checks the rest."""
    if isinstance(records, C.Array) and records._type_ is AlphaPiece:
        return records
    rows = list(records)
    arr = (AlphaPiece * len(rows))()
    for i, r in enumerate(rows):
        vals = list(r) if isinstance(r, (tuple, list)) else []
        if len(vals) not in (8, 9, 10):
            raise LlcompError(BAD_ARGS, f"a piece is (dst, src, dx, dy, sx, sy, w, h[, flags[, value_bits]]), got {r!r}")
        nums = [int(v) for v in vals] + [0] * (10 - len(vals))
        if min(nums) < 0 or max(nums) > 0xFFFFFFFF:
            raise LlcompError(BAD_ARGS, f"a piece takes unsigned values, got {r!r}")
        for name, v in zip(("dst", "src", "dx", "dy", "sx", "sy", "w", "h", "flags", "value_bits"), nums):
            setattr(arr[i], name, v)
    return arr


def alpha_paste_plan(alpha_px_bytes, alpha_byte, n_src, iw, ih, n_dst, ow, oh, c, pieces, dtype="float32", layout="chw"):
    """What an alpha_paste_batch call does (llcomp_mi_alpha_paste_plan, host only) -> (samples, first, order, n_workgroups), as
    paste_plan: the ignored pieces are those with w or h of 0."""
    recs = alpha_pieces(pieces)
    n_dst = int(n_dst)
    samples, first, order = np.zeros(max(n_dst, 1), np.uint32), np.zeros(max(n_dst, 1) + 1, np.uint32), np.zeros(max(len(recs), 1), np.uint32)
    ns, nw = C.c_uint32(0), C.c_uint64(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_alpha_paste_plan(int(alpha_px_bytes), int(alpha_byte), int(n_src), int(iw), int(ih), n_dst, int(ow), int(oh), int(c),
                                                  _dtype_code(dtype), _layout_code(layout), recs, len(recs), samples.ctypes.data_as(u32p),
                                                  first.ctypes.data_as(u32p), order.ctypes.data_as(u32p), C.byref(ns), C.byref(nw)))
    n = ns.value
    return samples[:n].copy(), first[:n + 1].copy(), order[:int(first[n])].copy(), int(nw.value)


def alpha_paste_reference(src, alpha, dst, pieces, layout="chw", dtype=None, alpha_byte=0):
    """The rule of the batch alpha paste on host arrays (llcomp_mi_alpha_paste_reference): src and dst as paste_reference's (src None
    when every piece is a VALUE piece); alpha uint8 [n_src, ih, iw] or [n_src, ih, iw, alpha_px_bytes] with a pixel's alpha in byte
    alpha_byte -- or src itself, a uint8 "hwc" batch with c <= 4 (RGBA under its own A: alpha_byte 3) -- or None when every piece is an
    OVER piece -> the blended dst batch, a new array."""
    d, code, lay, n_dst, c, oh, ow = _batch_array(dst, dtype, layout)
    s = None if src is None else np.ascontiguousarray(src)
    if s is not None and (s.ndim != 4 or s.dtype != d.dtype or (s.shape[1] if lay == LAYOUT_CHW else s.shape[3]) != c):
        raise LlcompError(BAD_ARGS, f"src is a 4-D batch of dst's type and channels, got {s.dtype} of shape {s.shape}")
    m = s if alpha is src else None if alpha is None else np.ascontiguousarray(alpha)
    if m is not None and (m.dtype != np.uint8 or m.ndim not in (3, 4)):
        raise LlcompError(BAD_ARGS, f"alpha is uint8 [n_src, ih, iw] or [n_src, ih, iw, alpha_px_bytes], got {m.dtype} of shape {m.shape}")
    if s is not None:
        n_src = s.shape[0]
        ih, iw = s.shape[2:] if lay == LAYOUT_CHW else s.shape[1:3]
    elif m is not None:
        n_src, ih, iw = m.shape[:3]
    else:
        raise LlcompError(BAD_ARGS, "a call reads src or alpha")
    apx = 1 if m is None else m.nbytes // max(n_src * ih * iw, 1)
    if m is not None and m.nbytes != apx * n_src * ih * iw:
        raise LlcompError(BAD_ARGS, f"alpha is n_src x ih x iw pixels, got shape {m.shape}")
    recs = alpha_pieces(pieces)
    out = np.empty_like(d)
    _check(_lib.load().llcomp_mi_alpha_paste_reference(None if s is None else s.ctypes.data, None if m is None else m.ctypes.data, apx, int(alpha_byte),
                                                       n_src, iw, ih, d.ctypes.data, n_dst, ow, oh, c, code, lay, recs, len(recs), out.ctypes.data))
    return out


def paste16_plan(n_src, iw, ih, n_dst, ow, oh, c, pieces, dtype="float32", layout="chw"):
    """What a paste_batch16 call does (llcomp_mi_paste16_plan, host only) -> (samples, first, order, n_workgroups), as paste_plan; order
    indexes the pieces of paste_pieces16(pieces), one per window."""
    recs = paste_pieces16(pieces)
    n_dst = int(n_dst)
    samples, first, order = np.zeros(max(n_dst, 1), np.uint32), np.zeros(max(n_dst, 1) + 1, np.uint32), np.zeros(max(len(recs), 1), np.uint32)
    ns, nw = C.c_uint32(0), C.c_uint64(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_paste16_plan(int(n_src), int(iw), int(ih), n_dst, int(ow), int(oh), int(c), _dtype_code(dtype), _layout_code(layout),
                                              recs, len(recs), samples.ctypes.data_as(u32p), first.ctypes.data_as(u32p), order.ctypes.data_as(u32p),
                                              C.byref(ns), C.byref(nw)))
    n = ns.value
    return samples[:n].copy(), first[:n + 1].copy(), order[:int(first[n])].copy(), int(nw.value)


def paste16_reference(src, mask, dst, pieces, layout="chw", dtype=None):
    """The rule of the batch copy-paste by 16-bit ids on host arrays (llcomp_mi_paste16_reference): src and dst as paste_reference's,
    mask [n_src, ih, iw] uint16 -- or src itself where src IS the id maps: uint8 "hwc" with c = 2, or a 2-byte dtype with c = 1 -> the
    pasted dst batch, a new array."""
    d, code, lay, n_dst, c, oh, ow = _batch_array(dst, dtype, layout)
    s = np.ascontiguousarray(src)
    if s.ndim != 4 or s.dtype != d.dtype or (s.shape[1] if lay == LAYOUT_CHW else s.shape[3]) != c:
        raise LlcompError(BAD_ARGS, f"src is a 4-D batch of dst's type and channels, got {s.dtype} of shape {s.shape}")
    n_src = s.shape[0]
    ih, iw = s.shape[2:] if lay == LAYOUT_CHW else s.shape[1:3]
    m = s if mask is src else np.ascontiguousarray(mask)
    if (m is not s and m.dtype != np.uint16) or m.nbytes != 2 * n_src * ih * iw:
        raise LlcompError(BAD_ARGS, f"mask is uint16 [n_src, ih, iw], got {m.dtype} of shape {m.shape}")
    recs = paste_pieces16(pieces)
    out = np.empty_like(d)
    _check(_lib.load().llcomp_mi_paste16_reference(s.ctypes.data, m.ctypes.data, n_src, iw, ih, d.ctypes.data, n_dst, ow, oh, c, code, lay, recs,
                                                   len(recs), out.ctypes.data))
    return out


# a record of Codec.label_boxes (llcomp_mi_label_box): the pixels of an id and their box [x0, x1) x [y0, y1)
LABEL_BOX_DTYPE = np.dtype([("count", "<u4"), ("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4")])


def label_boxes_rows():
    """the rows of the band of a sample that a workgroup of the label boxes' kernel takes (llcomp_mi_label_boxes_rows)"""
    return int(_lib.load().llcomp_mi_label_boxes_rows())


def label_boxes_reference(maps):
    """The rule of the label boxes on a host array (llcomp_mi_label_boxes_reference): maps [n, oh, ow] uint8 -> [n, 256] records of
    LABEL_BOX_DTYPE; an id without a pixel has (0, ow, oh, 0, 0)."""
    a = np.ascontiguousarray(maps)
    if a.ndim != 3 or a.dtype != np.uint8:
        raise LlcompError(BAD_ARGS, f"maps are uint8 [n, oh, ow], got {a.dtype} of shape {a.shape}")
    n, oh, ow = a.shape
    out = np.zeros((max(n, 1), 256), LABEL_BOX_DTYPE)
    _check(_lib.load().llcomp_mi_label_boxes_reference(a.ctypes.data if a.size else None, n, ow, oh, out.ctypes.data))
    return out[:n]


def label_boxes16_max_ids():
    """the most ids a sample of label_boxes16 lists (llcomp_mi_label_boxes16_max_ids)"""
    return int(_lib.load().llcomp_mi_label_boxes16_max_ids())


def _label_lists(ids, n, id_type=np.uint16):
    """per-sample sequences of ids -> (ids of id_type [total], first uint32 [n + 1]); the library checks the order and the lengths"""
    lists = [np.asarray(list(l), np.int64).reshape(-1) for l in ids]
    if len(lists) != n:
        raise LlcompError(BAD_ARGS, f"ids holds one sequence per sample, got {len(lists)} for {n} samples")
    top = int(np.iinfo(id_type).max)
    if any(l.size and (l.min() < 0 or l.max() > top) for l in lists):
        raise LlcompError(BAD_ARGS, f"an id is 0..{top}")
    first = np.zeros(n + 1, np.uint32)
    first[1:] = np.cumsum([l.size for l in lists])
    flat = np.concatenate(lists + [np.zeros(0, np.int64)]).astype(id_type)
    return np.ascontiguousarray(np.append(flat, id_type(0))), first  # (a pointer that is never NULL)


def label_boxes16_reference(maps, ids):
    """The rule of the label boxes of listed ids on a host array (llcomp_mi_label_boxes16_reference): maps [n, oh, ow] uint16, ids a
    sequence of n sequences of ids, each strictly ascending -> a flat array of LABEL_BOX_DTYPE, one record per listed id in the lists'
    order; an id without a pixel has (0, ow, oh, 0, 0)."""
    a = np.ascontiguousarray(maps)
    if a.ndim != 3 or a.dtype != np.uint16:
        raise LlcompError(BAD_ARGS, f"maps are uint16 [n, oh, ow], got {a.dtype} of shape {a.shape}")
    n, oh, ow = a.shape
    flat, first = _label_lists(ids, n)
    out = np.zeros(max(int(first[n]), 1), LABEL_BOX_DTYPE)
    _check(_lib.load().llcomp_mi_label_boxes16_reference(a.ctypes.data if a.size else None, n, ow, oh, flat.ctypes.data, first.ctypes.data, out.ctypes.data))
    return out[:int(first[n])]


# label targets (LLCOMP_MI_TARGET_*; include/llcomp_mi.h "Label targets"): the two kinds, and INDEX's dtypes
TARGET_INDEX, TARGET_PLANES = 0, 1
TARGET_U8, TARGET_I32, TARGET_I64 = 0, 1, 2
TARGET_KINDS = ("index", "planes")
_TARGET_INDEX_DTYPES = {"uint8": (TARGET_U8, np.uint8), "int32": (TARGET_I32, np.int32), "int64": (TARGET_I64, np.int64)}


def label_targets_segment():
    """the pixels of the segment of a sample that a workgroup of the label targets' kernel takes (llcomp_mi_label_targets_segment)"""
    return int(_lib.load().llcomp_mi_label_targets_segment())


def label_targets_max_planes():
    """the most planes a sample of label_targets owns (llcomp_mi_label_targets_max_planes)"""
    return int(_lib.load().llcomp_mi_label_targets_max_planes())


def _target_bits(value, code):
    """a number -> the bits of the element of DTYPE_* `code` that holds it, converted on the host by numpy (bfloat16: float32 rounded
    to nearest even)"""
    if code == DTYPE_U8:
        if not 0 <= int(value) <= 255:
            raise LlcompError(BAD_ARGS, f"on and off of uint8 planes are 0..255, got {value!r}")
        return int(value)
    if code == DTYPE_F16:
        return int(np.array(value, np.float16).view(np.uint16))
    b = int(np.array(value, np.float32).view(np.uint32))
    return b if code == DTYPE_F32 else ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def _label_targets(ids, values, n, map_bytes, kind, dtype, default, planes, on, off):
    """the arguments of a label targets call -> (LabelTargets, what must stay alive, the numpy type of the output's elements, the
    output's planes or None); the library checks the lists, the values and the planes"""
    if isinstance(kind, str) and kind.lower() in TARGET_KINDS:
        kind = TARGET_KINDS.index(kind.lower())
    if kind not in (TARGET_INDEX, TARGET_PLANES):
        raise LlcompError(BAD_ARGS, f"kind must be one of {TARGET_KINDS}, got {kind!r}")
    wide = int(map_bytes) > 2  # (the wide id maps: uint32 ids, llcomp_mi_label_targets32)
    flat, first = _label_lists(ids, n, np.uint32 if wide else np.uint16)
    vals = [np.asarray(list(l), np.int64).reshape(-1) for l in values]
    if [v.size for v in vals] != np.diff(first.astype(np.int64)).tolist():
        raise LlcompError(BAD_ARGS, "values holds one value per listed id")
    flat_v = np.concatenate(vals + [np.zeros(1, np.int64)])
    if flat_v.min() < -0x80000000 or flat_v.max() > 0x7FFFFFFF or not -0x80000000 <= int(default) <= 0x7FFFFFFF:
        raise LlcompError(BAD_ARGS, "a value is an int32")
    flat_v = np.ascontiguousarray(flat_v.astype(np.int32))
    struct = _lib.LabelTargets32 if wide else _lib.LabelTargets
    t = struct(C.sizeof(struct), int(map_bytes), kind, 0, int(default), 0, 0, flat.ctypes.data, flat_v.ctypes.data, first.ctypes.data, None)
    keep = [flat, flat_v, first]
    if kind == TARGET_INDEX:
        name = "int64" if dtype is None else str(dtype).replace("torch.", "")
        if name not in _TARGET_INDEX_DTYPES:
            raise LlcompError(BAD_ARGS, f"dtype of an index tensor must be uint8, int32 or int64, got {dtype!r}")
        t.dtype, np_type = _TARGET_INDEX_DTYPES[name]
        return t, keep, np_type, None
    t.dtype = _dtype_code(dtype)
    if planes is None:
        raise LlcompError(BAD_ARGS, "planes= is an int, or one count per sample")
    counts = [int(planes)] * n if isinstance(planes, (int, np.integer)) else [int(k) for k in planes]
    if len(counts) != n or any(k < 0 or k > 0xFFFF for k in counts):
        raise LlcompError(BAD_ARGS, f"planes holds one count per sample, got {len(counts)} for {n} samples")
    plane_first = np.zeros(n + 1, np.uint32)
    plane_first[1:] = np.cumsum(counts)
    keep.append(plane_first)
    t.plane_first = plane_first.ctypes.data
    t.on_bits = _target_bits(1 if on is None else on, t.dtype)
    t.off_bits = _target_bits(0 if off is None else off, t.dtype)
    return t, keep, _NP_OF_DTYPE[t.dtype], counts


def label_targets_reference(maps, ids, values, kind="index", dtype=None, default=0, planes=None, on=None, off=None):
    """The rule of the label targets on a host array (llcomp_mi_label_targets_reference): maps [n, oh, ow] uint8 or uint16; ids a
    sequence of n sequences of ids, each strictly ascending, values one int32 per listed id; a pixel's value is its id's, or `default`.
    kind "index" -> [n, oh, ow] of dtype uint8, int32 or int64 (the default).  kind "planes" -> the planes whose index the pixel's value
    is hold `on` (1), the others `off` (0), in dtype uint8 (the default), float32, float16 or bfloat16 (as uint16 bit patterns):
    [n, K, oh, ow] for planes=K, [sum of planes, oh, ow] for one count per sample."""
    a = np.ascontiguousarray(maps)
    if a.ndim != 3 or a.dtype not in (np.uint8, np.uint16):
        raise LlcompError(BAD_ARGS, f"maps are uint8 or uint16 [n, oh, ow], got {a.dtype} of shape {a.shape}")
    n, oh, ow = a.shape
    t, keep, np_type, counts = _label_targets(ids, values, n, a.itemsize, kind, dtype, default, planes, on, off)
    shape = (n, oh, ow) if counts is None else (n, counts[0], oh, ow) if isinstance(planes, (int, np.integer)) else (sum(counts), oh, ow)
    out = np.zeros(int(np.prod(shape)) + 1, np_type)
    _check(_lib.load().llcomp_mi_label_targets_reference(a.ctypes.data if a.size else None, n, ow, oh, C.byref(t), out.ctypes.data))
    return out[:-1].reshape(shape)


def _wide_maps(maps):
    """host id maps of 3 or 4 bytes per pixel (include/llcomp_mi.h "Wide id maps") -> (the array, map_bytes, n, oh, ow):
    [n, oh, ow, 3] uint8, the id b0 | b1 << 8 | b2 << 16, or [n, oh, ow] uint32"""
    a = np.ascontiguousarray(maps)
    if a.ndim == 4 and a.shape[3] == 3 and a.dtype == np.uint8:
        return a, 3, a.shape[0], a.shape[1], a.shape[2]
    if a.ndim == 3 and a.dtype == np.uint32:
        return a, 4, a.shape[0], a.shape[1], a.shape[2]
    raise LlcompError(BAD_ARGS, f"wide id maps are uint8 [n, oh, ow, 3] or uint32 [n, oh, ow], got {a.dtype} of shape {a.shape}")


def label_boxes32_reference(maps, ids):
    """label_boxes16_reference for id maps of 3 or 4 bytes per pixel (llcomp_mi_label_boxes32_reference): maps [n, oh, ow, 3] uint8 or
    [n, oh, ow] uint32, ids a sequence of n strictly ascending sequences of ids up to 0xFFFFFF or 0xFFFFFFFF."""
    a, mb, n, oh, ow = _wide_maps(maps)
    flat, first = _label_lists(ids, n, np.uint32)
    out = np.zeros(max(int(first[n]), 1), LABEL_BOX_DTYPE)
    _check(_lib.load().llcomp_mi_label_boxes32_reference(a.ctypes.data if a.size else None, mb, n, ow, oh, flat.ctypes.data, first.ctypes.data, out.ctypes.data))
    return out[:int(first[n])]


def label_targets32_reference(maps, ids, values, kind="index", dtype=None, default=0, planes=None, on=None, off=None):
    """label_targets_reference for id maps of 3 or 4 bytes per pixel (llcomp_mi_label_targets32_reference): maps [n, oh, ow, 3] uint8
    or [n, oh, ow] uint32; everything else as there."""
    a, mb, n, oh, ow = _wide_maps(maps)
    t, keep, np_type, counts = _label_targets(ids, values, n, mb, kind, dtype, default, planes, on, off)
    shape = (n, oh, ow) if counts is None else (n, counts[0], oh, ow) if isinstance(planes, (int, np.integer)) else (sum(counts), oh, ow)
    out = np.zeros(int(np.prod(shape)) + 1, np_type)
    _check(_lib.load().llcomp_mi_label_targets32_reference(a.ctypes.data if a.size else None, n, ow, oh, C.byref(t), out.ctypes.data))
    return out[:-1].reshape(shape)


def _view_groups(groups, c, signed=False):
    """a sequence of ViewGroup (or (views, ow, oh[, d_out]) tuples) -> (ctypes array of llcomp_mi_view_group, n, keep-alive list);
    everything about their contents is the library's to refuse.  signed (a padded call): a view's x and y may be negative, and go into
    the struct as two's complement"""
    groups = list(groups) if groups is not None else []
    arr, keep = (_ViewGroup * max(1, len(groups)))(), []
    for i, gr in enumerate(groups):
        if not isinstance(gr, ViewGroup):
            if not isinstance(gr, (tuple, list)) or not 3 <= len(gr) <= 4:
                raise LlcompError(BAD_ARGS, f"group {i} must be a ViewGroup or (views, ow, oh, d_out)")
            gr = ViewGroup(*gr)
        a = np.asarray(gr.views if len(gr.views) else np.zeros((0, 6), np.int64))
        if a.ndim != 2 or a.shape[1] not in (5, 6) or not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
            ok = signed and a.ndim == 2 and a.shape[1] in (5, 6) and np.issubdtype(a.dtype, np.integer) and a.max() <= 0x7FFFFFFF \
                and a[:, 1:3].min() >= -0x80000000 and np.delete(a, (1, 2), axis=1).min() >= 0
            if not ok:
                raise LlcompError(BAD_ARGS, f"the views of group {i} must be n x 5 or n x 6 non-negative integers, got shape {a.shape} {a.dtype}")
            a = a.astype(np.int64)
            a[:, 1:3] &= 0xFFFFFFFF
        n = a.shape[0]
        if a.shape[1] == 5:
            a = np.concatenate([a, np.zeros((n, 1), a.dtype)], axis=1)
        fl = _flags_table(a[:, 5] & 0xFF, n, gr.filter) if n else None
        views = (_View * max(1, n))(*[_View(*[int(v) for v in row[:5]], int(fl[j])) for j, row in enumerate(a.tolist())])
        fmt, _, keep_fmt = _output_format(c, **gr.format)
        keep += [views, keep_fmt]
        arr[i] = _ViewGroup(C.sizeof(_ViewGroup), n, C.cast(views, C.POINTER(_View)) if n else None, int(gr.ow), int(gr.oh),
                            C.pointer(fmt) if fmt is not None else None, gr.d_out or None)
    return arr, len(groups), keep


def views_plan(w, h, c, tile_w, tile_h, planar, frames, groups):
    """(unions, windows, n_used, n_classes) of a views decode (llcomp_mi_views_plan, host only): unions [frames, 4] = every frame's
    bounding box (x, y, rw, rh) of its views over all groups, zeros for a frame without a view; windows [frames, 4] and n_classes =
    resized_regions_plan of the used frames' unions.  groups: ViewGroup objects or (views, ow, oh) tuples.  LlcompError(BAD_ARGS) as the
    header lists: no groups, an empty group, a view of a frame >= frames, a rectangle empty or outside the image, an unknown filter, a
    downscale above the filter's limit."""
    arr, n, _keep = _view_groups(groups, c)
    uni, win = np.zeros((frames, 4), np.uint32), np.zeros((frames, 4), np.uint32)
    used, k = C.c_uint32(), C.c_uint32()
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_views_plan(w, h, c, tile_w, tile_h, int(bool(planar)), frames, arr, n, uni.ctypes.data_as(u32p),
                                            win.ctypes.data_as(u32p), C.byref(used), C.byref(k)))
    return uni, win, used.value, k.value


class WarpGroup:
    """Views under an affine map that share one output (llcomp_mi_warp_group): views = a sequence of (frame, m0, m1, m2, m3, m4, m5) or
    (frame, m0, ..., m5, flags) -- PIL's AFFINE data: output pixel (x, y) reads the frame at (m0 x + m1 y + m2, m3 x + m4 y + m5), pixel
    centres at + 0.5 -- the output is [n][oh][ow][c] at device address d_out in the format dtype, layout, scale, mean and std give;
    filter: "nearest", "bilinear" or "bicubic" (or its FILTER_* code) for every view of the group, or one per view, OR-ed into bits 4-6
    of the views' flags; fill: c values 0..255 for what lies outside the frame (None: zeros)."""

    def __init__(self, views, ow, oh, d_out=0, dtype=None, layout="hwc", scale=False, mean=None, std=None, filter=None, fill=None, photo=None):
        self.views, self.ow, self.oh, self.d_out = views, ow, oh, d_out
        self.format = dict(dtype=dtype, layout=layout, scale=scale, mean=mean, std=std)
        self.filter, self.fill = filter, fill
        self.photo = photo  # (a photometric chain for every view, or one per view: ViewGroup)


class PerspectiveGroup(WarpGroup):
    """Views under a projective map that share one output (llcomp_mi_perspective_group): views = a sequence of (frame, a0, ..., a7) or
    (frame, a0, ..., a7, flags) -- PIL's PERSPECTIVE data: output pixel (x, y) reads the frame at ((a0 x + a1 y + a2) / (a6 x + a7 y + 1),
    (a3 x + a4 y + a5) / (a6 x + a7 y + 1)), pixel centres at + 0.5; perspective_coeffs gives them from four point pairs.  Everything
    else as WarpGroup takes it."""


def _matrix(m, n=6):
    a = np.asarray(m, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise LlcompError(BAD_ARGS, f"{'an affine' if n == 6 else 'a perspective'} map takes {n} numbers, got {a.size}")
    return (C.c_double * n)(*a.tolist())


def _warp_groups(groups, c, persp=False):
    """a sequence of WarpGroup (or (views, ow, oh[, d_out]) tuples) -> (ctypes array of llcomp_mi_warp_group, n, keep-alive list);
    everything about their contents is the library's to refuse.  persp: PerspectiveGroup -> llcomp_mi_perspective_group, eight numbers."""
    groups = list(groups) if groups is not None else []
    Group, CGroup, CView, k = (PerspectiveGroup, _PerspectiveGroup, _PerspectiveView, 8) if persp else (WarpGroup, _WarpGroup, _WarpView, 6)
    arr, keep = (CGroup * max(1, len(groups)))(), []
    for i, gr in enumerate(groups):
        if not isinstance(gr, Group):
            if not isinstance(gr, (tuple, list)) or not 3 <= len(gr) <= 4:
                raise LlcompError(BAD_ARGS, f"group {i} must be a {Group.__name__} or (views, ow, oh, d_out)")
            gr = Group(*gr)
        rows = [list(v) for v in gr.views]
        n = len(rows)
        if any(len(r) not in (k + 1, k + 2) for r in rows):
            raise LlcompError(BAD_ARGS, f"the views of group {i} must be (frame, {k} numbers) or (frame, {k} numbers, flags)")
        frames = [int(r[0]) for r in rows]
        fl = [int(r[k + 1]) if len(r) == k + 2 else 0 for r in rows]
        if any(not 0 <= f <= 0xFFFFFFFF for f in frames) or any(not 0 <= f <= 255 for f in fl):
            raise LlcompError(BAD_ARGS, f"group {i}: a frame index or flags byte out of range")
        fl = _flags_table(fl, n, gr.filter) if n else None
        views = (CView * max(1, n))(*[CView(frames[j], int(fl[j]), _matrix(rows[j][1:k + 1], k)) for j in range(n)])
        fmt, _, keep_fmt = _output_format(c, **gr.format)
        fill = None
        if gr.fill is not None:
            f = np.asarray(gr.fill).reshape(-1)
            if f.size == 1:
                f = np.full(c, f[0])
            if f.size != c or f.min() < 0 or f.max() > 255:
                raise LlcompError(BAD_ARGS, f"fill takes {c} values in 0..255")
            fill = (C.c_uint8 * c)(*[int(v) for v in f.tolist()])
        keep += [views, keep_fmt, fill]
        arr[i] = CGroup(C.sizeof(CGroup), n, C.cast(views, C.POINTER(CView)) if n else None, int(gr.ow), int(gr.oh),
                            C.pointer(fmt) if fmt is not None else None, gr.d_out or None, C.cast(fill, _lib.u8p) if fill is not None else None)
    return arr, len(groups), keep


def warp_source_rect(w, h, m, filter, ow, oh):
    """((x, y, rw, rh), empty) of one view under an affine map (llcomp_mi_warp_source_rect, host only): the bounding box of the frame's
    pixels the rule reads for the output pixels that lie inside the frame; empty = True (and four zeros) when none does.
    LlcompError(BAD_ARGS) for the rule's limits."""
    rect, empty = (C.c_uint32 * 4)(), C.c_uint32()
    _check(_lib.load().llcomp_mi_warp_source_rect(w, h, _matrix(m), filter_code(filter), ow, oh, rect, C.byref(empty)))
    return tuple(rect), bool(empty.value)


def warp_views_plan(w, h, c, tile_w, tile_h, planar, frames, groups):
    """(unions, windows, n_used, n_classes) of a warped views decode (llcomp_mi_warp_views_plan, host only), in the shape of views_plan:
    a frame's union is the bounding box of its views' source rectangles; a frame whose views are all empty is unused."""
    arr, n, _keep = _warp_groups(groups, c)
    uni, win = np.zeros((frames, 4), np.uint32), np.zeros((frames, 4), np.uint32)
    used, k = C.c_uint32(), C.c_uint32()
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_warp_views_plan(w, h, c, tile_w, tile_h, int(bool(planar)), frames, arr, n, uni.ctypes.data_as(u32p),
                                                 win.ctypes.data_as(u32p), C.byref(used), C.byref(k)))
    return uni, win, used.value, k.value


def perspective_source_rect(w, h, a, filter, ow, oh):
    """((x, y, rw, rh), empty) of one view under a projective map (llcomp_mi_perspective_source_rect, host only): a rectangle that
    contains every pixel of the frame the rule reads for the output pixels inside the frame -- a bound, at most a pixel beyond them on
    any side; empty = True (and four zeros) exactly when no output pixel is inside.  LlcompError(BAD_ARGS) for the rule's limits."""
    rect, empty = (C.c_uint32 * 4)(), C.c_uint32()
    _check(_lib.load().llcomp_mi_perspective_source_rect(w, h, _matrix(a, 8), filter_code(filter), ow, oh, rect, C.byref(empty)))
    return tuple(rect), bool(empty.value)


def perspective_views_plan(w, h, c, tile_w, tile_h, planar, frames, groups):
    """(unions, windows, n_used, n_classes) of a perspective views decode (llcomp_mi_perspective_views_plan, host only), in the shape of
    views_plan: a frame's union is the bounding box of its views' source rectangles; a frame whose views are all empty is unused."""
    arr, n, _keep = _warp_groups(groups, c, persp=True)
    uni, win = np.zeros((frames, 4), np.uint32), np.zeros((frames, 4), np.uint32)
    used, k = C.c_uint32(), C.c_uint32()
    u32p = C.POINTER(C.c_uint32)
    _check(_lib.load().llcomp_mi_perspective_views_plan(w, h, c, tile_w, tile_h, int(bool(planar)), frames, arr, n, uni.ctypes.data_as(u32p),
                                                        win.ctypes.data_as(u32p), C.byref(used), C.byref(k)))
    return uni, win, used.value, k.value


def perspective_reference(frame, a, filter="nearest", ow=None, oh=None, fill=None):
    """The rule of the perspective views on a host image (llcomp_mi_perspective_reference): frame [h, w] or [h, w, c] uint8 ->
    [oh, ow(, c)], byte for byte PIL's Image.transform((ow, oh), Image.PERSPECTIVE, a, resample, fillcolor=fill) with independent bands.
    ow / oh default to the frame's size."""
    return warp_reference(frame, a, filter, ow, oh, fill, _persp=True)


def perspective_coeffs(startpoints, endpoints):
    """The eight numbers of the projective map that sends the output's `endpoints` to the source's `startpoints` (four (x, y) pairs
    each), as torchvision's RandomPerspective pairs them: the least-squares solution, in binary64, of the 8 x 8 system that
    torchvision's _get_perspective_coeffs sets up.  It is that system, not necessarily torchvision's last bits (torchvision solves it
    with its own routine, in its own precision): the byte-for-byte contract of the perspective calls is on the coefficients a caller
    passes, whatever produced them -- pass torchvision's own to reproduce torchvision."""
    sp, ep = np.asarray(startpoints, np.float64).reshape(-1, 2), np.asarray(endpoints, np.float64).reshape(-1, 2)
    if sp.shape != (4, 2) or ep.shape != (4, 2):
        raise LlcompError(BAD_ARGS, "startpoints and endpoints are four (x, y) pairs each")
    A = np.zeros((8, 8), np.float64)
    for i in range(4):
        (x, y), (u, v) = ep[i], sp[i]
        A[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
    return tuple(np.linalg.lstsq(A, sp.reshape(8), rcond=None)[0].tolist())


def warp_reference(frame, m, filter="nearest", ow=None, oh=None, fill=None, _persp=False):
    """The rule of the warped views on a host image (llcomp_mi_warp_reference): frame [h, w] or [h, w, c] uint8 -> [oh, ow(, c)], byte
    for byte PIL's Image.transform((ow, oh), Image.AFFINE, m, resample, fillcolor=fill) with independent bands.  ow / oh default to the
    frame's size (Image.rotate's output)."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    if a.ndim not in (2, 3) or not a.size:
        raise LlcompError(BAD_ARGS, f"a frame is [h, w] or [h, w, c], got shape {a.shape}")
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    ow, oh = int(w if ow is None else ow), int(h if oh is None else oh)
    if not (0 < ow <= 0xFFFFFFFF and 0 < oh <= 0xFFFFFFFF):
        raise LlcompError(BAD_ARGS, f"no output of {ow} x {oh}")
    fl = None
    if fill is not None:
        f = np.asarray(fill).reshape(-1)
        f = np.full(c, f[0]) if f.size == 1 else f
        if f.size != c or f.min() < 0 or f.max() > 255:
            raise LlcompError(BAD_ARGS, f"fill takes {c} values in 0..255")
        fl = np.ascontiguousarray(f, dtype=np.uint8)
    out = np.zeros((oh, ow) + a.shape[2:], np.uint8)
    L = _lib.load()
    rule = L.llcomp_mi_perspective_reference if _persp else L.llcomp_mi_warp_reference
    _check(rule(a.ctypes.data, w, h, c, _matrix(m, 8 if _persp else 6), filter_code(filter), fl.ctypes.data if fl is not None else None, ow, oh,
                out.ctypes.data))
    return out


def rotate_matrix(w, h, angle, center=None, translate=None):
    """The six numbers PIL's Image.rotate(angle, expand=False, center=center, translate=translate) builds for a w x h image -- degrees
    counter clockwise, the entries rounded to 15 decimals as PIL rounds them -- so warp_reference(frame, rotate_matrix(w, h, angle),
    filter) is Image.rotate for angles that are no multiples of 90 (at those PIL transposes instead)."""
    import math

    tx, ty = (0, 0) if translate is None else translate
    cx, cy = (w / 2, h / 2) if center is None else center
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx - tx, -cy - ty
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def pack_batch(containers):
    """(payload, slice_len) for Codec.decode / decode_region / decode_regions from single-frame SLICED containers of one shape, tiling,
    planar setting and model: the payloads back to back (np.uint8) and the slice tables back to back (np.uint32), in container order.
    LlcompError(BAD_ARGS) for an empty list, a LEGACY stream or a container that differs from the first; TRUNCATED for one whose payload
    is shorter than its table says (bytes after the last slice are dropped)."""
    if not containers:
        raise LlcompError(BAD_ARGS, "no containers")
    pays, lens, key0 = [], [], None
    for i, d in enumerate(containers):
        d = bytes(d)
        info = probe(d)
        key = (info.format, info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar, info.small_model, info.n_slices)
        if info.format != FORMAT_SLICED:
            raise LlcompError(BAD_ARGS, f"container {i} is not SLICED")
        if key0 is None:
            key0 = key
        elif key != key0:
            raise LlcompError(BAD_ARGS, f"container {i} differs from container 0 in shape, tiling, planar setting or model")
        t = np.frombuffer(d, dtype="<u4", count=info.n_slices, offset=info.table_offset).astype(np.uint32)
        n = int(t.sum(dtype=np.uint64))
        if len(d) - info.payload_offset < n:
            raise LlcompError(TRUNCATED, f"container {i} holds fewer payload bytes than its table says")
        lens.append(t)
        pays.append(np.frombuffer(d, dtype=np.uint8, count=n, offset=info.payload_offset))
    return np.concatenate(pays), np.concatenate(lens)


def _containers(containers):
    """(void* array, size_t array, keep-alive list) of a list of containers: bytes, bytearray, memoryview or contiguous uint8 arrays, passed
    without a copy"""
    keep, ptrs = [], []
    for d in containers:
        if isinstance(d, bytes):
            ptrs.append(C.cast(C.c_char_p(d), C.c_void_p).value)
        else:
            d = np.frombuffer(d, dtype=np.uint8) if not isinstance(d, np.ndarray) else d
            if d.dtype != np.uint8 or not d.flags["C_CONTIGUOUS"]:
                raise LlcompError(BAD_ARGS, "a container must be bytes or a contiguous uint8 array")
            ptrs.append(d.ctypes.data if d.size else C.cast(C.c_char_p(b""), C.c_void_p).value)
        keep.append(d)
    return (C.c_void_p * max(1, len(keep)))(*ptrs), (C.c_size_t * max(1, len(keep)))(*[len(d) if isinstance(d, bytes) else d.size for d in keep]), keep


def _frame_containers(containers, frames, allow_none=False):
    """_containers of exactly `frames` containers, one per frame of a codec.  allow_none: the container of a frame that the call never
    reads may be None -- it goes as a NULL pointer of length 0"""
    conts = list(containers)
    if allow_none and len(conts) != frames:
        raise LlcompError(BAD_ARGS, f"the codec takes {frames} containers, got {len(conts)}")
    ptrs, lens, keep = _containers([b"" if allow_none and d is None else d for d in conts])
    if len(keep) != frames:
        raise LlcompError(BAD_ARGS, f"the codec takes {frames} containers, got {len(keep)}")
    for f, d in enumerate(conts):
        if allow_none and d is None:
            ptrs[f], lens[f] = None, 0
    return ptrs, lens, keep


def regions_gather(containers, xy, rw, rh):
    """(payload np.uint8, slice_len np.uint32, n_classes): the table entries and payload bytes of every frame's window (regions_plan) of
    single-frame SLICED containers, class by class, frame order inside a class -- exactly what a regions decode of them reads
    (llcomp_mi_regions_gather, host only).  LlcompError as llcomp_mi_regions_gather reports it."""
    L = _lib.load()
    ptrs, lens, keep = _containers(containers)
    tab, n = _xy_table(xy, len(keep))
    nb, ns, nc = C.c_uint64(), C.c_uint32(), C.c_uint32()
    _check(L.llcomp_mi_regions_gather(ptrs, lens, n, tab, rw, rh, None, 0, None, 0, C.byref(nb), C.byref(ns), C.byref(nc)))
    pay, sl = np.empty(max(1, nb.value), np.uint8), np.empty(max(1, ns.value), np.uint32)
    _check(L.llcomp_mi_regions_gather(ptrs, lens, n, tab, rw, rh, pay.ctypes.data, nb.value, sl.ctypes.data, ns.value, C.byref(nb), C.byref(ns),
                                      C.byref(nc)))
    return pay[:nb.value], sl[:ns.value], nc.value


def decompress_region(data, x, y, w, h, *, device=-1, small_model=False):
    """RawImage(pixels: np.uint8[h,w,c], w, h, c) of the rectangle (x, y, w, h) of the picture (llcomp_mi_decode_region): only the
    slices of the tiles it touches are read and decoded.  A region decode does not validate the rest of the container."""
    L = _lib.load()
    data = bytes(data)
    src = C.cast(C.c_char_p(data or b"\0"), _lib.u8p)
    px, c = _lib.u8p(), C.c_uint32()
    _check(L.llcomp_mi_decode_region(src, len(data), device, 1 if small_model else 0, x, y, w, h, C.byref(px), C.byref(c)))
    try:
        n = w * h * c.value
        pixels = np.ctypeslib.as_array(px, shape=(max(n, 1),))[:n].copy().reshape(h, w, c.value)
    finally:
        L.llcomp_mi_free(px)
    return RawImage(pixels, w, h, c.value)


def decompress_region_into(data, out, x, y, w, h, *, device=-1, small_model=False):
    """llcomp_mi_decode_region_into: `data` / `out` numpy uint8 arrays owned by the caller -> channels.  Raises
    LlcompError(OUTPUT_OVERFLOW) with .channels set (and `out` untouched) when `out` is smaller than w * h * channels."""
    L = _lib.load()
    c = C.c_uint32()
    rc = L.llcomp_mi_decode_region_into(data.ctypes.data, data.size, device, 1 if small_model else 0, x, y, w, h, out.ctypes.data, out.size,
                                        C.byref(c))
    if rc != OK:
        e = LlcompError(rc)
        e.channels = c.value
        raise e
    return c.value


def _as_u8(a):
    """a contiguous uint8 array of bytes-like or array input (kept alive by the caller for the call)"""
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a, dtype=np.uint8)
    return np.frombuffer(bytes(a), dtype=np.uint8)


def _take(L, out, n):
    """bytes of a buffer the library allocated, which is then freed"""
    try:
        return bytes(np.ctypeslib.as_array(out, shape=(max(n, 1),))[:n])
    finally:
        L.llcomp_mi_free(out)


def replace_slices(data, box, new_len, new_payload):
    """bytes of the SLICED container `data` with the slices of the tiles box = (tx0, ty0, tx1, ty1) (region_plan) replaced: new_len = the
    covered slices' new lengths, new_payload = their streams back to back, both in sub-slice order (tile row, tile column, plane); every
    other slice stays byte for byte (llcomp_mi_replace_slices, host only).  LlcompError as llcomp_mi_replace_slices reports it."""
    L = _lib.load()
    src = _as_u8(data)
    lens = np.ascontiguousarray(new_len, dtype=np.uint32)
    pay = _as_u8(new_payload)
    if pay.size < int(lens.sum(dtype=np.uint64)):
        raise LlcompError(BAD_ARGS, "new_payload is shorter than the sum of new_len")
    b = (C.c_uint32 * 4)(*[int(v) for v in box])
    out, n = _lib.u8p(), C.c_size_t()
    _check(L.llcomp_mi_replace_slices(src.ctypes.data, src.size, b, lens.ctypes.data, pay.ctypes.data if pay.size else src.ctypes.data, C.byref(out),
                                      C.byref(n)))
    return _take(L, out, n.value)


def replace_slices_into(data, box, new_len, new_payload, out):
    """llcomp_mi_replace_slices_into: `out` a numpy uint8 array owned by the caller -> bytes written.  Raises LlcompError(OUTPUT_OVERFLOW)
    with .needed set (and `out` untouched) when `out` is too small."""
    L = _lib.load()
    src = _as_u8(data)
    lens = np.ascontiguousarray(new_len, dtype=np.uint32)
    pay = _as_u8(new_payload)
    if pay.size < int(lens.sum(dtype=np.uint64)):
        raise LlcompError(BAD_ARGS, "new_payload is shorter than the sum of new_len")
    b = (C.c_uint32 * 4)(*[int(v) for v in box])
    n = C.c_size_t()
    rc = L.llcomp_mi_replace_slices_into(src.ctypes.data, src.size, b, lens.ctypes.data, pay.ctypes.data if pay.size else src.ctypes.data,
                                         out.ctypes.data, out.size, C.byref(n))
    if rc != OK:
        e = LlcompError(rc)
        e.needed = n.value
        raise e
    return n.value


def _patch(patch):
    p = np.ascontiguousarray(patch, dtype=np.uint8)
    if p.ndim == 2:
        p = p[:, :, None]
    if p.ndim != 3 or p.size == 0:
        raise LlcompError(BAD_ARGS, "patch must be [h][w][c] (or [h][w]) and not empty")
    return p


def _check_patch_channels(src, p):
    """the channel byte of either header against the patch (a container too short or of no known magic is left to the C call's verdict)"""
    at = {0x79: 1, 0x9C: 2}.get(int(src[0])) if src.size >= 3 else None
    if at is not None and int(src[at]) != p.shape[2]:
        raise LlcompError(BAD_ARGS, "the patch's channel count is not the container's")


def update_region(data, x, y, patch, *, device=-1, small_model=False):
    """bytes of the container `data` (either format) with the rectangle at (x, y) of the picture replaced by patch (np.uint8 [h][w][c]):
    byte for byte what a full encode of the modified picture gives, but only the slices of the tiles the rectangle touches are coded
    again and only their bytes cross PCIe (llcomp_mi_update_region).  The patch's channel count must be the container's."""
    L = _lib.load()
    src = _as_u8(data)
    p = _patch(patch)
    _check_patch_channels(src, p)
    out, n = _lib.u8p(), C.c_size_t()
    _check(L.llcomp_mi_update_region(src.ctypes.data, src.size, device, 1 if small_model else 0, x, y, p.shape[1], p.shape[0], p.ctypes.data,
                                     C.byref(out), C.byref(n)))
    return _take(L, out, n.value)


def update_region_into(data, out, x, y, patch, *, device=-1, small_model=False):
    """llcomp_mi_update_region_into: `data` / `out` numpy uint8 arrays owned by the caller -> bytes written.  Raises
    LlcompError(OUTPUT_OVERFLOW) with .needed set (and `out` untouched) when `out` is too small."""
    L = _lib.load()
    p = _patch(patch)
    _check_patch_channels(data, p)
    n = C.c_size_t()
    rc = L.llcomp_mi_update_region_into(data.ctypes.data, data.size, device, 1 if small_model else 0, x, y, p.shape[1], p.shape[0], p.ctypes.data,
                                        out.ctypes.data, out.size, C.byref(n))
    if rc != OK:
        e = LlcompError(rc)
        e.needed = n.value
        raise e
    return n.value


def trim():
    """Release the idle coding lanes the host-buffer calls keep for the next call of the same shape (GBs of HBM) and
    the device memory the library parks for reuse instead of returning it to the driver (csrc/devmem.hip)."""
    _lib.load().llcomp_mi_trim()


def set_pool_limit(bytes_per_device):
    """Device memory the library may keep parked per device (csrc/devmem.hip); 0 = return every block to the driver."""
    _lib.load().llcomp_mi_set_pool_limit(int(bytes_per_device))


def pool_idle_bytes():
    return int(_lib.load().llcomp_mi_pool_idle_bytes())


def reload_tuning():
    """Have the library read its test / tuning hooks (LLCOMP_MI_*) from the environment again."""
    _lib.load().llcomp_mi_reload_tuning()


class PinnedBuffer:
    """Pinned host memory from llcomp_mi_host_alloc, exposed as a numpy uint8 array (`.array`): copies between it and
    the GPU are plain DMA."""

    def __init__(self, nbytes):
        self._L = _lib.load()
        self.nbytes = int(nbytes)
        self.ptr = self._L.llcomp_mi_host_alloc(self.nbytes)
        if not self.ptr:
            raise LlcompError(NOMEM)
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, _lib.u8p), shape=(max(self.nbytes, 1),))[: self.nbytes]

    def close(self):
        if self.ptr:
            self.array = None
            self._L.llcomp_mi_host_free(self.ptr)
            self.ptr = None

    __del__ = close


def compress_image_into(rgb, width, height, channels, out, *, format=FORMAT_LEGACY, tile_w=0, tile_h=0, planar=False, device=-1, small_model=False,
                        devices=None, chunks_per_device=0):
    """llcomp_mi_encode_into: `rgb` and `out` are numpy uint8 arrays owned by the caller (pinned: PinnedBuffer.array);
    returns the container length.  Raises LlcompError(OUTPUT_OVERFLOW) with .needed set when `out` is too small."""
    L = _lib.load()
    o, _keep = _opts(format, tile_w, tile_h, planar, device, small_model, devices, chunks_per_device)
    n = C.c_size_t()
    rc = L.llcomp_mi_encode_into(rgb.ctypes.data, width, height, channels, C.byref(o), out.ctypes.data, out.size, C.byref(n))
    if rc != OK:
        e = LlcompError(rc)
        e.needed = n.value
        raise e
    return n.value


def decompress_image_into(data, out, *, device=-1, small_model=False, devices=None, chunks_per_device=0):
    """llcomp_mi_decode_into_flags / _into_devices: `data` / `out` numpy uint8 arrays owned by the caller -> (width, height, channels)."""
    L = _lib.load()
    w, h, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if devices is not None:
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        rc = L.llcomp_mi_decode_into_devices(data.ctypes.data, data.size, arr, len(devices), int(chunks_per_device), 1 if small_model else 0,
                                             out.ctypes.data, out.size, C.byref(w), C.byref(h), C.byref(c))
    else:
        rc = L.llcomp_mi_decode_into_flags(data.ctypes.data, data.size, device, 1 if small_model else 0, out.ctypes.data, out.size, C.byref(w), C.byref(h), C.byref(c))
    if rc != OK:
        e = LlcompError(rc)
        e.shape = (w.value, h.value, c.value)
        raise e
    return w.value, h.value, c.value


StreamJob = namedtuple("StreamJob", "slot kind status tag data")


class Stream:
    """Streaming pipeline (llcomp_mi_stream_*): frames of one shape, host -> GPU -> host, `depth` jobs in flight, a job =
    `frames_per_job` frames.  submit_* return False instead of blocking when every slot is occupied (back-pressure);
    wait() returns the oldest job as StreamJob, valid until release(job).  Its .data is a numpy view of the stream's pinned
    output buffer: frames_per_job == 1: the container (encode) / the frame [h,w,c] (decode); more frames per job: a list of
    containers (encode) / the frames [F,h,w,c] (decode)."""

    def __init__(self, w, h, c, tile_w=0, tile_h=0, planar=True, depth=4, device=-1, frames_per_job=1, devices=None):
        self._L = _lib.load()
        self._h = C.c_void_p()
        if devices is not None:  # one pipeline of `depth` slots per device behind one object, jobs dealt round-robin
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            _check(self._L.llcomp_mi_stream_create_multi(C.byref(self._h), arr, len(devices), w, h, c, tile_w, tile_h, int(bool(planar)), depth, frames_per_job))
        else:
            _check(self._L.llcomp_mi_stream_create_ex(C.byref(self._h), device, w, h, c, tile_w, tile_h, int(bool(planar)), depth, frames_per_job))
        self.n_devices = self._L.llcomp_mi_stream_devices(self._h)
        self.shape = (h, w, c)
        self._shapes = []  # (frame shape, numpy element type) of every pending job, in submission order (results come back in that order)
        self.frames_per_job = frames_per_job
        self.container_capacity = self._L.llcomp_mi_stream_container_capacity(self._h)

    def close(self):
        if self._h:
            self._L.llcomp_mi_stream_destroy(self._h)
            self._h = None

    __del__ = close

    def _submit(self, rc, shape=None, dtype=np.uint8):
        if rc == BUSY:
            return False
        _check(rc)
        self._shapes.append((shape or self.shape, dtype))
        return True

    def submit_encode(self, px, tag=0):
        """px: numpy uint8, frames_per_job frames [h,w,c] back to back (C-contiguous); must stay alive and unchanged until
        the job's result came back."""
        assert px.flags["C_CONTIGUOUS"] and px.dtype == np.uint8 and px.size == self.frames_per_job * self.shape[0] * self.shape[1] * self.shape[2]
        return self._submit(self._L.llcomp_mi_stream_submit_encode(self._h, px.ctypes.data, tag))

    def submit_decode(self, data, tag=0):
        """data: numpy uint8 container (frames_per_job == 1) or a list of frames_per_job containers -- e.g. the .data of an
        encode job that has not been released yet."""
        parts = [data] if self.frames_per_job == 1 and not isinstance(data, (list, tuple)) else list(data)
        assert len(parts) == self.frames_per_job and all(p.flags["C_CONTIGUOUS"] and p.dtype == np.uint8 for p in parts)
        ptrs = (C.c_void_p * len(parts))(*[p.ctypes.data for p in parts])
        lens = (C.c_size_t * len(parts))(*[p.size for p in parts])
        return self._submit(self._L.llcomp_mi_stream_submit_decode_batch(self._h, ptrs, lens, tag))

    def submit_decode_regions(self, containers, xy, rw, rh, tag=0):
        """frames_per_job containers (bytes or uint8 arrays) and their rectangles' origins xy ([frames_per_job, 2]) -> a job whose
        .data is the crop [rh,rw,c] (one frame per job) / the crops [F,rh,rw,c].  Only the windows' bytes cross PCIe; the containers
        are read during this call only and may be reused as soon as it returns."""
        ptrs, lens, keep = _containers(containers)
        if len(keep) != self.frames_per_job:
            raise LlcompError(BAD_ARGS, f"a job takes {self.frames_per_job} containers, got {len(keep)}")
        tab, _ = _xy_table(xy, self.frames_per_job)
        rc = self._L.llcomp_mi_stream_submit_decode_regions(self._h, ptrs, lens, tab, rw, rh, tag)
        return self._submit(rc, (rh, rw, self.shape[2]))

    def submit_decode_resized_regions(self, containers, rects, ow, oh, flags=None, tag=0, dtype=None, layout="hwc", scale=False, mean=None,
                                      std=None, filter=None):
        """frames_per_job containers, their rectangles rects ([frames_per_job, 4] of (x, y, rw, rh)), optional mirror flags and the
        filter (one for the job or one per frame, as Codec.decode_resized_regions takes it) -> a job
        whose .data is the output [oh,ow,c] (one frame per job) / [F,oh,ow,c] -- [c,oh,ow] / [F,c,oh,ow] for layout="chw" -- in
        `dtype` (output_table: bfloat16 as uint16 bits), normalised by scale / mean / std.  The containers are read during this call
        only."""
        ptrs, lens, keep = _containers(containers)
        if len(keep) != self.frames_per_job:
            raise LlcompError(BAD_ARGS, f"a job takes {self.frames_per_job} containers, got {len(keep)}")
        tab, _ = _rects_table(rects, self.frames_per_job)
        fl = _flags_table(flags, self.frames_per_job, filter)
        c = self.shape[2]
        fmt, np_t, _keep = _output_format(c, dtype, layout, scale, mean, std)
        if fmt is None:
            rc = self._L.llcomp_mi_stream_submit_decode_resized_regions(self._h, ptrs, lens, tab, fl, ow, oh, tag)
        else:
            rc = self._L.llcomp_mi_stream_submit_decode_resized_regions_ex(self._h, ptrs, lens, tab, fl, ow, oh, C.byref(fmt), tag)
        return self._submit(rc, (c, oh, ow) if fmt is not None and fmt.layout == LAYOUT_CHW else (oh, ow, c), np_t)

    def pending(self):
        return self._L.llcomp_mi_stream_pending(self._h)

    def ready(self):
        return self._L.llcomp_mi_stream_poll(self._h) == OK

    def wait(self):
        r = _lib.StreamResult()
        _check(self._L.llcomp_mi_stream_wait(self._h, C.byref(r)))
        shape, np_t = self._shapes.pop(0)
        data = None
        if r.status == OK:
            whole = np.ctypeslib.as_array(C.cast(r.data, _lib.u8p), shape=(max(int(r.len), 1),))[: int(r.len)]
            if r.kind in (JOB_DECODE, JOB_DECODE_REGIONS, JOB_DECODE_RESIZED_REGIONS):
                whole = whole.view(np_t) if np_t is not np.uint8 else whole
                data = whole.reshape(shape) if self.frames_per_job == 1 else whole.reshape((self.frames_per_job,) + shape)
            elif self.frames_per_job == 1:
                data = whole
            else:
                data = []
                for f in range(self.frames_per_job):
                    p, n = C.c_void_p(), C.c_uint64()
                    _check(self._L.llcomp_mi_stream_result_part(self._h, r.slot, f, C.byref(p), C.byref(n)))
                    data.append(np.ctypeslib.as_array(C.cast(p, _lib.u8p), shape=(max(int(n.value), 1),))[: int(n.value)])
        return StreamJob(r.slot, r.kind, r.status, r.tag, data)

    def release(self, job):
        _check(self._L.llcomp_mi_stream_release(self._h, job.slot))


def _same_bytes(a, b):
    """bit-exact comparison of two uint8 arrays, eight bytes at a time where the layout allows"""
    a, b = a.reshape(-1), b.reshape(-1)
    if a.size != b.size:
        return False
    if a.size % 8 == 0 and a.ctypes.data % 8 == 0 and b.ctypes.data % 8 == 0 and a.flags["C_CONTIGUOUS"] and b.flags["C_CONTIGUOUS"]:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


def pipeline_roundtrip(stream, frames, max_encodes_in_flight=3, on_container=None, verify=True, verify_threads=4, clock_origin=None):
    """Drives BASELINE config 5 through a Stream: every frame host -> GPU -> host (container) -> GPU -> host.  An encode
    result (pinned containers) is handed to submit_decode as it is and released only when that decode has come back;
    submit_* returning False (back-pressure) makes the loop take a finished job first.  frames: list of C-contiguous
    uint8 arrays (pinned for DMA); with frames_per_job > 1 consecutive frames of a job must be adjacent in memory (views
    of one buffer) and len(frames) a multiple of it.  Returns (container lengths, completion time of every frame in
    seconds, number of times back-pressure was hit).  on_container(i, bytes_view) sees every container; verify compares
    every decoded frame with its source bit for bit -- on a few worker threads (numpy releases the GIL), the slot is
    released afterwards.  clock_origin: a time.perf_counter() value the completion times are measured from (several
    pipelines driven from several threads share one; default: this call's start)."""
    import time
    from concurrent.futures import ThreadPoolExecutor

    F = stream.frames_per_job
    n = len(frames)
    assert n % F == 0, "the number of frames must be a multiple of frames_per_job"
    n_jobs = n // F
    raw = frames[0].size
    jobs_px = []
    for j in range(n_jobs):
        if F == 1:
            jobs_px.append(frames[j])
        else:
            base = frames[j * F].ctypes.data
            assert all(frames[j * F + f].ctypes.data == base + f * raw for f in range(F)), "the frames of a job must be adjacent in memory"
            jobs_px.append(np.ctypeslib.as_array(C.cast(base, _lib.u8p), shape=(F * raw,)))
    lens, done_at, busy_seen = [0] * n, [0.0] * n, 0
    enc_held, to_decode, checking = {}, [], []
    next_job = finished = enc_in_flight = 0
    pool = ThreadPoolExecutor(max_workers=verify_threads) if verify and verify_threads > 0 else None

    def reap(block):
        nonlocal finished
        while checking and (block or checking[0][0].done()):
            fut, job = checking.pop(0)
            if not fut.result():
                raise AssertionError(f"job {job.tag} (frames {job.tag * F}..{job.tag * F + F - 1}) is not bit-exact after the round trip")
            stream.release(job)
            finished += 1
            block = False

    t0 = time.perf_counter() if clock_origin is None else clock_origin
    try:
        while finished < n_jobs:
            progressed = False
            reap(False)
            while to_decode:  # containers first: their decode frees two slots
                job = to_decode[0]
                if not stream.submit_decode(job.data, tag=job.tag):
                    busy_seen += 1
                    break
                enc_held[job.tag] = job
                to_decode.pop(0)
                progressed = True
            while next_job < n_jobs and enc_in_flight < max_encodes_in_flight and not to_decode:
                if not stream.submit_encode(jobs_px[next_job], tag=next_job):
                    busy_seen += 1
                    break
                next_job += 1
                enc_in_flight += 1
                progressed = True
            if stream.pending() and (not progressed or stream.ready()):
                job = stream.wait()
                if job.status != OK:
                    raise LlcompError(job.status)
                if job.kind == JOB_ENCODE:
                    enc_in_flight -= 1
                    for f, cont in enumerate([job.data] if F == 1 else job.data):
                        lens[job.tag * F + f] = cont.size
                        if on_container:
                            on_container(job.tag * F + f, cont)
                    to_decode.append(job)
                else:
                    now = time.perf_counter() - t0
                    for f in range(F):
                        done_at[job.tag * F + f] = now
                    stream.release(enc_held.pop(job.tag))
                    if pool:
                        checking.append((pool.submit(_same_bytes, job.data, jobs_px[job.tag]), job))
                    else:
                        if verify and not _same_bytes(job.data, jobs_px[job.tag]):
                            raise AssertionError(f"job {job.tag} is not bit-exact after the round trip")
                        stream.release(job)
                        finished += 1
            elif not progressed:
                reap(True)  # every slot is held by frames that are being compared
    finally:
        if pool:
            pool.shutdown(wait=True)
    return lens, done_at, busy_seen


def probe(data):
    L = _lib.load()
    data = bytes(data)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    info = Info()
    _check(L.llcomp_mi_probe(C.cast(buf, _lib.u8p), len(data), C.byref(info)))
    return info


def fnv1a64(*pieces):
    """FNV-1a-64 over the concatenation of `pieces` (bytes or contiguous numpy uint8 arrays), as a 16-digit hex string --
    the form tests/golden records container hashes in."""
    L = _lib.load()
    h = 0
    for p in pieces:
        a = np.frombuffer(p, dtype=np.uint8) if isinstance(p, (bytes, bytearray, memoryview)) else np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)
        if a.size:
            h = L.llcomp_mi_fnv1a64(a.ctypes.data, a.size, h)
    return "%016x" % (h or 1469598103934665603)


def suggest_tile_w(frames, w, h, c, planar=True):
    """slice width for one-row slices that keeps the GPU busy when `frames` frames are coded per call (llcomp_mi_suggest_tile_w)"""
    return int(_lib.load().llcomp_mi_suggest_tile_w(frames, w, h, c, int(bool(planar))))


def slice_count(w, h, c, tile_w=0, tile_h=0, planar=False):
    return _lib.load().llcomp_mi_slice_count(w, h, c, tile_w, tile_h, int(bool(planar)))


def merge_bands(bands):
    """Concatenate SLICED containers of consecutive horizontal bands (multi-GPU shards) into one container."""
    L = _lib.load()
    n = len(bands)
    keep = [(C.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) or b"\0") for b in bands]
    ptrs = (_lib.u8p * n)(*[C.cast(k, _lib.u8p) for k in keep])
    lens = (C.c_size_t * n)(*[len(b) for b in bands])
    out, m = _lib.u8p(), C.c_size_t()
    _check(L.llcomp_mi_merge_bands(ptrs, lens, n, C.byref(out), C.byref(m)))
    try:
        return C.string_at(out, m.value)
    finally:
        L.llcomp_mi_free(out)


def split_band(data, tile_row0, tile_row1):
    L = _lib.load()
    data = bytes(data)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    out, m = _lib.u8p(), C.c_size_t()
    _check(L.llcomp_mi_split_band(C.cast(buf, _lib.u8p), len(data), tile_row0, tile_row1, C.byref(out), C.byref(m)))
    try:
        return C.string_at(out, m.value)
    finally:
        L.llcomp_mi_free(out)


class Codec:
    """Device-resident batch codec (llcomp_mi_codec_*): `frames` images of one shape per call, buffers stay in HBM.
    Pointers are raw device addresses (e.g. torch tensor .data_ptr()); `stream` is a hipStream_t handle
    (torch.cuda.current_stream().cuda_stream) or 0."""

    def __init__(self, frames, w, h, c, tile_w=0, tile_h=0, planar=False, device=-1, small_model=False):
        self._L = _lib.load()
        self._h = C.c_void_p()
        _check(self._L.llcomp_mi_codec_create_ex(C.byref(self._h), device, frames, w, h, c, tile_w, tile_h, int(bool(planar)), 1 if small_model else 0))
        self.frames, self.w, self.h, self.c = frames, w, h, c
        self.n_slices = self._L.llcomp_mi_codec_slices(self._h)
        self.max_payload_bytes = self._L.llcomp_mi_codec_max_payload_bytes(self._h)
        self.workspace_bytes = self._L.llcomp_mi_codec_workspace_bytes(self._h)
        fam = self._L.llcomp_mi_codec_kernel_family(self._h)  # (diagnostic: tests make sure they run the family they mean to)
        self.family = {"rows": bool(fam & 1), "lds_table": bool(fam & 2), "snapshot": bool(fam & 16), "bank_cache": bool(fam & 32),
                       "lane_shift": (fam >> 8) & 0xFF, "slices_per_wave": (fam >> 16) & 0xFF}

    def close(self):
        if self._h:
            self._L.llcomp_mi_codec_destroy(self._h)
            self._h = None

    __del__ = close

    def encode(self, d_px, d_payload, payload_cap, d_slice_len, d_total, d_status, stream=0):
        _check(self._L.llcomp_mi_codec_encode(self._h, d_px, d_payload, payload_cap, d_slice_len, d_total, d_status, stream))

    def decode(self, d_payload, payload_bytes, d_slice_len, d_px, d_status, stream=0):
        _check(self._L.llcomp_mi_codec_decode(self._h, d_payload, payload_bytes, d_slice_len, d_px, d_status, stream))

    def decode_region(self, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_px, d_status, stream=0):
        """the rectangle (x, y, rw, rh) of every frame -> d_px [frames][rh][rw][c] (llcomp_mi_codec_decode_region); d_payload /
        d_slice_len are the full batch's"""
        _check(self._L.llcomp_mi_codec_decode_region(self._h, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_px, d_status, stream))

    def encode_region(self, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_rect, d_sub_payload, sub_payload_cap, d_sub_len, d_sub_total,
                      d_status, stream=0):
        """the rectangle (x, y, rw, rh) of every frame replaced by d_rect [frames][rh][rw][c]: the covered slices' new streams ->
        d_sub_payload (packed, sub-slice order), d_sub_len u32[covered slices of all frames], d_sub_total (llcomp_mi_codec_encode_region).
        d_payload / d_slice_len are the full batch's; they may be 0 when the rectangle is exactly its box's pixels."""
        _check(self._L.llcomp_mi_codec_encode_region(self._h, d_payload or None, payload_bytes, d_slice_len or None, x, y, rw, rh, d_rect,
                                                     d_sub_payload, sub_payload_cap, d_sub_len, d_sub_total, d_status, stream))

    def update_region(self, d_payload, payload_bytes, d_slice_len, x, y, rw, rh, d_rect, d_payload_out, payload_cap, d_slice_len_out, d_total,
                      d_status, stream=0):
        """... and the splice in HBM: the full batch's new d_payload_out, d_slice_len_out u32[slices] and d_total, as encode would write
        them for the modified frames (llcomp_mi_codec_update_region); the outputs must not overlap the inputs"""
        _check(self._L.llcomp_mi_codec_update_region(self._h, d_payload or None, payload_bytes, d_slice_len or None, x, y, rw, rh, d_rect,
                                                     d_payload_out, payload_cap, d_slice_len_out, d_total, d_status, stream))

    def region_family(self, x, y, rw, rh):
        """the kernel family a region decode of this rectangle runs (the keys of .family), None for a bad rectangle"""
        fam = self._L.llcomp_mi_codec_region_family(self._h, x, y, rw, rh)
        if not fam:
            return None
        return {"rows": bool(fam & 1), "lds_table": bool(fam & 2), "snapshot": bool(fam & 16), "bank_cache": bool(fam & 32),
                "lane_shift": (fam >> 8) & 0xFF, "slices_per_wave": (fam >> 16) & 0xFF}

    def decode_regions(self, d_payload, payload_bytes, d_slice_len, xy, rw, rh, d_px, d_status, stream=0):
        """frame f's rectangle (xy[f][0], xy[f][1], rw, rh) -> d_px [frames][rh][rw][c] (llcomp_mi_codec_decode_regions); xy = a
        sequence of (x, y) pairs or an int / uint32 array of shape [frames, 2], read during the call; d_payload / d_slice_len are the
        full batch's (pack_batch)"""
        tab, _ = _xy_table(xy, self.frames)
        _check(self._L.llcomp_mi_codec_decode_regions(self._h, d_payload, payload_bytes, d_slice_len, tab, rw, rh, d_px, d_status, stream))

    def decode_regions_host(self, containers, xy, rw, rh, d_px, d_status, stream=0):
        """decode_regions of host containers (llcomp_mi_codec_decode_regions_host): `containers` = the frames' single-frame SLICED
        containers (bytes or uint8 arrays), and only their windows' bytes cross PCIe.  The containers and xy are read during the call
        only; the decode is asynchronous on `stream`."""
        ptrs, lens, _keep = _frame_containers(containers, self.frames)
        tab, _ = _xy_table(xy, self.frames)
        _check(self._L.llcomp_mi_codec_decode_regions_host(self._h, ptrs, lens, tab, rw, rh, d_px, d_status, stream))

    # The resized, views and warped calls, each from either source: src = (d_payload, payload_bytes, d_slice_len) of the batch in HBM, or
    # -- host -- (ptrs, lens) of the frames' containers (_frame_containers); the C function by the source and by what the call asks for.
    def _resized(self, host, src, rects, ow, oh, d_px, d_status, flags, stream, dtype, layout, scale, mean, std, filter, pad_mode, fill):
        name = "llcomp_mi_codec_decode_%s_regions" + ("_host" if host else "")
        fl = _flags_table(flags, self.frames, filter)
        fmt, _, _keep = _output_format(self.c, dtype, layout, scale, mean, std)
        if pad_mode is not None or fill is not None:
            tab, _ = _signed_rects_table(rects, self.frames)
            pad, _keep_pad = _pad(self.c, pad_mode, fill)
            _check(getattr(self._L, name % "padded")(self._h, *src, tab, fl, ow, oh, C.byref(pad), C.byref(fmt) if fmt is not None else None, d_px,
                                                    d_status, stream))
            return
        tab, _ = _rects_table(rects, self.frames)
        if fmt is None:
            _check(getattr(self._L, name % "resized")(self._h, *src, tab, fl, ow, oh, d_px, d_status, stream))
        else:
            _check(getattr(self._L, name % "resized" + "_ex")(self._h, *src, tab, fl, ow, oh, C.byref(fmt), d_px, d_status, stream))

    def _views(self, host, src, groups, d_status, stream, pad_mode, fill):
        name = "llcomp_mi_codec_decode_%sviews" + ("_host" if host else "")
        groups = list(groups) if groups is not None else []
        padded = pad_mode is not None or fill is not None
        arr, n, _keep = _view_groups(groups, self.c, signed=padded)
        chains = any(getattr(gr, "photo", None) is not None for gr in groups)
        photo, _keep_photo = _photo_groups(groups, [arr[i].n_views for i in range(n)]) if chains else (None, None)
        pad, _keep_pad = _pad(self.c, pad_mode, fill) if padded else (None, None)
        if chains:
            _check(getattr(self._L, name % "photo_")(self._h, *src, arr, n, C.byref(pad) if padded else None, photo, d_status, stream))
        elif padded:
            _check(getattr(self._L, name % "padded_")(self._h, *src, arr, n, C.byref(pad), d_status, stream))
        else:
            _check(getattr(self._L, name % "")(self._h, *src, arr, n, d_status, stream))

    def _warped(self, host, src, groups, d_status, stream, persp=False):
        name = "llcomp_mi_codec_decode_%s" + ("perspective" if persp else "warped") + "_views" + ("_host" if host else "")
        groups = list(groups) if groups is not None else []
        arr, n, _keep = _warp_groups(groups, self.c, persp)
        if any(getattr(gr, "photo", None) is not None for gr in groups):
            photo, _keep_photo = _photo_groups(groups, [arr[i].n_views for i in range(n)])
            _check(getattr(self._L, name % "photo_")(self._h, *src, arr, n, photo, d_status, stream))
        else:
            _check(getattr(self._L, name % "")(self._h, *src, arr, n, d_status, stream))

    def decode_resized_regions(self, d_payload, payload_bytes, d_slice_len, rects, ow, oh, d_px, d_status, flags=None, stream=0, dtype=None,
                               layout="hwc", scale=False, mean=None, std=None, filter=None, pad_mode=None, fill=None):
        """frame f's rectangle rects[f] = (x, y, rw, rh), resampled to ow x oh (and mirrored where flags[f] & 1) -> d_px
        [frames][oh][ow][c] (llcomp_mi_codec_decode_resized_regions); rects and flags are read during the call.  filter: PIL's
        "bilinear" (the default), "box", "hamming", "bicubic", "lanczos", or "nearest" for label images -- a name or FILTER_* code for
        every frame, or a sequence of one per frame (a batch may mix them); it is OR-ed into bits 4-6 of the flags.  dtype ("float32",
        "float16", "bfloat16", "uint8" or the numpy / torch type), layout ("hwc" or "chw": [frames][c][oh][ow]), scale (divide by 255)
        and mean / std (c values) give the output as a model takes it (llcomp_mi_codec_decode_resized_regions_ex; output_table
        states the rule); d_px must be aligned to the element size.  pad_mode ("constant", "edge", "reflect", "symmetric" or a PAD_* code)
        and fill (one value or c values, "constant" only; alone it means "constant"): rectangles may leave the image, x and y may be
        negative, and frame f is np.pad(frame, pad_mode) cut at its rectangle (llcomp_mi_codec_decode_padded_regions) -- only the part
        inside the image is decoded.  Without them a rectangle outside the image stays BAD_ARGS."""
        self._resized(False, (d_payload, payload_bytes, d_slice_len), rects, ow, oh, d_px, d_status, flags, stream, dtype, layout, scale, mean, std,
                      filter, pad_mode, fill)

    def decode_resized_regions_host(self, containers, rects, ow, oh, d_px, d_status, flags=None, stream=0, dtype=None, layout="hwc", scale=False,
                                    mean=None, std=None, filter=None, pad_mode=None, fill=None):
        """decode_resized_regions of host containers (llcomp_mi_codec_decode_resized_regions_host(_ex)): only the windows' bytes cross
        PCIe; the containers, rects and flags are read during the call only; filter, pad_mode and fill as decode_resized_regions takes
        them (llcomp_mi_codec_decode_padded_regions_host: only the windows of the source rectangles cross)"""
        ptrs, lens, _keep = _frame_containers(containers, self.frames)
        self._resized(True, (ptrs, lens), rects, ow, oh, d_px, d_status, flags, stream, dtype, layout, scale, mean, std, filter, pad_mode, fill)

    def decode_views(self, d_payload, payload_bytes, d_slice_len, groups, d_status, stream=0, pad_mode=None, fill=None):
        """several views of each frame, each frame decoded once (llcomp_mi_codec_decode_views): groups = ViewGroup objects (or
        (views, ow, oh, d_out) tuples); view v of a group -> d_out[v], byte for byte what decode_resized_regions writes for that rectangle
        of that frame.  A frame decodes the bounding box of all its views; a frame without a view is not read.  d_payload / d_slice_len
        are the full batch's (pack_batch).  pad_mode / fill as decode_resized_regions takes them: views may leave the image, a view's x and
        y may be negative (llcomp_mi_codec_decode_padded_views), and a frame decodes the bounding box of its views' source rectangles."""
        self._views(False, (d_payload, payload_bytes, d_slice_len), groups, d_status, stream, pad_mode, fill)

    def decode_views_host(self, containers, groups, d_status, stream=0, pad_mode=None, fill=None):
        """decode_views of host containers (llcomp_mi_codec_decode_views_host): only the union windows' bytes cross PCIe; the container
        of a frame without a view may be None and is never read; pad_mode / fill as decode_views takes them
        (llcomp_mi_codec_decode_padded_views_host)"""
        ptrs, lens, _keep = _frame_containers(containers, self.frames, allow_none=True)
        self._views(True, (ptrs, lens), groups, d_status, stream, pad_mode, fill)

    def decode_warped_views(self, d_payload, payload_bytes, d_slice_len, groups, d_status, stream=0):
        """views under an affine map (llcomp_mi_codec_decode_warped_views): groups = WarpGroup objects; view v of a group -> d_out[v], byte
        for byte warp_reference of its frame (PIL's Image.transform(AFFINE)), mirrored and formatted as the other calls do.  A frame
        decodes once, and only the bounding box of the source pixels its views read; a frame without a view is not read."""
        self._warped(False, (d_payload, payload_bytes, d_slice_len), groups, d_status, stream)

    def decode_warped_views_host(self, containers, groups, d_status, stream=0):
        """decode_warped_views of host containers (llcomp_mi_codec_decode_warped_views_host): only the union windows' bytes cross PCIe;
        the container of a frame no view reads may be None and is never read"""
        ptrs, lens, _keep = _frame_containers(containers, self.frames, allow_none=True)
        self._warped(True, (ptrs, lens), groups, d_status, stream)

    def decode_perspective_views(self, d_payload, payload_bytes, d_slice_len, groups, d_status, stream=0):
        """views under a projective map (llcomp_mi_codec_decode_perspective_views): groups = PerspectiveGroup objects; view v of a group
        -> d_out[v], byte for byte perspective_reference of its frame (PIL's Image.transform(PERSPECTIVE)), mirrored and formatted as the
        other calls do.  A frame decodes once, and only a bounding box of the source pixels its views read; a frame without a view is
        not read.  A group with photo= runs its chains behind the gather (llcomp_mi_codec_decode_photo_perspective_views)."""
        self._warped(False, (d_payload, payload_bytes, d_slice_len), groups, d_status, stream, persp=True)

    def decode_perspective_views_host(self, containers, groups, d_status, stream=0):
        """decode_perspective_views of host containers (llcomp_mi_codec_decode_perspective_views_host): only the union windows' bytes
        cross PCIe; the container of a frame no view reads may be None and is never read"""
        ptrs, lens, _keep = _frame_containers(containers, self.frames, allow_none=True)
        self._warped(True, (ptrs, lens), groups, d_status, stream, persp=True)

    def perspective_workspace_bytes(self, total_views, photo=False):
        """the bound on .allocated_bytes() for perspective views calls of up to total_views views with outputs no larger than the image
        (llcomp_mi_codec_perspective_workspace_bytes); photo: for calls with photometric chains
        (llcomp_mi_codec_photo_perspective_workspace_bytes)"""
        if photo:
            return self._L.llcomp_mi_codec_photo_perspective_workspace_bytes(self._h, int(total_views))
        return self._L.llcomp_mi_codec_perspective_workspace_bytes(self._h, int(total_views))

    def warp_workspace_bytes(self, total_views):
        """the bound on .allocated_bytes() for warped views calls of up to total_views views with outputs no larger than the image
        (llcomp_mi_codec_warp_workspace_bytes)"""
        return self._L.llcomp_mi_codec_warp_workspace_bytes(self._h, int(total_views))

    def photo_workspace_bytes(self, total_views):
        """the bound on .allocated_bytes() for views and warped views calls with photometric chains (a group with photo=) of up to
        total_views views with outputs no larger than the image (llcomp_mi_codec_photo_workspace_bytes)"""
        return self._L.llcomp_mi_codec_photo_workspace_bytes(self._h, int(total_views))

    def mix_batch(self, d_batch, n, ow, oh, samples, dtype="float32", layout="chw", erase_value=None, stream=0):
        """RandomErasing, MixUp and CutMix in place on a dense batch in device memory (llcomp_mi_codec_mix_batch): n samples of the
        codec's channels and ow x oh pixels in the dtype and layout a decode call wrote them in; samples from mix_samples(); erase_value:
        one value or one per channel (default zeros).  Asynchronous on `stream`; samples and erase_value are read during the call."""
        ev = _per_channel(erase_value, self.c, "erase_value")
        _check(self._L.llcomp_mi_codec_mix_batch(self._h, d_batch, int(n), int(ow), int(oh), _dtype_code(dtype), _layout_code(layout),
                                                 _mix_records(samples, n), ev, stream))

    def mix_workspace_bytes(self, n, ow, oh, dtype="float32"):
        """the bound on .allocated_bytes() with mix_batch calls of up to n samples of ow x oh (llcomp_mi_codec_mix_workspace_bytes)"""
        return self._L.llcomp_mi_codec_mix_workspace_bytes(self._h, int(n), int(ow), int(oh), _dtype_code(dtype))

    def orient_batch(self, d_batch, n, ow, oh, codes, dtype="float32", layout="chw", stream=0):
        """A flip, quarter turn or transposition per sample, in place on a dense batch in device memory (llcomp_mi_codec_orient_batch):
        n samples of the codec's channels and ow x oh pixels in the dtype and layout a decode call wrote them in; codes: n orientations
        (orient_code: ORIENT_*, PIL's names or None) or one for every sample.  The transposing codes take ow == oh.  It goes behind
        the decode and ahead of mix_batch on the same stream."""
        n = int(n)
        if n <= 0:
            raise LlcompError(BAD_ARGS, f"n must be positive, got {n}")
        _check(self._L.llcomp_mi_codec_orient_batch(self._h, d_batch, n, int(ow), int(oh), _dtype_code(dtype), _layout_code(layout),
                                                    _orient_codes(codes, n), stream))

    def orient_workspace_bytes(self, n):
        """the bound on .allocated_bytes() with orient_batch calls of up to n samples (llcomp_mi_codec_orient_workspace_bytes)"""
        return self._L.llcomp_mi_codec_orient_workspace_bytes(self._h, int(n))

    def compose_batch(self, d_src, n_src, iw, ih, d_dst, n_dst, ow, oh, pieces, dtype="float32", layout="chw", fill=None, keep=False, stream=0):
        """Rectangles of one dense batch into another, the rest a fill or kept (llcomp_mi_codec_compose_batch): d_src, n_src samples of
        the codec's channels and iw x ih pixels (None and 0 when every piece is a FILL piece), d_dst, n_dst samples of ow x oh, both in
        device memory in the same dtype and layout; pieces from compose_pieces(), grid_pieces() or mosaic_pieces(), or records for
        compose_pieces(); fill: one value or one per channel (default zeros); keep: what no piece covers stays and is not written.
        Asynchronous on `stream`, behind the decode that wrote d_src; pieces and fill are read during the call."""
        recs = compose_pieces(pieces)
        _check(self._L.llcomp_mi_codec_compose_batch(self._h, d_src, int(n_src), int(iw), int(ih), d_dst, int(n_dst), int(ow), int(oh),
                                                     _dtype_code(dtype), _layout_code(layout), recs, len(recs), _per_channel(fill, self.c, "fill"),
                                                     COMPOSE_KEEP if keep else 0, stream))

    def compose_workspace_bytes(self, n_dst, n_pieces):
        """the bound on .allocated_bytes() with compose_batch calls of up to n_dst dst samples and n_pieces pieces
        (llcomp_mi_codec_compose_workspace_bytes)"""
        return self._L.llcomp_mi_codec_compose_workspace_bytes(self._h, int(n_dst), int(n_pieces))

    def paste_batch(self, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, pieces, dtype="float32", layout="chw", stream=0):
        """The pieces of one dense batch that an id map selects, into another, in place (llcomp_mi_codec_paste_batch): d_src, n_src
        samples of iw x ih, d_mask, their id maps (n_src x ih x iw bytes at any address; it may be d_src for c = 1 uint8), and d_dst,
        n_dst samples of ow x oh, in device memory; src and dst of the codec's channels in the same dtype and layout; pieces from
        paste_pieces(), or records for it.  What no piece selects stays and is not written.  Asynchronous on `stream`."""
        recs = paste_pieces(pieces)
        _check(self._L.llcomp_mi_codec_paste_batch(self._h, d_src, d_mask, int(n_src), int(iw), int(ih), d_dst, int(n_dst), int(ow), int(oh),
                                                   _dtype_code(dtype), _layout_code(layout), recs, len(recs), stream))

    def paste_workspace_bytes(self, n_dst, n_pieces):
        """the bound on .allocated_bytes() with paste_batch calls of up to n_dst dst samples and n_pieces pieces
        (llcomp_mi_codec_paste_workspace_bytes)"""
        return self._L.llcomp_mi_codec_paste_workspace_bytes(self._h, int(n_dst), int(n_pieces))

    def paste_batch16(self, d_src, d_mask, n_src, iw, ih, d_dst, n_dst, ow, oh, pieces, dtype="float32", layout="chw", stream=0):
        """paste_batch selected by 16-bit id maps (llcomp_mi_codec_paste_batch16): d_mask, n_src x ih x iw uint16 aligned to 2 bytes (it
        may be d_src for uint8 "hwc" with c = 2, or a 2-byte dtype with c = 1); pieces from paste_pieces16(), or records for it.  What no
        piece selects stays and is not written.  Asynchronous on `stream`."""
        recs = paste_pieces16(pieces)
        _check(self._L.llcomp_mi_codec_paste_batch16(self._h, d_src, d_mask, int(n_src), int(iw), int(ih), d_dst, int(n_dst), int(ow), int(oh),
                                                     _dtype_code(dtype), _layout_code(layout), recs, len(recs), stream))

    def paste_batch32(self, d_src, d_mask, map_bytes, n_src, iw, ih, d_dst, n_dst, ow, oh, pieces, dtype="float32", layout="chw", stream=0):
        """paste_batch selected by id maps of map_bytes 3 (any address) or 4 (aligned to 4 bytes) per pixel
        (llcomp_mi_codec_paste_batch32): d_mask may be d_src for uint8 "hwc" with c = map_bytes, or float32 with c = 1 for map_bytes 4;
        pieces from paste_pieces32(), or records for it.  What no piece selects stays and is not written.  Asynchronous on `stream`."""
        recs = paste_pieces32(pieces, map_bytes)
        _check(self._L.llcomp_mi_codec_paste_batch32(self._h, d_src, d_mask, int(map_bytes), int(n_src), int(iw), int(ih), d_dst, int(n_dst), int(ow),
                                                     int(oh), _dtype_code(dtype), _layout_code(layout), recs, len(recs), stream))

    def paste32_workspace_bytes(self, n_dst, n_pieces):
        """the bound on .allocated_bytes() with paste_batch32 calls of up to n_dst dst samples and n_pieces pieces
        (llcomp_mi_codec_paste32_workspace_bytes)"""
        return self._L.llcomp_mi_codec_paste32_workspace_bytes(self._h, int(n_dst), int(n_pieces))

    def alpha_paste_batch(self, d_src, d_alpha, alpha_px_bytes, alpha_byte, n_src, iw, ih, d_dst, n_dst, ow, oh, pieces, dtype="float32", layout="chw",
                          stream=0):
        """Pieces of one dense batch blended into another under a per-pixel alpha byte, in place (llcomp_mi_codec_alpha_paste_batch):
        PIL's paste with a mask, Image.composite and, with ALPHA_OVER pieces, Image.alpha_composite.  d_src, n_src samples of iw x ih
        (None when every piece is a VALUE piece); d_alpha, n_src x ih x iw pixels of alpha_px_bytes (1..4) bytes at any address, a
        pixel's alpha its byte alpha_byte (it may be d_src for uint8 "hwc" with c = alpha_px_bytes; None when every piece is OVER);
        d_dst, n_dst samples of ow x oh; src and dst of the codec's channels in the same dtype and layout; pieces from alpha_pieces(),
        or records for it, applied in order.  Asynchronous on `stream`."""
        recs = alpha_pieces(pieces)
        _check(self._L.llcomp_mi_codec_alpha_paste_batch(self._h, d_src, d_alpha, int(alpha_px_bytes), int(alpha_byte), int(n_src), int(iw), int(ih),
                                                         d_dst, int(n_dst), int(ow), int(oh), _dtype_code(dtype), _layout_code(layout), recs, len(recs),
                                                         stream))

    def alpha_paste_workspace_bytes(self, n_dst, n_pieces):
        """the bound on .allocated_bytes() with alpha_paste_batch calls of up to n_dst dst samples and n_pieces pieces
        (llcomp_mi_codec_alpha_paste_workspace_bytes)"""
        return self._L.llcomp_mi_codec_alpha_paste_workspace_bytes(self._h, int(n_dst), int(n_pieces))

    def paste16_workspace_bytes(self, n_dst, n_pieces):
        """the bound on .allocated_bytes() with paste_batch16 calls of up to n_dst dst samples and n_pieces pieces
        (llcomp_mi_codec_paste16_workspace_bytes)"""
        return self._L.llcomp_mi_codec_paste16_workspace_bytes(self._h, int(n_dst), int(n_pieces))

    def label_boxes(self, d_maps, n, ow, oh, d_boxes, stream=0):
        """The pixel count and bounding box of each of the 256 ids of n id maps (llcomp_mi_codec_label_boxes): d_maps, n x oh x ow bytes
        at any address, -> d_boxes, n * 256 records of LABEL_BOX_DTYPE (20 bytes each, 4-byte aligned), both in device memory; every
        record is written.  Asynchronous on `stream`."""
        _check(self._L.llcomp_mi_codec_label_boxes(self._h, d_maps, int(n), int(ow), int(oh), d_boxes, stream))

    def label_boxes16(self, d_maps, n, ow, oh, ids, d_boxes, stream=0):
        """The pixel count and bounding box of the ids listed for each of n 16-bit id maps (llcomp_mi_codec_label_boxes16): d_maps,
        n x oh x ow uint16 aligned to 2 bytes; ids, a sequence of n sequences of ids, each strictly ascending and of at most
        label_boxes16_max_ids() ids -> d_boxes, one record of LABEL_BOX_DTYPE per listed id in the lists' order (4-byte aligned), both in
        device memory; every record is written.  Asynchronous on `stream`; ids is read during the call."""
        flat, first = _label_lists(ids, int(n))
        _check(self._L.llcomp_mi_codec_label_boxes16(self._h, d_maps, int(n), int(ow), int(oh), flat.ctypes.data, first.ctypes.data, d_boxes, stream))

    def label_boxes16_workspace_bytes(self, n, total_ids):
        """the bound on .allocated_bytes() with label_boxes16 calls of up to n samples and total_ids listed ids
        (llcomp_mi_codec_label_boxes16_workspace_bytes)"""
        return self._L.llcomp_mi_codec_label_boxes16_workspace_bytes(self._h, int(n), int(total_ids))

    def label_targets(self, d_maps, n, ow, oh, ids, values, d_out, map_dtype="uint8", kind="index", dtype=None, default=0, planes=None, on=None, off=None,
                      stream=0):
        """What a loss takes from n id maps (llcomp_mi_codec_label_targets): d_maps, n x oh x ow pixels of map_dtype "uint8" (any
        address) or "uint16" (aligned to 2 bytes); ids, values, kind, dtype, default, planes, on and off as label_targets_reference ->
        d_out, the index tensor [n, oh, ow] or the planes, dense and aligned to its element, both in device memory and not overlapping;
        every element is written once.  planes= is an int for one-hot [n, K, oh, ow], or one count per sample.  Asynchronous on
        `stream`; the lists are read during the call."""
        name = str(map_dtype).replace("torch.", "")
        if name not in ("uint8", "uint16"):
            raise LlcompError(BAD_ARGS, f"map_dtype must be uint8 or uint16, got {map_dtype!r}")
        t, keep, _, _ = _label_targets(ids, values, int(n), 1 if name == "uint8" else 2, kind, dtype, default, planes, on, off)
        _check(self._L.llcomp_mi_codec_label_targets(self._h, d_maps, int(n), int(ow), int(oh), C.byref(t), d_out, stream))

    def label_boxes32(self, d_maps, map_bytes, n, ow, oh, ids, d_boxes, stream=0):
        """label_boxes16 for id maps of map_bytes 3 (any address) or 4 (aligned to 4 bytes) per pixel (llcomp_mi_codec_label_boxes32):
        ids a sequence of n strictly ascending sequences of ids up to 0xFFFFFF or 0xFFFFFFFF -> d_boxes, one record of LABEL_BOX_DTYPE
        per listed id in the lists' order.  Asynchronous on `stream`; the maps are only read."""
        flat, first = _label_lists(ids, int(n), np.uint32)
        _check(self._L.llcomp_mi_codec_label_boxes32(self._h, d_maps, int(map_bytes), int(n), int(ow), int(oh), flat.ctypes.data, first.ctypes.data, d_boxes, stream))

    def label_boxes32_workspace_bytes(self, n, total_ids):
        """the bound on .allocated_bytes() with label_boxes32 calls of up to n samples and total_ids listed ids
        (llcomp_mi_codec_label_boxes32_workspace_bytes)"""
        return self._L.llcomp_mi_codec_label_boxes32_workspace_bytes(self._h, int(n), int(total_ids))

    def label_targets32(self, d_maps, map_bytes, n, ow, oh, ids, values, d_out, kind="index", dtype=None, default=0, planes=None, on=None, off=None, stream=0):
        """label_targets for id maps of map_bytes 3 (any address) or 4 (aligned to 4 bytes) per pixel (llcomp_mi_codec_label_targets32);
        ids, values, kind, dtype, default, planes, on and off as label_targets_reference -> d_out.  Asynchronous on `stream`."""
        if int(map_bytes) not in (3, 4):
            raise LlcompError(BAD_ARGS, f"map_bytes of a wide id map is 3 or 4, got {map_bytes!r}")
        t, keep, _, _ = _label_targets(ids, values, int(n), int(map_bytes), kind, dtype, default, planes, on, off)
        _check(self._L.llcomp_mi_codec_label_targets32(self._h, d_maps, int(n), int(ow), int(oh), C.byref(t), d_out, stream))

    def label_targets32_workspace_bytes(self, n, total_ids):
        """the bound on .allocated_bytes() with label_targets32 calls of up to n samples and total_ids listed ids
        (llcomp_mi_codec_label_targets32_workspace_bytes)"""
        return self._L.llcomp_mi_codec_label_targets32_workspace_bytes(self._h, int(n), int(total_ids))

    def label_targets_workspace_bytes(self, n, total_ids):
        """the bound on .allocated_bytes() with label_targets calls of up to n samples and total_ids listed ids
        (llcomp_mi_codec_label_targets_workspace_bytes)"""
        return self._L.llcomp_mi_codec_label_targets_workspace_bytes(self._h, int(n), int(total_ids))

    def views_workspace_bytes(self, total_views):
        """.workspace_bytes for calls of up to total_views views (llcomp_mi_codec_views_workspace_bytes): the staged tables grow with them"""
        return self._L.llcomp_mi_codec_views_workspace_bytes(self._h, int(total_views))

    def padded_workspace_bytes(self, total_views=None):
        """the bound on .allocated_bytes() for padded calls of up to total_views views (default: one per frame, a padded resized call) with
        outputs no larger than the image (llcomp_mi_codec_padded_workspace_bytes): their staged tables are larger than the unpadded calls'"""
        return self._L.llcomp_mi_codec_padded_workspace_bytes(self._h, int(self.frames if total_views is None else total_views))

    def allocated_bytes(self):
        """device bytes the codec holds right now (llcomp_mi_codec_allocated_bytes; at most .workspace_bytes for outputs up to the image's
        size)"""
        return self._L.llcomp_mi_codec_allocated_bytes(self._h)

    def regions_family(self, xy, rw, rh):
        """the kernel family of every class a regions decode of these rectangles runs, in class order (the keys of .family); None
        for bad rectangles"""
        tab, _ = _xy_table(xy, self.frames)
        fam = (C.c_uint32 * 4)()
        n = self._L.llcomp_mi_codec_regions_family(self._h, tab, rw, rh, fam, 4)
        if not n:
            return None
        return [{"rows": bool(f & 1), "lds_table": bool(f & 2), "snapshot": bool(f & 16), "bank_cache": bool(f & 32),
                 "lane_shift": (f >> 8) & 0xFF, "slices_per_wave": (f >> 16) & 0xFF} for f in list(fam)[:n]]

    def model(self, d_px, d_sym, stream=0):
        _check(self._L.llcomp_mi_codec_model(self._h, d_px, d_sym, stream))

    PROFILE_SLOTS = ("clear_states_enc", "k_model_fwd", "k_encode_slices", "scan+pack", "k_scan_lengths_dec", "k_decode_slices", "k_model_inv", "clear_states_dec")

    def set_profiling(self, on=True):
        _check(self._L.llcomp_mi_codec_set_profiling(self._h, int(on)))

    def get_profile(self):
        """-> ({slot: total ms since last call}, n_encode, n_decode); drains the stream."""
        ms = (C.c_double * 8)()
        ne, nd = C.c_uint32(), C.c_uint32()
        _check(self._L.llcomp_mi_codec_get_profile(self._h, ms, C.byref(ne), C.byref(nd)))
        return dict(zip(self.PROFILE_SLOTS, list(ms))), ne.value, nd.value

    def prepare(self, encode=True, decode=True, region=False, regions=False, resized=False, update=False, views=False):
        """allocate now what the first encode / decode / region decode / regions decode / resized regions decode / region update / views
        decode would allocate inside the call (llcomp_mi_codec_prepare)"""
        _check(self._L.llcomp_mi_codec_prepare(self._h, (1 if encode else 0) | (2 if decode else 0) | (8 if region else 0) | (16 if regions else 0)
                                               | (32 if resized else 0) | (64 if update else 0) | (128 if views else 0)))

    COUNTERS = ("dec_cached_waves", "dec_bypassed_waves", "cache_lookups", "cache_misses", "cache_writebacks", "dec_replays", "enc_carry_backs",
                "generation_wraps", "dec_launches_cached", "dec_launches_plain", "host_staged_bytes", "bias_launches")

    def counters(self, reset=False):
        """{name: count} -- what the rare and adaptive paths of this codec's kernels did so far (llcomp_mi_codec_get_counters);
        waits for the codec's last call"""
        v = (C.c_uint64 * 16)()
        _check(self._L.llcomp_mi_codec_get_counters(self._h, v, 16, int(bool(reset))))
        return dict(zip(self.COUNTERS, list(v)))

    def status(self, bits):
        return self._L.llcomp_mi_status_from_bits(int(bits))
