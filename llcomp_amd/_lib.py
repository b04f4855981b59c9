"""ctypes loader for the product library libllcomp_mi.so (HIP kernels + C ABI, include/llcomp_mi.h).

There is deliberately no fallback: if the library is missing this raises, and if there is no HIP device the
library's calls return LLCOMP_MI_NO_DEVICE -- nothing in this package can code a single byte on the CPU."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LLCOMP_MI_LIB: load another build of the same sources instead (tools/clock_probe.py loads the diagnostic library with
# in-kernel clock stamps, csrc/Makefile `probe`); the tests, bench.py and smoke() never set it
LIB_PATH = os.environ.get("LLCOMP_MI_LIB") or os.path.join(_HERE, "libllcomp_mi.so")

ABI_VERSION = 4  # LLCOMP_MI_ABI_VERSION of the header this binding mirrors

# every symbol include/llcomp_mi.h declares (tests/test_abi.py checks the header against this list and the .so)
SYMBOLS = [
    "llcomp_mi_encode", "llcomp_mi_decode", "llcomp_mi_free", "llcomp_mi_strerror", "llcomp_mi_abi_version",
    "llcomp_mi_device_count", "llcomp_mi_probe", "llcomp_mi_slice_count", "llcomp_mi_merge_bands",
    "llcomp_mi_split_band", "llcomp_mi_codec_create", "llcomp_mi_codec_destroy", "llcomp_mi_codec_slices", "llcomp_mi_codec_kernel_family",
    "llcomp_mi_codec_workspace_bytes", "llcomp_mi_codec_max_payload_bytes", "llcomp_mi_codec_encode",
    "llcomp_mi_codec_decode", "llcomp_mi_codec_model", "llcomp_mi_status_from_bits",
    "llcomp_mi_codec_set_profiling", "llcomp_mi_codec_get_profile",
    "llcomp_mi_encode_into", "llcomp_mi_decode_into", "llcomp_mi_host_alloc", "llcomp_mi_host_free",
    "llcomp_mi_reload_tuning", "llcomp_mi_trim", "llcomp_mi_device_copy_segments", "llcomp_mi_decode_flags", "llcomp_mi_codec_create_ex",
    "llcomp_mi_stream_create", "llcomp_mi_stream_create_ex", "llcomp_mi_stream_frames_per_job", "llcomp_mi_stream_submit_decode_batch",
    "llcomp_mi_stream_result_part", "llcomp_mi_stream_destroy", "llcomp_mi_stream_container_capacity",
    "llcomp_mi_stream_submit_encode", "llcomp_mi_stream_submit_decode", "llcomp_mi_stream_pending",
    "llcomp_mi_stream_poll", "llcomp_mi_stream_wait", "llcomp_mi_stream_release",
    "llcomp_mi_set_pool_limit", "llcomp_mi_pool_limit", "llcomp_mi_pool_idle_bytes", "llcomp_mi_fnv1a64", "llcomp_mi_suggest_tile_w", "llcomp_mi_decode_into_flags", "llcomp_mi_device_range_sums",
    "llcomp_mi_decode_devices", "llcomp_mi_decode_into_devices", "llcomp_mi_last_device_error", "llcomp_mi_plan_chunks",
    "llcomp_mi_stream_create_multi", "llcomp_mi_stream_devices", "llcomp_mi_codec_get_counters", "llcomp_mi_codec_prepare",
    "llcomp_mi_region_plan", "llcomp_mi_decode_region", "llcomp_mi_decode_region_into", "llcomp_mi_codec_decode_region",
    "llcomp_mi_codec_region_family", "llcomp_mi_regions_plan", "llcomp_mi_codec_decode_regions", "llcomp_mi_codec_regions_family",
    "llcomp_mi_regions_gather", "llcomp_mi_codec_decode_regions_host", "llcomp_mi_stream_submit_decode_regions",
    "llcomp_mi_resize_weights", "llcomp_mi_resized_regions_plan", "llcomp_mi_codec_decode_resized_regions",
    "llcomp_mi_codec_decode_resized_regions_host", "llcomp_mi_stream_submit_decode_resized_regions", "llcomp_mi_codec_allocated_bytes",
    "llcomp_mi_output_table", "llcomp_mi_codec_decode_resized_regions_ex", "llcomp_mi_codec_decode_resized_regions_host_ex",
    "llcomp_mi_stream_submit_decode_resized_regions_ex",
    "llcomp_mi_replace_slices", "llcomp_mi_replace_slices_into", "llcomp_mi_update_region", "llcomp_mi_update_region_into",
    "llcomp_mi_codec_encode_region", "llcomp_mi_codec_update_region", "llcomp_mi_resize_filter_weights",
    "llcomp_mi_views_plan", "llcomp_mi_codec_decode_views", "llcomp_mi_codec_decode_views_host", "llcomp_mi_codec_views_workspace_bytes",
    "llcomp_mi_pad_axis", "llcomp_mi_padded_filter_weights", "llcomp_mi_padded_regions_plan", "llcomp_mi_codec_decode_padded_regions",
    "llcomp_mi_codec_decode_padded_regions_host", "llcomp_mi_codec_decode_padded_views", "llcomp_mi_codec_decode_padded_views_host",
    "llcomp_mi_codec_padded_workspace_bytes",
    "llcomp_mi_warp_source_rect", "llcomp_mi_warp_views_plan", "llcomp_mi_warp_reference", "llcomp_mi_codec_decode_warped_views",
    "llcomp_mi_codec_decode_warped_views_host", "llcomp_mi_codec_warp_workspace_bytes",
    "llcomp_mi_photo_reference", "llcomp_mi_codec_decode_photo_views", "llcomp_mi_codec_decode_photo_views_host",
    "llcomp_mi_codec_decode_photo_warped_views", "llcomp_mi_codec_decode_photo_warped_views_host", "llcomp_mi_codec_photo_workspace_bytes",
    "llcomp_mi_perspective_source_rect", "llcomp_mi_perspective_views_plan", "llcomp_mi_perspective_reference",
    "llcomp_mi_codec_decode_perspective_views", "llcomp_mi_codec_decode_perspective_views_host",
    "llcomp_mi_codec_decode_photo_perspective_views", "llcomp_mi_codec_decode_photo_perspective_views_host",
    "llcomp_mi_codec_perspective_workspace_bytes", "llcomp_mi_codec_photo_perspective_workspace_bytes",
    "llcomp_mi_mix_plan", "llcomp_mi_mix_segment", "llcomp_mi_mix_reference", "llcomp_mi_codec_mix_batch",
    "llcomp_mi_codec_mix_workspace_bytes",
    "llcomp_mi_orient_reference", "llcomp_mi_orient_tile", "llcomp_mi_codec_orient_batch", "llcomp_mi_codec_orient_workspace_bytes",
    "llcomp_mi_compose_reference", "llcomp_mi_compose_plan", "llcomp_mi_compose_tile", "llcomp_mi_compose_tile_rows",
    "llcomp_mi_compose_max_pieces_per_sample", "llcomp_mi_codec_compose_batch", "llcomp_mi_codec_compose_workspace_bytes",
    "llcomp_mi_paste_reference", "llcomp_mi_paste_plan", "llcomp_mi_paste_max_pieces_per_sample", "llcomp_mi_codec_paste_batch",
    "llcomp_mi_codec_paste_workspace_bytes",
    "llcomp_mi_label_boxes_reference", "llcomp_mi_label_boxes_rows", "llcomp_mi_codec_label_boxes",
    "llcomp_mi_paste16_reference", "llcomp_mi_paste16_plan", "llcomp_mi_codec_paste_batch16", "llcomp_mi_codec_paste16_workspace_bytes",
    "llcomp_mi_label_boxes16_reference", "llcomp_mi_label_boxes16_max_ids", "llcomp_mi_codec_label_boxes16",
    "llcomp_mi_codec_label_boxes16_workspace_bytes",
    "llcomp_mi_label_targets_reference", "llcomp_mi_label_targets_out_bytes", "llcomp_mi_label_targets_segment",
    "llcomp_mi_label_targets_max_planes", "llcomp_mi_codec_label_targets", "llcomp_mi_codec_label_targets_workspace_bytes",
    "llcomp_mi_label_boxes32_reference", "llcomp_mi_codec_label_boxes32", "llcomp_mi_codec_label_boxes32_workspace_bytes",
    "llcomp_mi_label_targets32_reference", "llcomp_mi_label_targets32_out_bytes", "llcomp_mi_codec_label_targets32",
    "llcomp_mi_codec_label_targets32_workspace_bytes",
    "llcomp_mi_paste32_reference", "llcomp_mi_paste32_plan", "llcomp_mi_codec_paste_batch32", "llcomp_mi_codec_paste32_workspace_bytes",
    "llcomp_mi_alpha_paste_reference", "llcomp_mi_alpha_paste_plan", "llcomp_mi_codec_alpha_paste_batch",
    "llcomp_mi_codec_alpha_paste_workspace_bytes",
]

u8p = C.POINTER(C.c_uint8)


class Opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("planar", C.c_uint32), ("device", C.c_int32), ("small_model", C.c_uint32),
                ("n_devices", C.c_uint32), ("devices", C.POINTER(C.c_int32)), ("chunks_per_device", C.c_uint32), ("reserved", C.c_uint32)]


class OutputFormat(C.Structure):
    """llcomp_mi_output_format (include/llcomp_mi.h): 32 bytes, mean at 16, std at 24"""
    _fields_ = [("struct_size", C.c_uint32), ("dtype", C.c_uint32), ("layout", C.c_uint32), ("scale", C.c_uint32),
                ("mean", C.POINTER(C.c_float)), ("std", C.POINTER(C.c_float))]


class View(C.Structure):
    """llcomp_mi_view (include/llcomp_mi.h): 24 bytes"""
    _fields_ = [("frame", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("rw", C.c_uint32), ("rh", C.c_uint32), ("flags", C.c_uint32)]


class ViewGroup(C.Structure):
    """llcomp_mi_view_group (include/llcomp_mi.h): 40 bytes, views at 8, fmt at 24, d_out at 32"""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", C.c_uint32), ("views", C.POINTER(View)), ("ow", C.c_uint32), ("oh", C.c_uint32),
                ("fmt", C.POINTER(OutputFormat)), ("d_out", C.c_void_p)]


class Pad(C.Structure):
    """llcomp_mi_pad (include/llcomp_mi.h): 16 bytes, fill at 8"""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("fill", u8p)]


class WarpView(C.Structure):
    """llcomp_mi_warp_view (include/llcomp_mi.h): 56 bytes, m at 8"""
    _fields_ = [("frame", C.c_uint32), ("flags", C.c_uint32), ("m", C.c_double * 6)]


class WarpGroup(C.Structure):
    """llcomp_mi_warp_group (include/llcomp_mi.h): 48 bytes, views at 8, fmt at 24, d_out at 32, fill at 40"""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", C.c_uint32), ("views", C.POINTER(WarpView)), ("ow", C.c_uint32), ("oh", C.c_uint32),
                ("fmt", C.POINTER(OutputFormat)), ("d_out", C.c_void_p), ("fill", u8p)]


class PerspectiveView(C.Structure):
    """llcomp_mi_perspective_view (include/llcomp_mi.h): 72 bytes, a at 8"""
    _fields_ = [("frame", C.c_uint32), ("flags", C.c_uint32), ("a", C.c_double * 8)]


class PerspectiveGroup(C.Structure):
    """llcomp_mi_perspective_group (include/llcomp_mi.h): 48 bytes, llcomp_mi_warp_group's fields around the perspective view"""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", C.c_uint32), ("views", C.POINTER(PerspectiveView)), ("ow", C.c_uint32),
                ("oh", C.c_uint32), ("fmt", C.POINTER(OutputFormat)), ("d_out", C.c_void_p), ("fill", u8p)]


PHOTO_MAX_OPS = 8


class PhotoOp(C.Structure):
    """llcomp_mi_photo_op (include/llcomp_mi.h): 8 bytes"""
    _fields_ = [("op", C.c_uint32), ("param", C.c_float)]


class PhotoChain(C.Structure):
    """llcomp_mi_photo_chain (include/llcomp_mi.h): 68 bytes"""
    _fields_ = [("n_ops", C.c_uint32), ("ops", PhotoOp * PHOTO_MAX_OPS)]


class PhotoGroup(C.Structure):
    """llcomp_mi_photo_group (include/llcomp_mi.h): 16 bytes, chains at 8"""
    _fields_ = [("struct_size", C.c_uint32), ("chains", C.POINTER(PhotoChain))]


class MixSample(C.Structure):
    """llcomp_mi_mix_sample (include/llcomp_mi.h): 48 bytes"""
    _fields_ = [("partner", C.c_uint32), ("flags", C.c_uint32), ("w_own", C.c_float), ("w_partner", C.c_float), ("box", C.c_uint32 * 4),
                ("erase", C.c_uint32 * 4)]


class ComposePiece(C.Structure):
    """llcomp_mi_compose_piece (include/llcomp_mi.h): 40 bytes"""
    _fields_ = [("dst", C.c_uint32), ("src", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32), ("sx", C.c_uint32), ("sy", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PastePiece16(C.Structure):
    """llcomp_mi_paste_piece16 (include/llcomp_mi.h): 76 bytes, ids at 44"""
    _fields_ = [("dst", C.c_uint32), ("src", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32), ("sx", C.c_uint32), ("sy", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("flags", C.c_uint32), ("value_bits", C.c_uint32), ("id_base", C.c_uint32),
                ("ids", C.c_uint32 * 8)]


class PastePiece32(PastePiece16):
    """llcomp_mi_paste_piece32 (include/llcomp_mi.h): the same 76 bytes, id_base any 32-bit value, flags bit 1 VALUE_PIXEL"""


class AlphaPiece(C.Structure):
    """llcomp_mi_alpha_piece (include/llcomp_mi.h): 40 bytes"""
    _fields_ = [("dst", C.c_uint32), ("src", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32), ("sx", C.c_uint32), ("sy", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("flags", C.c_uint32), ("value_bits", C.c_uint32)]


class PastePiece(C.Structure):
    """llcomp_mi_paste_piece (include/llcomp_mi.h): 72 bytes, ids at 40"""
    _fields_ = [("dst", C.c_uint32), ("src", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32), ("sx", C.c_uint32), ("sy", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("flags", C.c_uint32), ("value", C.c_float), ("ids", C.c_uint32 * 8)]


class LabelBox(C.Structure):
    """llcomp_mi_label_box (include/llcomp_mi.h): 20 bytes"""
    _fields_ = [("count", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


class LabelTargets(C.Structure):
    """llcomp_mi_label_targets (include/llcomp_mi.h): 64 bytes, ids at 32"""
    _fields_ = [("struct_size", C.c_uint32), ("map_bytes", C.c_uint32), ("kind", C.c_uint32), ("dtype", C.c_uint32), ("default_value", C.c_int32),
                ("on_bits", C.c_uint32), ("off_bits", C.c_uint32), ("ids", C.c_void_p), ("values", C.c_void_p), ("first", C.c_void_p),
                ("plane_first", C.c_void_p)]


class LabelTargets32(LabelTargets):
    """llcomp_mi_label_targets32 (include/llcomp_mi.h): the same 64 bytes, ids of uint32_t, map_bytes 3 or 4"""


class Info(C.Structure):
    _fields_ = [("format", C.c_uint32), ("channels", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("planar", C.c_uint32), ("n_slices", C.c_uint32),
                ("table_offset", C.c_uint64), ("payload_offset", C.c_uint64), ("small_model", C.c_uint32), ("reserved", C.c_uint32)]


class StreamResult(C.Structure):
    _fields_ = [("slot", C.c_uint32), ("kind", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_uint32),
                ("tag", C.c_uint64), ("data", C.c_void_p), ("len", C.c_uint64)]


_lib = None


def _preload_hip_runtime():
    """libllcomp_mi.so is linked without its own HIP runtime (see csrc/Makefile): exactly one libamdhip64 may live
    in a process.  PyTorch wheels bundle a private copy, so when torch is installed that copy is the one to share
    (streams and device pointers handed over from torch then belong to the same runtime); otherwise /opt/rocm's."""
    import importlib.util

    cands = []
    spec = importlib.util.find_spec("torch")
    if spec is not None and spec.origin:
        cands.append(os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so"))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cands += [os.path.join(rocm, "lib", "libamdhip64.so.7"), os.path.join(rocm, "lib", "libamdhip64.so"), "libamdhip64.so"]
    errs = []
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            return C.CDLL(c, mode=C.RTLD_GLOBAL)
        except OSError as e:  # keep looking
            errs.append(f"{c}: {e}")
    raise ImportError("no HIP runtime (libamdhip64) found for libllcomp_mi.so: " + "; ".join(errs))


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C llcomp_amd/csrc`). llcomp_amd has no CPU fallback.")
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.llcomp_mi_encode.restype = C.c_int
    L.llcomp_mi_encode.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Opts), C.POINTER(u8p), C.POINTER(C.c_size_t)]
    L.llcomp_mi_decode.restype = C.c_int
    L.llcomp_mi_decode.argtypes = [u8p, C.c_size_t, C.c_int32, C.POINTER(u8p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.llcomp_mi_free.restype = None
    L.llcomp_mi_free.argtypes = [C.c_void_p]
    L.llcomp_mi_strerror.restype = C.c_char_p
    L.llcomp_mi_strerror.argtypes = [C.c_int]
    L.llcomp_mi_abi_version.restype = C.c_int
    L.llcomp_mi_device_count.restype = C.c_int
    L.llcomp_mi_probe.restype = C.c_int
    L.llcomp_mi_probe.argtypes = [u8p, C.c_size_t, C.POINTER(Info)]
    L.llcomp_mi_slice_count.restype = C.c_uint32
    L.llcomp_mi_slice_count.argtypes = [C.c_uint32] * 6
    L.llcomp_mi_merge_bands.restype = C.c_int
    L.llcomp_mi_merge_bands.argtypes = [C.POINTER(u8p), C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t)]
    L.llcomp_mi_split_band.restype = C.c_int
    L.llcomp_mi_split_band.argtypes = [u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t)]
    L.llcomp_mi_codec_create.restype = C.c_int
    L.llcomp_mi_codec_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32] + [C.c_uint32] * 7
    L.llcomp_mi_codec_destroy.restype = None
    L.llcomp_mi_codec_destroy.argtypes = [C.c_void_p]
    L.llcomp_mi_codec_slices.restype = C.c_uint32
    L.llcomp_mi_codec_slices.argtypes = [C.c_void_p]
    if hasattr(L, "llcomp_mi_codec_kernel_family"):  # (a stale library must reach the ABI check below, not an AttributeError)
        L.llcomp_mi_codec_kernel_family.restype = C.c_uint32
        L.llcomp_mi_codec_kernel_family.argtypes = [C.c_void_p]
    L.llcomp_mi_codec_workspace_bytes.restype = C.c_uint64
    L.llcomp_mi_codec_workspace_bytes.argtypes = [C.c_void_p]
    L.llcomp_mi_codec_max_payload_bytes.restype = C.c_uint64
    L.llcomp_mi_codec_max_payload_bytes.argtypes = [C.c_void_p]
    L.llcomp_mi_codec_encode.restype = C.c_int
    L.llcomp_mi_codec_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.llcomp_mi_codec_decode.restype = C.c_int
    L.llcomp_mi_codec_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.llcomp_mi_codec_model.restype = C.c_int
    L.llcomp_mi_codec_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.llcomp_mi_status_from_bits.restype = C.c_uint32
    L.llcomp_mi_status_from_bits.argtypes = [C.c_uint32]
    L.llcomp_mi_codec_set_profiling.restype = C.c_int
    L.llcomp_mi_codec_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.llcomp_mi_codec_get_profile.restype = C.c_int
    L.llcomp_mi_codec_get_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.llcomp_mi_encode_into.restype = C.c_int
    L.llcomp_mi_encode_into.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Opts), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.llcomp_mi_decode_into.restype = C.c_int
    L.llcomp_mi_decode_into.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_decode_into_flags"):
        L.llcomp_mi_decode_into_flags.restype = C.c_int
        L.llcomp_mi_decode_into_flags.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.llcomp_mi_host_alloc.restype = C.c_void_p
    L.llcomp_mi_host_alloc.argtypes = [C.c_size_t]
    L.llcomp_mi_host_free.restype = None
    L.llcomp_mi_host_free.argtypes = [C.c_void_p]
    L.llcomp_mi_device_copy_segments.restype = C.c_int
    L.llcomp_mi_device_copy_segments.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint64, C.c_void_p]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_device_range_sums"):
        L.llcomp_mi_device_range_sums.restype = C.c_int
        L.llcomp_mi_device_range_sums.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p]
    L.llcomp_mi_decode_flags.restype = C.c_int
    L.llcomp_mi_decode_flags.argtypes = [u8p, C.c_size_t, C.c_int32, C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.llcomp_mi_codec_create_ex.restype = C.c_int
    L.llcomp_mi_codec_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32] + [C.c_uint32] * 8
    L.llcomp_mi_trim.restype = None
    L.llcomp_mi_trim.argtypes = []
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_set_pool_limit"):  # (an A/B build of older sources may lack them)
        L.llcomp_mi_set_pool_limit.restype = None
        L.llcomp_mi_set_pool_limit.argtypes = [C.c_uint64]
        L.llcomp_mi_pool_limit.restype = C.c_uint64
        L.llcomp_mi_pool_limit.argtypes = []
        L.llcomp_mi_pool_idle_bytes.restype = C.c_uint64
        L.llcomp_mi_pool_idle_bytes.argtypes = []
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_fnv1a64"):
        L.llcomp_mi_fnv1a64.restype = C.c_uint64
        L.llcomp_mi_fnv1a64.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_suggest_tile_w"):
        L.llcomp_mi_suggest_tile_w.restype = C.c_uint32
        L.llcomp_mi_suggest_tile_w.argtypes = [C.c_uint32] * 5
    L.llcomp_mi_reload_tuning.restype = None
    L.llcomp_mi_reload_tuning.argtypes = []
    L.llcomp_mi_stream_create.restype = C.c_int
    L.llcomp_mi_stream_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32] + [C.c_uint32] * 7
    L.llcomp_mi_stream_create_ex.restype = C.c_int
    L.llcomp_mi_stream_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32] + [C.c_uint32] * 8
    L.llcomp_mi_stream_frames_per_job.restype = C.c_uint32
    L.llcomp_mi_stream_frames_per_job.argtypes = [C.c_void_p]
    L.llcomp_mi_stream_submit_decode_batch.restype = C.c_int
    L.llcomp_mi_stream_submit_decode_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint64]
    L.llcomp_mi_stream_result_part.restype = C.c_int
    L.llcomp_mi_stream_result_part.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.llcomp_mi_stream_destroy.restype = None
    L.llcomp_mi_stream_destroy.argtypes = [C.c_void_p]
    L.llcomp_mi_stream_container_capacity.restype = C.c_uint64
    L.llcomp_mi_stream_container_capacity.argtypes = [C.c_void_p]
    L.llcomp_mi_stream_submit_encode.restype = C.c_int
    L.llcomp_mi_stream_submit_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.llcomp_mi_stream_submit_decode.restype = C.c_int
    L.llcomp_mi_stream_submit_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]
    L.llcomp_mi_stream_pending.restype = C.c_int
    L.llcomp_mi_stream_pending.argtypes = [C.c_void_p]
    L.llcomp_mi_stream_poll.restype = C.c_int
    L.llcomp_mi_stream_poll.argtypes = [C.c_void_p]
    L.llcomp_mi_stream_wait.restype = C.c_int
    L.llcomp_mi_stream_wait.argtypes = [C.c_void_p, C.POINTER(StreamResult)]
    L.llcomp_mi_stream_release.restype = C.c_int
    L.llcomp_mi_stream_release.argtypes = [C.c_void_p, C.c_uint32]
    old_ab_build = "LLCOMP_MI_LIB" in os.environ and L.llcomp_mi_abi_version() != ABI_VERSION  # (tools/lib_ab.sh against earlier commits)
    if not old_ab_build:
        i32p = C.POINTER(C.c_int32)
        L.llcomp_mi_decode_devices.restype = C.c_int
        L.llcomp_mi_decode_devices.argtypes = [u8p, C.c_size_t, i32p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.llcomp_mi_decode_into_devices.restype = C.c_int
        L.llcomp_mi_decode_into_devices.argtypes = [C.c_void_p, C.c_size_t, i32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.llcomp_mi_last_device_error.restype = C.c_int
        L.llcomp_mi_last_device_error.argtypes = [i32p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.llcomp_mi_plan_chunks.restype = C.c_int
        L.llcomp_mi_plan_chunks.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        L.llcomp_mi_stream_create_multi.restype = C.c_int
        L.llcomp_mi_stream_create_multi.argtypes = [C.POINTER(C.c_void_p), i32p, C.c_uint32] + [C.c_uint32] * 8
        L.llcomp_mi_stream_devices.restype = C.c_uint32
        L.llcomp_mi_stream_devices.argtypes = [C.c_void_p]
        L.llcomp_mi_codec_prepare.restype = C.c_int
        L.llcomp_mi_codec_prepare.argtypes = [C.c_void_p, C.c_uint32]
        L.llcomp_mi_codec_get_counters.restype = C.c_int
        L.llcomp_mi_codec_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_int]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_region_plan"):  # region decode
        u32p = C.POINTER(C.c_uint32)
        L.llcomp_mi_region_plan.restype = C.c_int
        L.llcomp_mi_region_plan.argtypes = [C.c_uint32] * 10 + [u32p, u32p]
        L.llcomp_mi_decode_region.restype = C.c_int
        L.llcomp_mi_decode_region.argtypes = [u8p, C.c_size_t, C.c_int32, C.c_uint32] + [C.c_uint32] * 4 + [C.POINTER(u8p), u32p]
        L.llcomp_mi_decode_region_into.restype = C.c_int
        L.llcomp_mi_decode_region_into.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p, C.c_size_t, u32p]
        L.llcomp_mi_codec_decode_region.restype = C.c_int
        L.llcomp_mi_codec_decode_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 3
        L.llcomp_mi_codec_region_family.restype = C.c_uint32
        L.llcomp_mi_codec_region_family.argtypes = [C.c_void_p] + [C.c_uint32] * 4
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_regions_plan"):  # a rectangle per frame
        u32p = C.POINTER(C.c_uint32)
        L.llcomp_mi_regions_plan.restype = C.c_int
        L.llcomp_mi_regions_plan.argtypes = [C.c_uint32] * 8 + [u32p, C.c_uint32, u32p, u32p]
        L.llcomp_mi_codec_decode_regions.restype = C.c_int
        L.llcomp_mi_codec_decode_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u32p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
        L.llcomp_mi_codec_regions_family.restype = C.c_uint32
        L.llcomp_mi_codec_regions_family.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, u32p, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_regions_gather"):  # crops of host containers
        u32p, u64p, ptrs, sizes = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        L.llcomp_mi_regions_gather.restype = C.c_int
        L.llcomp_mi_regions_gather.argtypes = [ptrs, sizes, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                               u64p, u32p, u32p]
        L.llcomp_mi_codec_decode_regions_host.restype = C.c_int
        L.llcomp_mi_codec_decode_regions_host.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
        L.llcomp_mi_stream_submit_decode_regions.restype = C.c_int
        L.llcomp_mi_stream_submit_decode_regions.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_uint32, C.c_uint32, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_resize_weights"):  # crops of different sizes, resized to one shape
        u32p, i32p, ptrs, sizes = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        L.llcomp_mi_resize_weights.restype = C.c_uint32
        L.llcomp_mi_resize_weights.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_resized_regions_plan.restype = C.c_int
        L.llcomp_mi_resized_regions_plan.argtypes = [C.c_uint32] * 6 + [u32p, C.c_uint32, u32p, u32p]
        L.llcomp_mi_codec_decode_resized_regions.restype = C.c_int
        L.llcomp_mi_codec_decode_resized_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u32p, C.c_void_p, C.c_uint32,
                                                             C.c_uint32] + [C.c_void_p] * 3
        L.llcomp_mi_codec_decode_resized_regions_host.restype = C.c_int
        L.llcomp_mi_codec_decode_resized_regions_host.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
        L.llcomp_mi_stream_submit_decode_resized_regions.restype = C.c_int
        L.llcomp_mi_stream_submit_decode_resized_regions.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]
        L.llcomp_mi_codec_allocated_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_allocated_bytes.argtypes = [C.c_void_p]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_output_table"):  # ... in an output format (dtype, layout, normalisation)
        u32p, ptrs, sizes, fmtp = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(OutputFormat)
        L.llcomp_mi_output_table.restype = C.c_int
        L.llcomp_mi_output_table.argtypes = [fmtp, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_decode_resized_regions_ex.restype = C.c_int
        L.llcomp_mi_codec_decode_resized_regions_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u32p, C.c_void_p, C.c_uint32,
                                                                C.c_uint32, fmtp] + [C.c_void_p] * 3
        L.llcomp_mi_codec_decode_resized_regions_host_ex.restype = C.c_int
        L.llcomp_mi_codec_decode_resized_regions_host_ex.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                                     fmtp] + [C.c_void_p] * 3
        L.llcomp_mi_stream_submit_decode_resized_regions_ex.restype = C.c_int
        L.llcomp_mi_stream_submit_decode_resized_regions_ex.argtypes = [C.c_void_p, ptrs, sizes, u32p, C.c_void_p, C.c_uint32, C.c_uint32, fmtp,
                                                                        C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_replace_slices"):  # region update
        u32p, sizep = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)
        L.llcomp_mi_replace_slices.restype = C.c_int
        L.llcomp_mi_replace_slices.argtypes = [C.c_void_p, C.c_size_t, u32p, C.c_void_p, C.c_void_p, C.POINTER(u8p), sizep]
        L.llcomp_mi_replace_slices_into.restype = C.c_int
        L.llcomp_mi_replace_slices_into.argtypes = [C.c_void_p, C.c_size_t, u32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, sizep]
        L.llcomp_mi_update_region.restype = C.c_int
        L.llcomp_mi_update_region.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p, C.POINTER(u8p), sizep]
        L.llcomp_mi_update_region_into.restype = C.c_int
        L.llcomp_mi_update_region_into.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p,
                                                                                                                    C.c_size_t, sizep]
        L.llcomp_mi_codec_encode_region.restype = C.c_int
        L.llcomp_mi_codec_encode_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p,
                                                                                                                        C.c_uint64] + [C.c_void_p] * 4
        L.llcomp_mi_codec_update_region.restype = C.c_int
        L.llcomp_mi_codec_update_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p,
                                                                                                                        C.c_uint64] + [C.c_void_p] * 4
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_resize_filter_weights"):  # PIL's filters, one per frame
        L.llcomp_mi_resize_filter_weights.restype = C.c_uint32
        L.llcomp_mi_resize_filter_weights.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_views_plan"):  # several views of each frame
        u32p, ptrs, sizes, grp = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(ViewGroup)
        L.llcomp_mi_views_plan.restype = C.c_int
        L.llcomp_mi_views_plan.argtypes = [C.c_uint32] * 7 + [grp, C.c_uint32, u32p, u32p, u32p, u32p]
        L.llcomp_mi_codec_decode_views.restype = C.c_int
        L.llcomp_mi_codec_decode_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, grp, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_views_host.argtypes = [C.c_void_p, ptrs, sizes, grp, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_views_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_views_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_pad_axis"):  # crops that leave the image
        u32p, i32p, ptrs, sizes = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        grp, fmtp, padp = C.POINTER(ViewGroup), C.POINTER(OutputFormat), C.POINTER(Pad)
        L.llcomp_mi_pad_axis.restype = C.c_int
        L.llcomp_mi_pad_axis.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, u32p, u32p]
        L.llcomp_mi_padded_filter_weights.restype = C.c_uint32
        L.llcomp_mi_padded_filter_weights.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u32p] + [C.c_void_p] * 3
        L.llcomp_mi_padded_regions_plan.restype = C.c_int
        L.llcomp_mi_padded_regions_plan.argtypes = [C.c_uint32, C.c_uint32, i32p, C.c_uint32, padp, u32p]
        L.llcomp_mi_codec_decode_padded_regions.restype = C.c_int
        L.llcomp_mi_codec_decode_padded_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, i32p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                            padp, fmtp] + [C.c_void_p] * 3
        L.llcomp_mi_codec_decode_padded_regions_host.restype = C.c_int
        L.llcomp_mi_codec_decode_padded_regions_host.argtypes = [C.c_void_p, ptrs, sizes, i32p, C.c_void_p, C.c_uint32, C.c_uint32, padp,
                                                                 fmtp] + [C.c_void_p] * 3
        L.llcomp_mi_codec_decode_padded_views.restype = C.c_int
        L.llcomp_mi_codec_decode_padded_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, grp, C.c_uint32, padp, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_padded_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_padded_views_host.argtypes = [C.c_void_p, ptrs, sizes, grp, C.c_uint32, padp, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_padded_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_padded_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_warp_source_rect"):  # views under an affine map
        u32p, f64p, ptrs, sizes, wgrp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(WarpGroup)
        L.llcomp_mi_warp_source_rect.restype = C.c_int
        L.llcomp_mi_warp_source_rect.argtypes = [C.c_uint32, C.c_uint32, f64p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
        L.llcomp_mi_warp_views_plan.restype = C.c_int
        L.llcomp_mi_warp_views_plan.argtypes = [C.c_uint32] * 7 + [wgrp, C.c_uint32, u32p, u32p, u32p, u32p]
        L.llcomp_mi_warp_reference.restype = C.c_int
        L.llcomp_mi_warp_reference.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, f64p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.c_void_p]
        L.llcomp_mi_codec_decode_warped_views.restype = C.c_int
        L.llcomp_mi_codec_decode_warped_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, wgrp, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_warped_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_warped_views_host.argtypes = [C.c_void_p, ptrs, sizes, wgrp, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_warp_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_warp_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_photo_reference"):  # photometric chains
        ptrs, sizes, padp = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(Pad)
        grp, wgrp, pgrp = C.POINTER(ViewGroup), C.POINTER(WarpGroup), C.POINTER(PhotoGroup)
        L.llcomp_mi_photo_reference.restype = C.c_int
        L.llcomp_mi_photo_reference.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PhotoOp), C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_decode_photo_views.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, grp, C.c_uint32, padp, pgrp, C.c_void_p,
                                                         C.c_void_p]
        L.llcomp_mi_codec_decode_photo_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_views_host.argtypes = [C.c_void_p, ptrs, sizes, grp, C.c_uint32, padp, pgrp, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_photo_warped_views.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_warped_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, wgrp, C.c_uint32, pgrp, C.c_void_p,
                                                                C.c_void_p]
        L.llcomp_mi_codec_decode_photo_warped_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_warped_views_host.argtypes = [C.c_void_p, ptrs, sizes, wgrp, C.c_uint32, pgrp, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_photo_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_photo_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_perspective_source_rect"):  # views under a projective map
        u32p, f64p, ptrs, sizes = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        qgrp, pgrp = C.POINTER(PerspectiveGroup), C.POINTER(PhotoGroup)
        L.llcomp_mi_perspective_source_rect.restype = C.c_int
        L.llcomp_mi_perspective_source_rect.argtypes = [C.c_uint32, C.c_uint32, f64p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
        L.llcomp_mi_perspective_views_plan.restype = C.c_int
        L.llcomp_mi_perspective_views_plan.argtypes = [C.c_uint32] * 7 + [qgrp, C.c_uint32, u32p, u32p, u32p, u32p]
        L.llcomp_mi_perspective_reference.restype = C.c_int
        L.llcomp_mi_perspective_reference.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, f64p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                      C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_decode_perspective_views.restype = C.c_int
        L.llcomp_mi_codec_decode_perspective_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, qgrp, C.c_uint32, C.c_void_p,
                                                               C.c_void_p]
        L.llcomp_mi_codec_decode_perspective_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_perspective_views_host.argtypes = [C.c_void_p, ptrs, sizes, qgrp, C.c_uint32, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_photo_perspective_views.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_perspective_views.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, qgrp, C.c_uint32, pgrp,
                                                                     C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_decode_photo_perspective_views_host.restype = C.c_int
        L.llcomp_mi_codec_decode_photo_perspective_views_host.argtypes = [C.c_void_p, ptrs, sizes, qgrp, C.c_uint32, pgrp, C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_perspective_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_perspective_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
        L.llcomp_mi_codec_photo_perspective_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_photo_perspective_workspace_bytes.argtypes = [C.c_void_p, C.c_uint64]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_mix_plan"):  # batch mixing
        u32p, recs, f32p = C.POINTER(C.c_uint32), C.POINTER(MixSample), C.POINTER(C.c_float)
        L.llcomp_mi_mix_plan.restype = C.c_int
        L.llcomp_mi_mix_plan.argtypes = [C.c_uint32, recs, u32p, u32p, u32p, u32p]
        L.llcomp_mi_mix_segment.restype = C.c_uint32
        L.llcomp_mi_mix_segment.argtypes = []
        L.llcomp_mi_mix_reference.restype = C.c_int
        L.llcomp_mi_mix_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [recs, f32p, C.c_void_p]
        L.llcomp_mi_codec_mix_batch.restype = C.c_int
        L.llcomp_mi_codec_mix_batch.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [recs, f32p, C.c_void_p]
        L.llcomp_mi_codec_mix_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_mix_workspace_bytes.argtypes = [C.c_void_p] + [C.c_uint32] * 4
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_orient_reference"):  # batch orientation
        L.llcomp_mi_orient_reference.restype = C.c_int
        L.llcomp_mi_orient_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [u8p, C.c_void_p]
        L.llcomp_mi_orient_tile.restype = C.c_uint32
        L.llcomp_mi_orient_tile.argtypes = []
        L.llcomp_mi_codec_orient_batch.restype = C.c_int
        L.llcomp_mi_codec_orient_batch.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [u8p, C.c_void_p]
        L.llcomp_mi_codec_orient_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_orient_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_compose_reference"):  # batch composition
        u32p, recs, f32p = C.POINTER(C.c_uint32), C.POINTER(ComposePiece), C.POINTER(C.c_float)
        L.llcomp_mi_compose_reference.restype = C.c_int
        L.llcomp_mi_compose_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 6 + [recs, C.c_uint32, f32p,
                                                                                                                  C.c_uint32, C.c_void_p]
        L.llcomp_mi_compose_plan.restype = C.c_int
        L.llcomp_mi_compose_plan.argtypes = [C.c_uint32] * 9 + [recs, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        L.llcomp_mi_compose_tile.restype = C.c_uint32
        L.llcomp_mi_compose_tile.argtypes = []
        L.llcomp_mi_compose_tile_rows.restype = C.c_uint32
        L.llcomp_mi_compose_tile_rows.argtypes = [C.c_uint32]
        L.llcomp_mi_compose_max_pieces_per_sample.restype = C.c_uint32
        L.llcomp_mi_compose_max_pieces_per_sample.argtypes = []
        L.llcomp_mi_codec_compose_batch.restype = C.c_int
        L.llcomp_mi_codec_compose_batch.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 5 + [
            recs, C.c_uint32, f32p, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_compose_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_compose_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_paste_reference"):  # batch copy-paste
        u32p, recs = C.POINTER(C.c_uint32), C.POINTER(PastePiece)
        L.llcomp_mi_paste_reference.restype = C.c_int
        L.llcomp_mi_paste_reference.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 6 + [recs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_paste_plan.restype = C.c_int
        L.llcomp_mi_paste_plan.argtypes = [C.c_uint32] * 9 + [recs, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        L.llcomp_mi_paste_max_pieces_per_sample.restype = C.c_uint32
        L.llcomp_mi_paste_max_pieces_per_sample.argtypes = []
        L.llcomp_mi_codec_paste_batch.restype = C.c_int
        L.llcomp_mi_codec_paste_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 5 + [
            recs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_paste_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_paste_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_paste16_reference"):  # batch copy-paste by 16-bit ids
        u32p, recs = C.POINTER(C.c_uint32), C.POINTER(PastePiece16)
        L.llcomp_mi_paste16_reference.restype = C.c_int
        L.llcomp_mi_paste16_reference.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 6 + [recs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_paste16_plan.restype = C.c_int
        L.llcomp_mi_paste16_plan.argtypes = [C.c_uint32] * 9 + [recs, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        L.llcomp_mi_codec_paste_batch16.restype = C.c_int
        L.llcomp_mi_codec_paste_batch16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 5 + [
            recs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_paste16_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_paste16_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_label_boxes_reference"):  # label boxes
        L.llcomp_mi_label_boxes_reference.restype = C.c_int
        L.llcomp_mi_label_boxes_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p]
        L.llcomp_mi_label_boxes_rows.restype = C.c_uint32
        L.llcomp_mi_label_boxes_rows.argtypes = []
        L.llcomp_mi_codec_label_boxes.restype = C.c_int
        L.llcomp_mi_codec_label_boxes.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_label_boxes16_reference"):  # label boxes of listed ids
        L.llcomp_mi_label_boxes16_reference.restype = C.c_int
        L.llcomp_mi_label_boxes16_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] * 3
        L.llcomp_mi_label_boxes16_max_ids.restype = C.c_uint32
        L.llcomp_mi_label_boxes16_max_ids.argtypes = []
        L.llcomp_mi_codec_label_boxes16.restype = C.c_int
        L.llcomp_mi_codec_label_boxes16.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] * 4
        L.llcomp_mi_codec_label_boxes16_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_label_boxes16_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_label_targets_reference"):  # label targets
        L.llcomp_mi_label_targets_reference.restype = C.c_int
        L.llcomp_mi_label_targets_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.POINTER(LabelTargets), C.c_void_p]
        L.llcomp_mi_label_targets_out_bytes.restype = C.c_uint64
        L.llcomp_mi_label_targets_out_bytes.argtypes = [C.c_uint32] * 3 + [C.POINTER(LabelTargets)]
        L.llcomp_mi_label_targets_segment.restype = C.c_uint32
        L.llcomp_mi_label_targets_segment.argtypes = []
        L.llcomp_mi_label_targets_max_planes.restype = C.c_uint32
        L.llcomp_mi_label_targets_max_planes.argtypes = []
        L.llcomp_mi_codec_label_targets.restype = C.c_int
        L.llcomp_mi_codec_label_targets.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.POINTER(LabelTargets), C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_label_targets_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_label_targets_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_label_boxes32_reference"):  # wide id maps
        L.llcomp_mi_label_boxes32_reference.restype = C.c_int
        L.llcomp_mi_label_boxes32_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 3
        L.llcomp_mi_codec_label_boxes32.restype = C.c_int
        L.llcomp_mi_codec_label_boxes32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 4
        L.llcomp_mi_codec_label_boxes32_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_label_boxes32_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.llcomp_mi_label_targets32_reference.restype = C.c_int
        L.llcomp_mi_label_targets32_reference.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.POINTER(LabelTargets32), C.c_void_p]
        L.llcomp_mi_label_targets32_out_bytes.restype = C.c_uint64
        L.llcomp_mi_label_targets32_out_bytes.argtypes = [C.c_uint32] * 3 + [C.POINTER(LabelTargets32)]
        L.llcomp_mi_codec_label_targets32.restype = C.c_int
        L.llcomp_mi_codec_label_targets32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 3 + [C.POINTER(LabelTargets32), C.c_void_p, C.c_void_p]
        L.llcomp_mi_codec_label_targets32_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_label_targets32_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_paste32_reference"):  # batch copy-paste by wide ids
        recs32, u32p = C.POINTER(PastePiece32), C.POINTER(C.c_uint32)
        L.llcomp_mi_paste32_reference.restype = C.c_int
        L.llcomp_mi_paste32_reference.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] + [C.c_uint32] * 6 + [recs32, C.c_uint32, C.c_void_p]
        L.llcomp_mi_paste32_plan.restype = C.c_int
        L.llcomp_mi_paste32_plan.argtypes = [C.c_uint32] * 10 + [recs32, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        L.llcomp_mi_codec_paste_batch32.restype = C.c_int
        L.llcomp_mi_codec_paste_batch32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] + [C.c_uint32] * 5 + [recs32, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_paste32_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_paste32_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ or hasattr(L, "llcomp_mi_alpha_paste_reference"):  # batch alpha paste
        arecs, u32p = C.POINTER(AlphaPiece), C.POINTER(C.c_uint32)
        L.llcomp_mi_alpha_paste_reference.restype = C.c_int
        L.llcomp_mi_alpha_paste_reference.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] + [C.c_uint32] * 6 + [arecs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_alpha_paste_plan.restype = C.c_int
        L.llcomp_mi_alpha_paste_plan.argtypes = [C.c_uint32] * 11 + [arecs, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        L.llcomp_mi_codec_alpha_paste_batch.restype = C.c_int
        L.llcomp_mi_codec_alpha_paste_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] + [C.c_uint32] * 5 + [arecs, C.c_uint32, C.c_void_p]
        L.llcomp_mi_codec_alpha_paste_workspace_bytes.restype = C.c_uint64
        L.llcomp_mi_codec_alpha_paste_workspace_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if "LLCOMP_MI_LIB" not in os.environ and L.llcomp_mi_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {L.llcomp_mi_abi_version()}, this binding was written for {ABI_VERSION}: rebuild the library")
    _lib = L
    return L
