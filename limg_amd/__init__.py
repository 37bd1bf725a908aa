"""limg_amd -- MI355X (gfx950) implementation of limg's encode hot path.

This package is a thin ctypes view of the C ABI in include/limg_hip.h (liblimg_hip.so, built in-tree by limg_amd/build.py
from the hand-written HIP sources in limg_amd/csrc).  It is plumbing for the tests and the bench: the product is the
shared library.  There is NO CPU fallback: if the library is missing, or no HIP device is present, calls raise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_LIB_PATH = os.path.join(HERE, "liblimg_hip_test.so")  # the -DLIMG_HIP_TEST_HOOKS build (include/limg_hip_test_hooks.h): what tests/conftest.py selects
LIB_PATH = os.environ.get("LIMG_HIP_LIB") or os.path.join(HERE, "liblimg_hip.so")  # LIMG_HIP_LIB: A/B runs against another build of the same ABI ("test" = TEST_LIB_PATH)
if LIB_PATH == "test":
    LIB_PATH = TEST_LIB_PATH

P32 = ("pDecoded", "pShiftABCX", "pColAMin", "pColAMax", "pColBMin", "pColBMax", "pColCMin", "pColCMax")
P8 = ("pFactorsA", "pFactorsB", "pFactorsC")
PLANES = P32 + P8

# every symbol include/limg_hip.h declares (checked by tests/test_host.py without a GPU)
ABI_SYMBOLS = (
    "limg_hip_init", "limg_hip_shutdown", "limg_hip_default_options_sized", "limg_hip_set_options", "limg_hip_get_options", "limg_hip_encode3d", "limg_hip_encode3d_perf",
    "limg_hip_encode3d_stats", "limg_hip_blocked_encode3d_stats",
    "limg_hip_encode3d_device", "limg_hip_encode3d_batch_device", "limg_hip_last_stats", "limg_hip_compare", "limg_hip_compare_device", "limg_hip_synth_random_gradient_device",
    "limg_hip_synth_photo_noise_device", "limg_hip_context_device_bytes", "limg_hip_version", "limg_hip_profile_begin", "limg_hip_profile_end",
    "limg_hip_host_noise_table", "limg_hip_noise_table_device", "limg_hip_host_chain_call", "limg_hip_host_chain_checkpoints", "limg_hip_host_dense_checkpoints", "limg_hip_host_accurate_table", "limg_hip_host_partition", "limg_hip_check_device_status",
    "limg_hip_stream_bound", "limg_hip_encode_stream_device", "limg_hip_decode_stream_device", "limg_hip_encode_stream", "limg_hip_decode_stream",
    "limg_hip_stream_info", "limg_hip_encode_stream_batch_device", "limg_hip_encode_stream_batch", "limg_hip_encode_stream_batch_ef_device", "limg_hip_encode_stream_batch_ef",
    "limg_hip_stream_sizes_device", "limg_hip_stream_sizes", "limg_hip_encode_stream_budget_device", "limg_hip_encode_stream_budget",
    "limg_hip_encode_stream_budget_batch_device", "limg_hip_encode_stream_budget_batch",
    "limg_hip_encode_stream_quality_device", "limg_hip_encode_stream_quality", "limg_hip_encode_stream_quality_batch_device", "limg_hip_encode_stream_quality_batch",
    "limg_hip_encode_stream_list_device", "limg_hip_encode_stream_list", "limg_hip_encode_stream_quality_list_device", "limg_hip_encode_stream_quality_list",
    "limg_hip_encode_stream_budget_list_device", "limg_hip_encode_stream_budget_list", "limg_hip_stream_sizes_list_device", "limg_hip_stream_sizes_list",
    "limg_hip_blocked_stream_bound", "limg_hip_blocked_encode_stream_device", "limg_hip_blocked_decode_stream_device", "limg_hip_blocked_encode_stream",
    "limg_hip_blocked_decode_stream", "limg_hip_blocked_stream_info", "limg_hip_blocked_last_stream",
    "limg_hip_decode_stream_window_device", "limg_hip_blocked_decode_stream_window_device", "limg_hip_decode_stream_window", "limg_hip_blocked_decode_stream_window",
    "limg_hip_decode_stream_windows_device", "limg_hip_blocked_decode_stream_windows_device", "limg_hip_decode_stream_windows", "limg_hip_blocked_decode_stream_windows",
    "limg_hip_decode_stream_windows_error_device", "limg_hip_blocked_decode_stream_windows_error_device", "limg_hip_decode_stream_windows_error",
    "limg_hip_blocked_decode_stream_windows_error", "limg_hip_stream_compare", "limg_hip_error_sum_for_psnr",
    "limg_hip_decode_stream_windows_tensor_device", "limg_hip_blocked_decode_stream_windows_tensor_device", "limg_hip_decode_stream_windows_tensor",
    "limg_hip_blocked_decode_stream_windows_tensor",
    "limg_hip_decode_stream_windows_scaled_device", "limg_hip_blocked_decode_stream_windows_scaled_device", "limg_hip_decode_stream_windows_scaled_tensor_device",
    "limg_hip_blocked_decode_stream_windows_scaled_tensor_device", "limg_hip_decode_stream_windows_scaled", "limg_hip_blocked_decode_stream_windows_scaled",
    "limg_hip_decode_stream_windows_scaled_tensor", "limg_hip_blocked_decode_stream_windows_scaled_tensor",
    "limg_hip_decode_stream_windows_resized_device", "limg_hip_blocked_decode_stream_windows_resized_device", "limg_hip_decode_stream_windows_resized_tensor_device",
    "limg_hip_blocked_decode_stream_windows_resized_tensor_device", "limg_hip_decode_stream_windows_resized", "limg_hip_blocked_decode_stream_windows_resized",
    "limg_hip_decode_stream_windows_resized_tensor", "limg_hip_blocked_decode_stream_windows_resized_tensor",
    "limg_hip_stream_splice_device", "limg_hip_stream_splice", "limg_hip_stream_crop_device", "limg_hip_stream_crop",
    "limg_hip_blocked_encode3d", "limg_hip_blocked_encode3d_device", "limg_hip_blocked_regions", "limg_hip_blocked_timing", "limg_hip_blocked_kernel_timing", "limg_hip_blocked_match_bits", "limg_hip_host_blocked_matches",
    "limg_hip_host_blocked_merge", "limg_hip_host_blocked_match_words", "limg_hip_host_blocked_match_bits",
    "limg_hip_comm_unique_id", "limg_hip_comm_init", "limg_hip_comm_destroy", "limg_hip_comm_info", "limg_hip_gather_stream", "limg_hip_encode3d_single_chain_device",
    "limg_hip_encode3d_chain_device", "limg_hip_host_gather_offsets", "limg_hip_host_chain_bases",
)
TEST_ABI_SYMBOLS = ("limg_hip_default_test_options_sized", "limg_hip_set_test_options", "limg_hip_test_live_resources")  # include/limg_hip_test_hooks.h: exported by liblimg_hip_test.so only
COMM_ID_BYTES = 128

# limg_blocked_encode3d_info (src/limg.h:39-44), member order
BLOCKED_PLANES = (("pDecoded", np.uint32), ("pFactorsA", np.uint8), ("pFactorsB", np.uint8), ("pFactorsC", np.uint8), ("pBlockError", np.uint8), ("pBitsPerPixel", np.uint8),
                  ("pShiftABCX", np.uint32), ("pColAMin", np.uint32), ("pColAMax", np.uint32), ("pColBMin", np.uint32), ("pColBMax", np.uint32), ("pColCMin", np.uint32),
                  ("pColCMax", np.uint32), ("pBlockIndex", np.uint32))
REGION_DTYPE = np.dtype([("ox", "<u4"), ("oy", "<u4"), ("rx", "<u4"), ("ry", "<u4")])

STREAM_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("sizeX", "<u4"), ("sizeY", "<u4"), ("channels", "<u4"), ("errorFactor", "<u4"),
                                ("blocksX", "<u4"), ("blocksY", "<u4"), ("payloadWords", "<u8"), ("totalBytes", "<u8"), ("flags", "<u4"), ("reserved", "<u4", 3)])
STREAM_BLOCK_DTYPE = np.dtype([("dirA_min", "<i2", 4), ("dirA_max", "<i2", 4), ("dirB_offset", "<i2", 4), ("dirB_mag", "<i2", 4), ("dirC_offset", "<i2", 4),
                               ("dirC_mag", "<i2", 4), ("shift", "<u4"), ("payloadWord", "<u4")])

# version 2 (merged-block) stream: the header is STREAM_HEADER_DTYPE with version = 2, reserved[0] = rectangle count, flags bit 2
STREAM_VERSION_BLOCKED = 2
STREAM_FLAG_MERGED = 4
STREAM_RECT_DTYPE = np.dtype([("dirA_min", "<i2", 4), ("dirA_max", "<i2", 4), ("dirB_offset", "<i2", 4), ("dirB_mag", "<i2", 4), ("dirC_offset", "<i2", 4),
                              ("dirC_mag", "<i2", 4), ("shift", "<u4"), ("payloadWord", "<u4"), ("ox", "<u2"), ("oy", "<u2"), ("rx", "<u2"), ("ry", "<u2")])

RECORD_DTYPE = np.dtype([("avg", "<f4", 4), ("dirA_min", "<i2", 4), ("dirA_max", "<i2", 4), ("dirB_offset", "<i2", 4),
                         ("dirB_mag", "<i2", 4), ("dirC_offset", "<i2", 4), ("dirC_mag", "<i2", 4)])


class LimgHipError(RuntimeError):
    pass


class Info(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PLANES]


class CompactOut(C.Structure):
    _fields_ = [("pRecords", C.c_void_p), ("pShifts", C.c_void_p)]


class Window(C.Structure):
    """limg_hip_window: one window and where it goes"""
    _fields_ = [("x0", C.c_size_t), ("y0", C.c_size_t), ("width", C.c_size_t), ("height", C.c_size_t), ("pOut", C.c_void_p), ("outStridePixels", C.c_size_t)]


class WindowJob(C.Structure):
    """limg_hip_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", Window)]


class ErrorWindow(C.Structure):
    """limg_hip_error_window: one window and the original it is compared with"""
    _fields_ = [("x0", C.c_size_t), ("y0", C.c_size_t), ("width", C.c_size_t), ("height", C.c_size_t), ("pOriginal", C.c_void_p), ("originalStridePixels", C.c_size_t)]


class ErrorWindowJob(C.Structure):
    """limg_hip_error_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", ErrorWindow)]


TENSOR_F32, TENSOR_F16 = 0, 1  # limg_hip_tensor_format.type


class TensorFormat(C.Structure):
    """limg_hip_tensor_format: element type, plane count and the per-channel scale / bias of the tensor entries"""
    _fields_ = [("type", C.c_uint32), ("planes", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class TensorWindow(C.Structure):
    """limg_hip_tensor_window: one window and the planes it goes to"""
    _fields_ = [("x0", C.c_size_t), ("y0", C.c_size_t), ("width", C.c_size_t), ("height", C.c_size_t), ("pOut", C.c_void_p), ("rowStride", C.c_size_t),
                ("planeStride", C.c_size_t)]


class TensorWindowJob(C.Structure):
    """limg_hip_tensor_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", TensorWindow)]


class ScaledWindow(C.Structure):
    """limg_hip_scaled_window: limg_hip_window and the level"""
    _fields_ = Window._fields_ + [("log2Scale", C.c_uint32)]


class ScaledWindowJob(C.Structure):
    """limg_hip_scaled_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", ScaledWindow)]


class ScaledTensorWindow(C.Structure):
    """limg_hip_scaled_tensor_window: limg_hip_tensor_window and the level"""
    _fields_ = TensorWindow._fields_ + [("log2Scale", C.c_uint32)]


class ScaledTensorWindowJob(C.Structure):
    """limg_hip_scaled_tensor_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", ScaledTensorWindow)]


RESIZE_AUTO, RESIZE_FLIP_X = 0xFFFFFFFF, 1  # limg_hip_resized_*window.log2Scale / .flags


class ResizedWindow(C.Structure):
    """limg_hip_resized_window: a source rectangle, the output's size, the level (0 .. 3 or RESIZE_AUTO) and the flags"""
    _fields_ = Window._fields_ + [("outWidth", C.c_size_t), ("outHeight", C.c_size_t), ("log2Scale", C.c_uint32), ("flags", C.c_uint32)]


class ResizedWindowJob(C.Structure):
    """limg_hip_resized_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", ResizedWindow)]


class ResizedTensorWindow(C.Structure):
    """limg_hip_resized_tensor_window: the same into planes"""
    _fields_ = TensorWindow._fields_ + [("outWidth", C.c_size_t), ("outHeight", C.c_size_t), ("log2Scale", C.c_uint32), ("flags", C.c_uint32)]


class ResizedTensorWindowJob(C.Structure):
    """limg_hip_resized_tensor_window_job: one window of one stream"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("sizeX", C.c_size_t), ("sizeY", C.c_size_t), ("window", ResizedTensorWindow)]


# (a level leads the window tuple, the pixels go to planes) -> the entry's window and job struct
_WINDOW_TYPES = {(False, False): (Window, WindowJob), (False, True): (TensorWindow, TensorWindowJob),
                 (True, False): (ScaledWindow, ScaledWindowJob), (True, True): (ScaledTensorWindow, ScaledTensorWindowJob)}


def tensor_format(dtype, planes, scale, bias):
    """dtype: "float32" / "float16" (or the numpy / torch dtype); scale, bias: one value per plane (a 4th is 1 / 0 where only three are given)"""
    name = str(dtype).split(".")[-1].replace("'>", "")
    assert name in ("float32", "float16"), dtype
    scale, bias = list(scale) + [1.0] * (4 - len(scale)), list(bias) + [0.0] * (4 - len(bias))
    return TensorFormat(TENSOR_F16 if name == "float16" else TENSOR_F32, planes, (C.c_float * 4)(*scale[:4]), (C.c_float * 4)(*bias[:4]))


class BudgetResult(C.Structure):
    """limg_hip_budget_result: what a budgeted stream encode chose"""
    _fields_ = [("struct_size", C.c_uint32), ("errorFactor", C.c_uint32), ("probes", C.c_uint32), ("withinBudget", C.c_uint32), ("bytes", C.c_uint64)]


class QualityResult(C.Structure):
    """limg_hip_quality_result: what a stream encode to a quality target chose"""
    _fields_ = [("struct_size", C.c_uint32), ("errorFactor", C.c_uint32), ("probes", C.c_uint32), ("withinTarget", C.c_uint32), ("bytes", C.c_uint64), ("errorSum", C.c_uint64)]


class StreamListItem(C.Structure):
    """limg_hip_stream_list_item: one image of a list of mixed shapes -- its pixels, its stream buffer and capacity, its size and its error factor"""
    _fields_ = [("pIn", C.c_void_p), ("pStream", C.c_void_p), ("capacity", C.c_uint64), ("sizeX", C.c_uint32), ("sizeY", C.c_uint32), ("errorFactor", C.c_uint32),
                ("reserved", C.c_uint32)]


class SplicePiece(C.Structure):
    """limg_hip_splice_piece: a rectangle of blocks of a source stream and where its first block lands in the output's block grid"""
    _fields_ = [("pStream", C.c_void_p), ("streamBytes", C.c_size_t), ("srcSizeX", C.c_uint32), ("srcSizeY", C.c_uint32), ("srcBx", C.c_uint32), ("srcBy", C.c_uint32),
                ("dstBx", C.c_uint32), ("dstBy", C.c_uint32), ("blocksW", C.c_uint32), ("blocksH", C.c_uint32)]


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("forced_shift", C.c_int32 * 3), ("force_split_kernels", C.c_int32), ("dither_pcg", C.c_int32), ("float_mode", C.c_int32),
                ("legacy_float_stage", C.c_int32), ("collect_stats", C.c_int32), ("host_noise_table", C.c_int32), ("batch_sub_images", C.c_int32), ("ragged_bands", C.c_int32),
                ("ragged_walk_threads", C.c_int32)]


class TestOptions(C.Structure):
    """include/limg_hip_test_hooks.h -- liblimg_hip_test.so only"""
    _fields_ = [("struct_size", C.c_uint32), ("record_limit", C.c_int32), ("batch_chunk", C.c_int32), ("wg_per_cu", C.c_int32), ("whole_image_ragged", C.c_int32),
                ("pipeline", C.c_int32), ("fail_chain_phase1", C.c_int32), ("blocked_no_bound", C.c_int32), ("lookback_spins", C.c_int32), ("base_error_strip", C.c_int32),
                ("skip_publish_strip", C.c_int32), ("blocked_no_order", C.c_int32), ("blocked_no_vec_store", C.c_int32), ("resize_tile_pixels", C.c_int32)]


def load_library(path=None):
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise LimgHipError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). There is no CPU fallback." % path)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; if liblimg_hip.so pulled
    # in /opt/rocm's copy first, torch's later initialisation would find "no HIP GPUs".  Importing torch first makes the
    # loader resolve our DT_NEEDED libamdhip64.so.7 to the already-loaded copy (same SONAME).  C/C++ users are unaffected.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.limg_hip_version.restype = C.c_char_p
    L.limg_hip_init.restype = C.c_int
    L.limg_hip_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.limg_hip_shutdown.argtypes = [C.POINTER(C.c_void_p)]
    L.limg_hip_default_options_sized.argtypes = [C.c_void_p, C.c_size_t]
    if hasattr(L, "limg_hip_set_test_options"):
        L.limg_hip_default_test_options_sized.argtypes = [C.c_void_p, C.c_size_t]
        L.limg_hip_set_test_options.restype = C.c_int
        L.limg_hip_set_test_options.argtypes = [C.c_void_p, C.c_void_p]
        L.limg_hip_test_live_resources.restype = None
        L.limg_hip_test_live_resources.argtypes = [C.POINTER(C.c_uint64)]
    L.limg_hip_set_options.restype = C.c_int
    L.limg_hip_set_options.argtypes = [C.c_void_p, C.c_void_p]
    L.limg_hip_get_options.restype = C.c_int
    L.limg_hip_get_options.argtypes = [C.c_void_p, C.c_void_p]
    L.limg_hip_encode3d_stats.restype = C.c_int
    L.limg_hip_encode3d_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_blocked_encode3d_stats.restype = C.c_int
    L.limg_hip_blocked_encode3d_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_encode3d.restype = C.c_int
    L.limg_hip_encode3d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    L.limg_hip_encode3d_perf.restype = C.c_int
    L.limg_hip_encode3d_perf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_int, C.c_int]
    L.limg_hip_encode3d_device.restype = C.c_int
    L.limg_hip_encode3d_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_encode3d_batch_device.restype = C.c_int
    L.limg_hip_encode3d_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_compare.restype = C.c_double
    L.limg_hip_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_compare_device.restype = C.c_double
    L.limg_hip_compare_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.limg_hip_synth_random_gradient_device.restype = C.c_int
    L.limg_hip_synth_random_gradient_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_int, C.c_size_t, C.c_void_p]
    L.limg_hip_synth_photo_noise_device.restype = C.c_int
    L.limg_hip_synth_photo_noise_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_size_t, C.c_void_p]
    L.limg_hip_profile_begin.restype = C.c_int
    L.limg_hip_profile_begin.argtypes = [C.c_void_p]
    L.limg_hip_profile_end.restype = C.c_int
    L.limg_hip_profile_end.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.limg_hip_check_device_status.restype = C.c_int
    L.limg_hip_check_device_status.argtypes = [C.c_void_p]
    L.limg_hip_host_noise_table.restype = C.c_int
    L.limg_hip_host_noise_table.argtypes = [C.c_void_p, C.c_size_t]
    L.limg_hip_last_stats.restype = C.c_int
    L.limg_hip_last_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.limg_hip_noise_table_device.restype = C.c_int
    L.limg_hip_noise_table_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.limg_hip_host_chain_call.restype = C.c_uint64
    L.limg_hip_host_chain_call.argtypes = [C.c_uint64, C.c_size_t, C.c_void_p, C.c_int]
    L.limg_hip_host_chain_checkpoints.restype = C.c_uint64
    L.limg_hip_host_chain_checkpoints.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]
    L.limg_hip_host_dense_checkpoints.restype = C.c_int
    L.limg_hip_host_dense_checkpoints.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p]
    L.limg_hip_host_accurate_table.restype = C.c_int
    L.limg_hip_host_accurate_table.argtypes = [C.c_void_p, C.c_size_t]
    L.limg_hip_host_partition.restype = C.c_int
    L.limg_hip_host_partition.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.limg_hip_context_device_bytes.restype = C.c_size_t
    L.limg_hip_context_device_bytes.argtypes = [C.c_void_p]
    L.limg_hip_blocked_encode3d.restype = C.c_int
    L.limg_hip_blocked_encode3d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int]
    L.limg_hip_blocked_encode3d_device.restype = C.c_int
    L.limg_hip_blocked_encode3d_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.limg_hip_blocked_regions.restype = C.c_int
    L.limg_hip_blocked_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.limg_hip_blocked_timing.restype = C.c_int
    L.limg_hip_blocked_timing.argtypes = [C.c_void_p, C.c_void_p]
    L.limg_hip_blocked_match_bits.restype = C.c_int
    L.limg_hip_blocked_match_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.limg_hip_blocked_kernel_timing.restype = C.c_int
    L.limg_hip_blocked_kernel_timing.argtypes = [C.c_void_p, C.c_void_p]
    L.limg_hip_host_blocked_matches.restype = C.c_int
    L.limg_hip_host_blocked_matches.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_host_blocked_merge.restype = C.c_int
    L.limg_hip_host_blocked_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.limg_hip_host_blocked_match_words.restype = C.c_size_t
    L.limg_hip_host_blocked_match_bits.restype = C.c_int
    L.limg_hip_host_blocked_match_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    L.limg_hip_stream_bound.restype = C.c_size_t
    L.limg_hip_stream_bound.argtypes = [C.c_size_t, C.c_size_t]
    L.limg_hip_encode_stream_device.restype = C.c_int
    L.limg_hip_encode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint32, C.c_int, C.c_int,
                                                C.c_void_p]
    L.limg_hip_decode_stream_device.restype = C.c_int
    L.limg_hip_decode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.limg_hip_encode_stream.restype = C.c_int
    L.limg_hip_encode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint32, C.c_int, C.c_int]
    L.limg_hip_decode_stream.restype = C.c_int
    L.limg_hip_decode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.limg_hip_stream_info.restype = C.c_int
    L.limg_hip_stream_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.limg_hip_encode_stream_batch_device.restype = C.c_int  # ctx, count, ins (host array), sizeX, sizeY, hasAlpha, streams (host array), capacityEach, sizes, ef, pool, fast, hipStream
    L.limg_hip_encode_stream_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int,
                                                      C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_batch.restype = C.c_int
    L.limg_hip_encode_stream_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    L.limg_hip_encode_stream_batch_ef_device.restype = C.c_int  # as limg_hip_encode_stream_batch_device, ef: host array of `count` uint32
    L.limg_hip_encode_stream_batch_ef_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_batch_ef.restype = C.c_int
    L.limg_hip_encode_stream_batch_ef.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.limg_hip_stream_sizes_device.restype = C.c_int  # ctx, in, sizeX, sizeY, hasAlpha, error factors (host), count, sizes (host), pool, fast, hipStream
    L.limg_hip_stream_sizes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_stream_sizes.restype = C.c_int
    L.limg_hip_stream_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.limg_hip_encode_stream_budget_device.restype = C.c_int  # ctx, in, sizeX, sizeY, hasAlpha, stream, capacity, maxBytes, min ef, max ef, pool, fast, result, hipStream
    L.limg_hip_encode_stream_budget_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int,
                                                       C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_encode_stream_budget.restype = C.c_int
    L.limg_hip_encode_stream_budget.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                                C.c_void_p]
    L.limg_hip_encode_stream_budget_batch_device.restype = C.c_int  # ctx, count, ins, sizeX, sizeY, hasAlpha, streams, capacityEach, budgets (host), min ef, max ef, pool, fast, results, hipStream
    L.limg_hip_encode_stream_budget_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                                             C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_encode_stream_budget_batch.restype = C.c_int
    L.limg_hip_encode_stream_budget_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32,
                                                      C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_quality_device.restype = C.c_int  # ctx, in, sizeX, sizeY, hasAlpha, stream, capacity, maxErrorSum, min ef, max ef, pool, fast, result, hipStream
    L.limg_hip_encode_stream_quality_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                                                        C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_encode_stream_quality.restype = C.c_int
    L.limg_hip_encode_stream_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                                 C.c_void_p]
    L.limg_hip_encode_stream_quality_batch_device.restype = C.c_int  # ctx, count, ins, sizeX, sizeY, hasAlpha, streams, capacityEach, limits (host), min ef, max ef, pool, fast, results, hipStream
    L.limg_hip_encode_stream_quality_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                                              C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.limg_hip_encode_stream_quality_batch.restype = C.c_int
    L.limg_hip_encode_stream_quality_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32,
                                                       C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_list_device.restype = C.c_int  # ctx, count, items (host), itemSize, hasAlpha, bytes (host or NULL), pool, fast, hipStream
    L.limg_hip_encode_stream_list_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_list.restype = C.c_int
    L.limg_hip_encode_stream_list.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.limg_hip_encode_stream_quality_list_device.restype = C.c_int  # ctx, count, items, itemSize, hasAlpha, limits (host), min ef, max ef, pool, fast, results, hipStream
    L.limg_hip_encode_stream_quality_list_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                             C.c_void_p]
    L.limg_hip_encode_stream_quality_list.restype = C.c_int
    L.limg_hip_encode_stream_quality_list.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_encode_stream_budget_list_device.restype = C.c_int  # ctx, count, items, itemSize, hasAlpha, budgets (host), min ef, max ef, pool, fast, results, hipStream
    L.limg_hip_encode_stream_budget_list_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                            C.c_void_p]
    L.limg_hip_encode_stream_budget_list.restype = C.c_int
    L.limg_hip_encode_stream_budget_list.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_stream_sizes_list_device.restype = C.c_int  # ctx, count, items, itemSize, hasAlpha, error factors (host), factorCount, sizes (host), pool, fast, hipStream
    L.limg_hip_stream_sizes_list_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.limg_hip_stream_sizes_list.restype = C.c_int
    L.limg_hip_stream_sizes_list.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.limg_hip_stream_compare.restype = C.c_double  # ctx, stream, bytes, original, pixels, mse, max
    L.limg_hip_stream_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.limg_hip_error_sum_for_psnr.restype = C.c_uint64
    L.limg_hip_error_sum_for_psnr.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_double]
    L.limg_hip_blocked_stream_bound.restype = C.c_size_t
    L.limg_hip_blocked_stream_bound.argtypes = [C.c_size_t, C.c_size_t]
    L.limg_hip_blocked_encode_stream_device.restype = C.c_int
    L.limg_hip_blocked_encode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint32, C.c_int,
                                                        C.c_void_p]
    L.limg_hip_blocked_decode_stream_device.restype = C.c_int
    L.limg_hip_blocked_decode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.limg_hip_blocked_encode_stream.restype = C.c_int
    L.limg_hip_blocked_encode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint32, C.c_int]
    L.limg_hip_blocked_decode_stream.restype = C.c_int
    L.limg_hip_blocked_decode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    P, Z = C.c_void_p, C.c_size_t
    for args, names in (  # the window entries, limg_hip_[blocked_]decode_stream_<name>: both versions of a name share its argument list
            ([P, P, Z] + [Z] * 6 + [P, Z, P], ("window_device",)),  # ctx, stream, bytes, sizeX, sizeY, x0, y0, width, height, out, outStridePixels, hipStream
            ([P, P, Z] + [Z] * 4 + [P, Z], ("window",)),  # ctx, stream, bytes, x0, y0, width, height, out, outStridePixels
            ([P, P, Z, P, P], ("windows_device", "windows_scaled_device", "windows_resized_device")),  # ctx, jobs (host), count, jobStatus (device), hipStream
            ([P, P, Z, P, Z], ("windows", "windows_scaled", "windows_resized")),  # ctx, stream, bytes, windows (host), count
            ([P, P, Z, P, P, P], ("windows_error_device",)),  # ctx, jobs (host), count, errorSums (device), jobStatus (device), hipStream
            ([P, P, Z, P, Z, P], ("windows_error",)),  # ctx, stream, bytes, windows (host), count, errorSums (host)
            ([P, P, Z, P, P, P], ("windows_tensor_device", "windows_scaled_tensor_device", "windows_resized_tensor_device")),  # ctx, jobs (host), count, format (host), jobStatus (device), hipStream
            ([P, P, Z, P, Z, P], ("windows_tensor", "windows_scaled_tensor", "windows_resized_tensor"))):  # ctx, stream, bytes, windows (host), count, format (host)
        for name in names:
            for version in ("limg_hip_decode_stream_", "limg_hip_blocked_decode_stream_"):
                getattr(L, version + name).restype = C.c_int
                getattr(L, version + name).argtypes = args
    L.limg_hip_blocked_last_stream.restype = C.c_int
    L.limg_hip_blocked_last_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.limg_hip_blocked_stream_info.restype = C.c_int
    L.limg_hip_blocked_stream_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    L.limg_hip_comm_unique_id.restype = C.c_int
    L.limg_hip_comm_unique_id.argtypes = [C.c_void_p]
    L.limg_hip_comm_init.restype = C.c_int
    L.limg_hip_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.limg_hip_comm_info.restype = C.c_int
    L.limg_hip_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.limg_hip_comm_destroy.restype = C.c_int
    L.limg_hip_comm_destroy.argtypes = [C.c_void_p]
    L.limg_hip_gather_stream.restype = C.c_int
    L.limg_hip_gather_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.limg_hip_encode3d_single_chain_device.restype = C.c_int
    L.limg_hip_encode3d_single_chain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_void_p]
    L.limg_hip_encode3d_chain_device.restype = C.c_int
    L.limg_hip_encode3d_chain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                 C.c_void_p]
    L.limg_hip_host_gather_offsets.restype = C.c_int
    L.limg_hip_host_gather_offsets.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.limg_hip_host_chain_bases.restype = C.c_int
    L.limg_hip_host_chain_bases.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    # ctx, pieces (host array), count, pieceSize, sizeX, sizeY, hasAlpha, errorFactor, flags, out, capacity, bytes[, hipStream]
    L.limg_hip_stream_splice_device.restype = C.c_int
    L.limg_hip_stream_splice_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                                C.POINTER(C.c_size_t), C.c_void_p]
    L.limg_hip_stream_splice.restype = C.c_int
    L.limg_hip_stream_splice.argtypes = L.limg_hip_stream_splice_device.argtypes[:-1]
    # ctx, stream, streamBytes, sizeX, sizeY, hasAlpha, x0, y0, width, height, errorFactor, flags, out, capacity, bytes, hipStream
    L.limg_hip_stream_crop_device.restype = C.c_int
    L.limg_hip_stream_crop_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.limg_hip_stream_crop.restype = C.c_int
    L.limg_hip_stream_crop.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    return L


def _check(r, what):
    if r != 0:
        raise LimgHipError("%s failed with limg_hip_result %d" % (what, r))


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def live_resources(lib):
    """(device buffers, device bytes, pinned buffers, streams, events) that the contexts opened through `lib` hold right now.  Test build only (include/limg_hip_test_hooks.h)."""
    out = (C.c_uint64 * 5)()
    lib.limg_hip_test_live_resources(out)
    return tuple(int(v) for v in out)


def stream_info(stream, lib=None):
    """(sizeX, sizeY, hasAlpha, totalBytes) of a stream held in a numpy uint8 array (host-only, no GPU touched)."""
    lib = lib or load_library()
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    sx, sy, tb, ha = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    _check(lib.limg_hip_stream_info(_np_ptr(stream), stream.size, C.byref(sx), C.byref(sy), C.byref(ha), C.byref(tb)), "limg_hip_stream_info")
    return sx.value, sy.value, bool(ha.value), tb.value


def blocked_stream_bound(w, h, lib=None):
    """Worst-case size of a version 2 (merged-block) stream; host only."""
    return (lib or load_library()).limg_hip_blocked_stream_bound(w, h)


def blocked_stream_info(stream, lib=None):
    """(sizeX, sizeY, hasAlpha, totalBytes, rectangles) of a version 2 (merged-block) stream held in a numpy uint8 array (host-only, no GPU touched)."""
    lib = lib or load_library()
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    sx, sy, tb, nr, ha = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    _check(lib.limg_hip_blocked_stream_info(_np_ptr(stream), stream.size, C.byref(sx), C.byref(sy), C.byref(ha), C.byref(tb), C.byref(nr)), "limg_hip_blocked_stream_info")
    return sx.value, sy.value, bool(ha.value), tb.value, nr.value


def host_gather_offsets(sizes, lib=None):
    """Offsets (len + 1 entries, the last is the total) of the variable-size stream gather; host only."""
    lib = lib or load_library()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    out = np.zeros(sizes.size + 1, dtype=np.uint64)
    _check(lib.limg_hip_host_gather_offsets(_np_ptr(sizes), sizes.size, _np_ptr(out)), "limg_hip_host_gather_offsets")
    return out


def host_chain_bases(calls, lib=None):
    """Every rank's first dither-call index in a chain that runs through all strips in rank order; host only."""
    lib = lib or load_library()
    calls = np.ascontiguousarray(calls, dtype=np.uint64)
    out = np.zeros(calls.size, dtype=np.uint64)
    _check(lib.limg_hip_host_chain_bases(_np_ptr(calls), calls.size, _np_ptr(out)), "limg_hip_host_chain_bases")
    return out


def host_accurate_table(states, lib=None):
    """The accurate shift search's automaton as a context uploads it: (states, 8) uint32, `states` = LIMG_SEARCH_ACC_STATES (the library refuses any other size);
    host only."""
    lib = lib or load_library()
    out = np.zeros((states, 8), dtype=np.uint32)
    _check(lib.limg_hip_host_accurate_table(_np_ptr(out), out.size), "limg_hip_host_accurate_table")
    return out


def host_blocked_matches(channels, seed, cand, lib=None):
    """The similarity predicate as the host merge evaluates it (records: numpy RECORD_DTYPE items); no GPU touched."""
    lib = lib or load_library()
    a = np.ascontiguousarray(seed); b = np.ascontiguousarray(cand)
    return bool(lib.limg_hip_host_blocked_matches(channels, _np_ptr(a), _np_ptr(b)))


def host_blocked_merge(fits, channels, use_bits=True, lib=None):
    """fits: (by, bx) array of RECORD_DTYPE -> rectangles (REGION_DTYPE) in creation order; host only.  use_bits: go through the precomputed
    similarity-bit window (as the GPU pipeline does) instead of evaluating every pair on demand."""
    lib = lib or load_library()
    fits = np.ascontiguousarray(fits)
    by, bx = fits.shape
    bits = None
    if use_bits:
        bits = np.zeros(by * bx * lib.limg_hip_host_blocked_match_words(), dtype=np.uint64)
        _check(lib.limg_hip_host_blocked_match_bits(_np_ptr(fits), bx, by, channels, _np_ptr(bits)), "limg_hip_host_blocked_match_bits")
    out = np.zeros(by * bx, dtype=REGION_DTYPE)
    n = C.c_size_t(0)
    _check(lib.limg_hip_host_blocked_merge(_np_ptr(fits), _np_ptr(bits) if bits is not None else None, bx, by, channels, _np_ptr(out), out.size, C.byref(n)), "limg_hip_host_blocked_merge")
    return out[:n.value].copy()


class LimgHip:
    """One context on one GPU.  Host-array methods mirror the reference API (src/limg.h:35,37,48); *_device methods take
    torch CUDA tensors (used only as device memory) and run asynchronously on torch's current stream."""

    def __init__(self, device=-1, lib_path=None):
        self.lib = load_library(lib_path)
        self.ctx = C.c_void_p()
        self.comm_rank, self.comm_world = 0, 1
        _check(self.lib.limg_hip_init(device, C.byref(self.ctx)), "limg_hip_init")

    def close(self):
        if self.ctx:
            self.lib.limg_hip_shutdown(C.byref(self.ctx))
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, forced_shift=None, force_split=False, dither_pcg=False, float_fast=False, legacy_float_stage=False, host_noise_table=False, collect_stats=False,
                    batch_sub_images=0, ragged_bands=0, ragged_walk_threads=0, **test_hooks):
        """Every call sets ALL options (unnamed ones to their defaults).  Keywords starting with `test_` are the hooks of include/limg_hip_test_hooks.h
        (test_base_error_strip=N -> limg_hip_test_options.base_error_strip): they need liblimg_hip_test.so and raise on the product library."""
        o = Options()
        self.lib.limg_hip_default_options_sized(C.byref(o), C.sizeof(o))
        if forced_shift is not None:
            for i in range(3):
                o.forced_shift[i] = int(forced_shift[i])
        o.force_split_kernels = int(force_split)
        o.dither_pcg = int(dither_pcg)
        o.float_mode = 1 if float_fast else 0
        o.legacy_float_stage = int(legacy_float_stage)
        o.host_noise_table = int(host_noise_table)
        o.collect_stats = int(collect_stats)
        o.batch_sub_images = int(batch_sub_images)
        o.ragged_bands = int(ragged_bands)
        o.ragged_walk_threads = int(ragged_walk_threads)
        _check(self.lib.limg_hip_set_options(self.ctx, C.byref(o)), "limg_hip_set_options")
        hooks = {}
        for k, v in test_hooks.items():
            if not k.startswith("test_") or k[5:] not in dict(TestOptions._fields_):
                raise TypeError("set_options: unknown option %r" % k)
            hooks[k[5:]] = int(v)
        if self.has_test_hooks:
            t = TestOptions()
            self.lib.limg_hip_default_test_options_sized(C.byref(t), C.sizeof(t))
            for k, v in hooks.items():
                setattr(t, k, v)
            _check(self.lib.limg_hip_set_test_options(self.ctx, C.byref(t)), "limg_hip_set_test_options")
        elif any(hooks.values()):
            raise LimgHipError("test hooks %s need liblimg_hip_test.so (LIMG_HIP_LIB=test); the product library has none" % sorted(k for k, v in hooks.items() if v))

    @property
    def has_test_hooks(self):
        return hasattr(self.lib, "limg_hip_set_test_options")

    def get_options(self):
        o = Options()
        o.struct_size = C.sizeof(o)
        _check(self.lib.limg_hip_get_options(self.ctx, C.byref(o)), "limg_hip_get_options")
        return o

    def set_forced_shift(self, shift=None):
        self.set_options(forced_shift=shift)

    # ---- host pointers (drop-in for limg_encode3d_test / _perf / limg_compare) ---------------------------------------------
    def encode3d(self, img, has_alpha, error_factor=100, pool_threads=0, fast=True):
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = {k: np.zeros((h, w), dtype=np.uint32) for k in P32}
        out.update({k: np.zeros((h, w), dtype=np.uint8) for k in P8})
        info = Info(*[out[k].ctypes.data for k in PLANES])
        _check(self.lib.limg_hip_encode3d(self.ctx, _np_ptr(img), w, h, int(has_alpha), C.byref(info), error_factor, pool_threads, int(fast)), "limg_hip_encode3d")
        return out

    def encode3d_stats(self, img, has_alpha, error_factor=100, pool_threads=0, fast=True):
        """limg_hip_encode3d_stats: the planes AND the bit counters of this very encode -> (planes, counters[30], pixels)"""
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = {k: np.zeros((h, w), dtype=np.uint32) for k in P32}
        out.update({k: np.zeros((h, w), dtype=np.uint8) for k in P8})
        info = Info(*[out[k].ctypes.data for k in PLANES])
        cnt = np.zeros(30, dtype=np.uint64)
        px = C.c_uint64(0)
        _check(self.lib.limg_hip_encode3d_stats(self.ctx, _np_ptr(img), w, h, int(has_alpha), C.byref(info), error_factor, pool_threads, int(fast), _np_ptr(cnt), C.byref(px)),
               "limg_hip_encode3d_stats")
        return out, cnt, px.value

    def encode3d_perf(self, img, has_alpha, error_factor=100, pool_threads=0, fast=True):
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        _check(self.lib.limg_hip_encode3d_perf(self.ctx, _np_ptr(img), w, h, int(has_alpha), error_factor, pool_threads, int(fast)), "limg_hip_encode3d_perf")

    def compare(self, a, b, has_alpha):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        mse, mx = C.c_double(), C.c_double()
        p = self.lib.limg_hip_compare(self.ctx, _np_ptr(a), _np_ptr(b), a.shape[1], a.shape[0], int(has_alpha), C.byref(mse), C.byref(mx))
        return p, mse.value

    # ---- device pointers ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def alloc_planes_device(self, w, h, device="cuda"):
        import torch
        d = {k: torch.empty((h, w), dtype=torch.int32, device=device) for k in P32}
        d.update({k: torch.empty((h, w), dtype=torch.uint8, device=device) for k in P8})
        return d

    def encode3d_device(self, img, has_alpha, planes=None, error_factor=100, pool_threads=0, fast=True, records=None, shifts=None):
        """img: torch int32 CUDA tensor (h, w); planes: dict from alloc_planes_device or None (`_perf` behaviour)."""
        h, w = img.shape
        info = None
        if planes is not None:
            info = Info(*[(planes[k].data_ptr() if k in planes else None) for k in PLANES])  # compact mode: only the factor planes
        comp = None
        if records is not None or shifts is not None:
            comp = CompactOut(records.data_ptr() if records is not None else None, shifts.data_ptr() if shifts is not None else None)
        _check(self.lib.limg_hip_encode3d_device(self.ctx, C.c_void_p(img.data_ptr()), w, h, int(has_alpha), C.byref(info) if info else None,
                                                 C.byref(comp) if comp else None, error_factor, pool_threads, int(fast), self._stream()), "limg_hip_encode3d_device")

    def encode3d_batch_device(self, imgs, has_alpha, planes_list, error_factor=100, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors of one shape; planes_list: one alloc_planes_device dict per image.  One launch pair for the whole list."""
        n = len(imgs)
        h, w = imgs[0].shape
        assert all(tuple(i.shape) == (h, w) for i in imgs) and len(planes_list) == n
        ins = (C.c_void_p * n)(*[i.data_ptr() for i in imgs])
        infos = (Info * n)(*[Info(*[(pl[k].data_ptr() if k in pl else None) for k in PLANES]) for pl in planes_list])
        _check(self.lib.limg_hip_encode3d_batch_device(self.ctx, n, ins, w, h, int(has_alpha), infos, error_factor, pool_threads, int(fast), self._stream()),
               "limg_hip_encode3d_batch_device")

    def last_stats(self):
        """(counters[30], pixels) of the last encode made with set_options(collect_stats=True): the reference's "Average Block Bits" counters (src/limg.cpp:1971-1999)."""
        out = np.zeros(30, dtype=np.uint64)
        px = C.c_uint64(0)
        _check(self.lib.limg_hip_last_stats(self.ctx, _np_ptr(out), C.byref(px)), "limg_hip_last_stats")
        return out, px.value

    def compare_device(self, a, b, has_alpha):
        mse, mx = C.c_double(), C.c_double()
        h, w = a.shape
        p = self.lib.limg_hip_compare_device(self.ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), w, h, int(has_alpha), C.byref(mse), C.byref(mx), self._stream())
        return p, mse.value

    def synth_device(self, kind, w, h, seed=1, opaque=True, y0=0, device="cuda"):
        import torch
        out = torch.empty((h, w), dtype=torch.int32, device=device)
        if kind == "random_gradient":
            _check(self.lib.limg_hip_synth_random_gradient_device(C.c_void_p(out.data_ptr()), w, h, seed, int(opaque), y0, self._stream()), "synth")
        elif kind == "photo_noise":
            _check(self.lib.limg_hip_synth_photo_noise_device(C.c_void_p(out.data_ptr()), w, h, seed, y0, self._stream()), "synth")
        else:
            raise ValueError(kind)
        return out

    # ---- merged-block encoder (limg_blocked_encode3d_test) --------------------------------------------------------------------------
    def blocked_encode3d(self, img, has_alpha, error_factor=100, fast=True):
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = {k: np.zeros((h, w), dtype=t) for k, t in BLOCKED_PLANES}
        info = (C.c_void_p * 14)(*[out[k].ctypes.data for k, _ in BLOCKED_PLANES])
        _check(self.lib.limg_hip_blocked_encode3d(self.ctx, _np_ptr(img), w, h, int(has_alpha), info, error_factor, int(fast)), "limg_hip_blocked_encode3d")
        out["regions"] = self.blocked_regions()
        return out

    def blocked_encode3d_device(self, img, has_alpha, planes, error_factor=100, fast=True):
        """img: torch int32 CUDA (h, w); planes: dict name -> torch CUDA tensor for every BLOCKED_PLANES name except pBlockError."""
        h, w = img.shape
        info = (C.c_void_p * 14)(*[(planes[k].data_ptr() if k in planes else None) for k, _ in BLOCKED_PLANES])
        _check(self.lib.limg_hip_blocked_encode3d_device(self.ctx, C.c_void_p(img.data_ptr()), w, h, int(has_alpha), info, error_factor, int(fast), self._stream()),
               "limg_hip_blocked_encode3d_device")

    def alloc_blocked_planes_device(self, w, h, device="cuda"):
        import torch
        return {k: torch.empty((h, w), dtype=(torch.int32 if t == np.uint32 else torch.uint8), device=device) for k, t in BLOCKED_PLANES if k != "pBlockError"}

    def blocked_regions(self):
        n = C.c_size_t(0)
        _check(self.lib.limg_hip_blocked_regions(self.ctx, None, 0, C.byref(n)), "limg_hip_blocked_regions")
        out = np.zeros(n.value, dtype=REGION_DTYPE)
        _check(self.lib.limg_hip_blocked_regions(self.ctx, _np_ptr(out), out.size, C.byref(n)), "limg_hip_blocked_regions")
        return out

    def blocked_timing(self):
        ms = np.zeros(6, dtype=np.float64)
        _check(self.lib.limg_hip_blocked_timing(self.ctx, _np_ptr(ms)), "limg_hip_blocked_timing")
        return dict(zip(("pass1_match_gpu", "merge_host", "fit_search_gpu", "chain_host", "store_gpu", "total"), ms.tolist()))

    def blocked_match_bits(self):
        """The similarity bits (uint64 words, host_blocked_merge's layout) the last merged-block encode's merge worked from."""
        n = C.c_size_t(0)
        _check(self.lib.limg_hip_blocked_match_bits(self.ctx, None, 0, C.byref(n)), "limg_hip_blocked_match_bits")
        out = np.zeros(n.value, dtype=np.uint64)
        _check(self.lib.limg_hip_blocked_match_bits(self.ctx, _np_ptr(out), out.size, C.byref(n)), "limg_hip_blocked_match_bits")
        return out

    def blocked_kernel_timing(self):
        """GPU milliseconds (HIP events) of the last merged-block encode's launches: pass 1, similarity kernels, and -- summed over the worker's batches -- the
        per-rectangle fit + search kernel and the expansion + store kernels."""
        ms = np.zeros(4, dtype=np.float64)
        _check(self.lib.limg_hip_blocked_kernel_timing(self.ctx, _np_ptr(ms)), "limg_hip_blocked_kernel_timing")
        return dict(zip(("pass1_kernel", "match_kernels", "fit_search_kernel", "expand_store_kernels"), ms.tolist()))

    # ---- compact stream ("limg_encode" / "limg_decode"): version 1 (8x8 blocks) and version 2 (what the merged-block encoder produced) ----------------
    # The two versions' entries take the same arguments but for pool_threads (version 1 only): `name` is the entry, `opts` its arguments after the size pointer.
    def _stream_call(self, name, *args):
        _check(getattr(self.lib, name)(self.ctx, *args), name)

    def _encode_stream(self, name, cap, img, has_alpha, opts):
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = np.zeros(cap(w, h), dtype=np.uint8)
        n = C.c_size_t(0)
        self._stream_call(name, _np_ptr(img), w, h, int(has_alpha), _np_ptr(out), out.size, C.byref(n), *opts)
        return out[:n.value].copy()

    def _decode_stream(self, name, stream, w, h):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        out = np.zeros((h, w), dtype=np.uint32)
        self._stream_call(name, _np_ptr(stream), stream.size, _np_ptr(out), out.size)
        return out

    def _encode_stream_device(self, name, cap, img, has_alpha, out, want_size, opts):
        import torch
        h, w = img.shape
        if out is None:
            out = torch.empty(cap(w, h), dtype=torch.uint8, device=img.device)
        n = C.c_size_t(0)
        self._stream_call(name, C.c_void_p(img.data_ptr()), w, h, int(has_alpha), C.c_void_p(out.data_ptr()), out.numel(), C.byref(n) if want_size else None, *opts, self._stream())
        return out, (n.value if want_size else None)

    def _decode_stream_device(self, name, stream, nbytes, w, h, out):
        import torch
        if out is None:
            out = torch.empty((h, w), dtype=torch.int32, device=stream.device)
        self._stream_call(name, C.c_void_p(stream.data_ptr()), int(nbytes), C.c_void_p(out.data_ptr()), w, h, self._stream())
        return out

    def stream_bound(self, w, h):
        return self.lib.limg_hip_stream_bound(w, h)

    def encode_stream(self, img, has_alpha, error_factor=100, pool_threads=0, fast=True):
        """host uint32 image -> stream bytes (numpy uint8)"""
        return self._encode_stream("limg_hip_encode_stream", self.stream_bound, img, has_alpha, (error_factor, pool_threads, int(fast)))

    def decode_stream(self, stream):
        w, h, _, _ = stream_info(stream, self.lib)
        return self._decode_stream("limg_hip_decode_stream", stream, w, h)

    def encode_stream_device(self, img, has_alpha, out=None, error_factor=100, pool_threads=0, fast=True, want_size=True):
        """img: torch int32 CUDA (h, w) -> (torch uint8 CUDA stream buffer of worst-case size, bytes used or None)"""
        return self._encode_stream_device("limg_hip_encode_stream_device", self.stream_bound, img, has_alpha, out, want_size, (error_factor, pool_threads, int(fast)))

    def decode_stream_device(self, stream, nbytes, w, h, out=None):
        return self._decode_stream_device("limg_hip_decode_stream_device", stream, nbytes, w, h, out)

    # ---- stream sizes and the encode to a byte budget (contract: include/limg_hip.h) ----
    def stream_sizes(self, img, has_alpha, error_factors, pool_threads=0, fast=True):
        """host uint32 image -> [len(encode_stream(img, ..., error_factor=ef)) for ef in error_factors], without encoding"""
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        n = len(error_factors)
        efs, sizes = (C.c_uint32 * max(n, 1))(*error_factors), (C.c_size_t * max(n, 1))()
        self._stream_call("limg_hip_stream_sizes", _np_ptr(img), w, h, int(has_alpha), efs, n, sizes, pool_threads, int(fast))
        return [int(v) for v in sizes[:n]]

    def stream_sizes_device(self, img, has_alpha, error_factors, pool_threads=0, fast=True):
        """img: torch int32 CUDA (h, w); waits for torch's current stream"""
        h, w = img.shape
        n = len(error_factors)
        efs, sizes = (C.c_uint32 * max(n, 1))(*error_factors), (C.c_size_t * max(n, 1))()
        self._stream_call("limg_hip_stream_sizes_device", C.c_void_p(img.data_ptr()), w, h, int(has_alpha), efs, n, sizes, pool_threads, int(fast), self._stream())
        return [int(v) for v in sizes[:n]]

    def encode_stream_budget(self, img, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True):
        """host uint32 image -> (stream bytes (numpy uint8), BudgetResult): the stream of encode_stream at the error factor the search chose for max_bytes"""
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = np.zeros(self.stream_bound(w, h), dtype=np.uint8)
        res = BudgetResult(C.sizeof(BudgetResult))
        self._stream_call("limg_hip_encode_stream_budget", _np_ptr(img), w, h, int(has_alpha), _np_ptr(out), out.size, int(max_bytes), min_error_factor, max_error_factor,
                          pool_threads, int(fast), C.byref(res))
        return out[:res.bytes].copy(), res

    def encode_stream_budget_device(self, img, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, out=None, pool_threads=0, fast=True):
        """img: torch int32 CUDA (h, w) -> (torch uint8 CUDA stream buffer of worst-case size, BudgetResult); waits for torch's current stream"""
        import torch
        h, w = img.shape
        if out is None:
            out = torch.empty(self.stream_bound(w, h), dtype=torch.uint8, device=img.device)
        res = BudgetResult(C.sizeof(BudgetResult))
        self._stream_call("limg_hip_encode_stream_budget_device", C.c_void_p(img.data_ptr()), w, h, int(has_alpha), C.c_void_p(out.data_ptr()), out.numel(), int(max_bytes),
                          min_error_factor, max_error_factor, pool_threads, int(fast), C.byref(res), self._stream())
        return out, res

    # ---- the list entries of the stream encode family (contract: include/limg_hip.h) ----
    def _stream_list(self, name, imgs, has_alpha, outs, rest, device):
        """One call of list entry `name`: the pointer arrays of the images (device: torch int32 CUDA tensors, else host arrays) and of the stream buffers (`outs`, or made
        here at the worst-case size), the smallest buffer as the capacity, then the entry's own arguments `rest`.  An empty list is a call too, of 8 x 8 images.  -> outs"""
        if not device:
            imgs = [np.ascontiguousarray(i, dtype=np.uint32) for i in imgs]
        n = len(imgs)
        h, w = tuple(imgs[0].shape) if n else (8, 8)
        assert all(tuple(i.shape) == (h, w) for i in imgs)
        bound = self.stream_bound(w, h)
        if outs is None and device:
            import torch
            outs = [torch.empty(bound, dtype=torch.uint8, device=imgs[0].device) for _ in range(n)]
        elif outs is None:
            outs = [np.zeros(bound, dtype=np.uint8) for _ in range(n)]
        assert len(outs) == n
        ptr = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
        cap = min([o.numel() if device else o.size for o in outs], default=bound)
        self._stream_call(name, n, (C.c_void_p * max(n, 1))(*map(ptr, imgs)), w, h, int(has_alpha), (C.c_void_p * max(n, 1))(*map(ptr, outs)), cap, *rest,
                          *([self._stream()] if device else []))
        return outs

    # ---- batched stream encode: a list of same-shape images, stream i = encode_stream of image i ----
    def encode_stream_batch(self, imgs, has_alpha, error_factor=100, pool_threads=0, fast=True):
        """host uint32 images of one shape -> list of stream bytes (numpy uint8), one batched call"""
        sizes = (C.c_size_t * max(len(imgs), 1))()
        outs = self._stream_list("limg_hip_encode_stream_batch", imgs, has_alpha, None, (sizes, error_factor, pool_threads, int(fast)), False)
        return [o[:sizes[k]].copy() for k, o in enumerate(outs)]

    def encode_stream_batch_device(self, imgs, has_alpha, outs=None, want_sizes=True, error_factor=100, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of one shape -> (list of torch uint8 CUDA stream buffers of worst-case size, list of bytes used or None).
        outs: the buffers to use (each at least stream_bound(w, h) bytes, the smallest is the capacity handed on).  Asynchronous on torch's current stream unless
        want_sizes."""
        sizes = (C.c_size_t * max(len(imgs), 1))()
        outs = self._stream_list("limg_hip_encode_stream_batch_device", imgs, has_alpha, outs, (sizes if want_sizes else None, error_factor, pool_threads, int(fast)), True)
        return outs, ([int(v) for v in sizes[:len(imgs)]] if want_sizes else None)

    # ---- ... each image at its own error factor: stream i = encode_stream of image i at error_factors[i] ----
    @staticmethod
    def _factor_list(error_factors, n):
        assert len(error_factors) == n
        return (C.c_uint32 * max(n, 1))(*[int(e) for e in error_factors])

    def encode_stream_batch_ef(self, imgs, has_alpha, error_factors, pool_threads=0, fast=True):
        """host uint32 images of one shape, one error factor per image -> list of stream bytes (numpy uint8), one batched call"""
        sizes = (C.c_size_t * max(len(imgs), 1))()
        outs = self._stream_list("limg_hip_encode_stream_batch_ef", imgs, has_alpha, None, (sizes, self._factor_list(error_factors, len(imgs)), pool_threads, int(fast)), False)
        return [o[:sizes[k]].copy() for k, o in enumerate(outs)]

    def encode_stream_batch_ef_device(self, imgs, has_alpha, error_factors, outs=None, want_sizes=True, pool_threads=0, fast=True):
        """encode_stream_batch_device with one error factor per image (error_factors: host sequence of len(imgs))"""
        sizes = (C.c_size_t * max(len(imgs), 1))()
        outs = self._stream_list("limg_hip_encode_stream_batch_ef_device", imgs, has_alpha, outs,
                                 (sizes if want_sizes else None, self._factor_list(error_factors, len(imgs)), pool_threads, int(fast)), True)
        return outs, ([int(v) for v in sizes[:len(imgs)]] if want_sizes else None)

    # ---- budgeted stream encode of a list: result i = encode_stream_budget of image i with its budget (contract: include/limg_hip.h) ----
    @staticmethod
    def _budget_list(max_bytes, n):
        budgets = [int(max_bytes)] * n if np.isscalar(max_bytes) else [int(b) for b in max_bytes]
        assert len(budgets) == n
        results = (BudgetResult * max(n, 1))()
        for r in results:
            r.struct_size = C.sizeof(BudgetResult)
        return (C.c_size_t * max(n, 1))(*budgets), results

    def encode_stream_budget_batch(self, imgs, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True):
        """host uint32 images of one shape, max_bytes an int or one per image -> (list of stream bytes (numpy uint8), list of BudgetResult), one batched call"""
        budgets, results = self._budget_list(max_bytes, len(imgs))
        outs = self._stream_list("limg_hip_encode_stream_budget_batch", imgs, has_alpha, None, (budgets, min_error_factor, max_error_factor, pool_threads, int(fast), results), False)
        return [o[:results[k].bytes].copy() for k, o in enumerate(outs)], results[:len(imgs)]

    def encode_stream_budget_batch_device(self, imgs, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, outs=None, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of one shape, max_bytes an int or one per image -> (list of torch uint8 CUDA stream buffers of worst-case size,
        list of BudgetResult).  outs: the buffers to use (each at least stream_bound(w, h) bytes).  Waits for torch's current stream."""
        budgets, results = self._budget_list(max_bytes, len(imgs))
        outs = self._stream_list("limg_hip_encode_stream_budget_batch_device", imgs, has_alpha, outs, (budgets, min_error_factor, max_error_factor, pool_threads, int(fast), results), True)
        return outs, results[:len(imgs)]

    # ---- stream encode to a quality target: the coarsest error factor the search finds whose error sum meets the limit (contract: include/limg_hip.h) ----
    def encode_stream_quality(self, img, has_alpha, max_error_sum, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True):
        """host uint32 image -> (stream bytes (numpy uint8), QualityResult): the stream of encode_stream at the error factor the search chose for max_error_sum"""
        img = np.ascontiguousarray(img, dtype=np.uint32)
        h, w = img.shape
        out = np.zeros(self.stream_bound(w, h), dtype=np.uint8)
        res = QualityResult(C.sizeof(QualityResult))
        self._stream_call("limg_hip_encode_stream_quality", _np_ptr(img), w, h, int(has_alpha), _np_ptr(out), out.size, int(max_error_sum), min_error_factor, max_error_factor,
                          pool_threads, int(fast), C.byref(res))
        return out[:res.bytes].copy(), res

    def encode_stream_quality_device(self, img, has_alpha, max_error_sum, min_error_factor=0, max_error_factor=0, out=None, pool_threads=0, fast=True):
        """img: torch int32 CUDA (h, w) -> (torch uint8 CUDA stream buffer of worst-case size, QualityResult); waits for torch's current stream once per probe"""
        import torch
        h, w = img.shape
        if out is None:
            out = torch.empty(self.stream_bound(w, h), dtype=torch.uint8, device=img.device)
        res = QualityResult(C.sizeof(QualityResult))
        self._stream_call("limg_hip_encode_stream_quality_device", C.c_void_p(img.data_ptr()), w, h, int(has_alpha), C.c_void_p(out.data_ptr()), out.numel(), int(max_error_sum),
                          min_error_factor, max_error_factor, pool_threads, int(fast), C.byref(res), self._stream())
        return out, res

    @staticmethod
    def _quality_list(max_error_sums, n):
        limits = [int(max_error_sums)] * n if np.isscalar(max_error_sums) else [int(b) for b in max_error_sums]
        assert len(limits) == n
        results = (QualityResult * max(n, 1))()
        for r in results:
            r.struct_size = C.sizeof(QualityResult)
        return (C.c_uint64 * max(n, 1))(*limits), results

    def encode_stream_quality_batch(self, imgs, has_alpha, max_error_sums, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True):
        """host uint32 images of one shape, max_error_sums an int or one per image -> (list of stream bytes (numpy uint8), list of QualityResult), one batched call"""
        limits, results = self._quality_list(max_error_sums, len(imgs))
        outs = self._stream_list("limg_hip_encode_stream_quality_batch", imgs, has_alpha, None, (limits, min_error_factor, max_error_factor, pool_threads, int(fast), results), False)
        return [o[:results[k].bytes].copy() for k, o in enumerate(outs)], results[:len(imgs)]

    def encode_stream_quality_batch_device(self, imgs, has_alpha, max_error_sums, min_error_factor=0, max_error_factor=0, outs=None, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of one shape, max_error_sums an int or one per image -> (list of torch uint8 CUDA stream buffers of worst-case
        size, list of QualityResult).  outs: the buffers to use (each at least stream_bound(w, h) bytes).  Waits for torch's current stream once per round."""
        limits, results = self._quality_list(max_error_sums, len(imgs))
        outs = self._stream_list("limg_hip_encode_stream_quality_batch_device", imgs, has_alpha, outs, (limits, min_error_factor, max_error_factor, pool_threads, int(fast), results), True)
        return outs, results[:len(imgs)]

    # ---- a list of MIXED shapes: stream i = encode_stream of image i at error_factors[i], the images that can share launches in one launch pair per chunk ----
    def _stream_items(self, imgs, error_factors, outs, device):
        """the item array of a mixed-shape list entry: images of any shapes (device: torch int32 CUDA tensors, else host arrays), the stream buffers (`outs`, or made
        here at each image's worst-case size) -> (imgs, outs, ctypes array of StreamListItem); all three must stay alive until the call has returned"""
        if not device:
            imgs = [np.ascontiguousarray(i, dtype=np.uint32) for i in imgs]
        n = len(imgs)
        efs = [int(error_factors)] * n if np.isscalar(error_factors) else [int(e) for e in error_factors]
        assert len(efs) == n
        if outs is None and device:
            import torch
            outs = [torch.empty(self.stream_bound(i.shape[1], i.shape[0]), dtype=torch.uint8, device=i.device) for i in imgs]
        elif outs is None:
            outs = [np.zeros(self.stream_bound(i.shape[1], i.shape[0]), dtype=np.uint8) for i in imgs]
        assert len(outs) == n
        ptr = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
        items = (StreamListItem * max(n, 1))()
        for k in range(n):
            items[k] = StreamListItem(ptr(imgs[k]), ptr(outs[k]), outs[k].numel() if device else outs[k].size, imgs[k].shape[1], imgs[k].shape[0], efs[k], 0)
        return imgs, outs, items

    def encode_stream_list(self, imgs, has_alpha, error_factors, pool_threads=0, fast=True):
        """host uint32 images of ANY shapes, one error factor per image (or one int for all) -> list of stream bytes (numpy uint8), one call"""
        imgs, outs, items = self._stream_items(imgs, error_factors, None, False)
        sizes = (C.c_size_t * max(len(imgs), 1))()
        self._stream_call("limg_hip_encode_stream_list", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), sizes, pool_threads, int(fast))
        return [o[:sizes[k]].copy() for k, o in enumerate(outs)]

    def encode_stream_list_device(self, imgs, has_alpha, error_factors, outs=None, want_sizes=True, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of ANY shapes -> (list of torch uint8 CUDA stream buffers, each of its image's worst-case size, list of bytes
        used or None).  outs: the buffers to use (each at least its image's stream_bound).  Asynchronous on torch's current stream unless want_sizes."""
        imgs, outs, items = self._stream_items(imgs, error_factors, outs, True)
        sizes = (C.c_size_t * max(len(imgs), 1))()
        self._stream_call("limg_hip_encode_stream_list_device", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), sizes if want_sizes else None, pool_threads, int(fast),
                          self._stream())
        return outs, ([int(v) for v in sizes[:len(imgs)]] if want_sizes else None)

    def _quality_limits(self, imgs, has_alpha, max_error_sums, min_psnr):
        """the limits of a mixed-shape quality list: max_error_sums (an int or one per image), or -- min_psnr, a float or one per image -- error_sum_for_psnr per image"""
        if min_psnr is None:
            return max_error_sums
        assert max_error_sums is None
        targets = [float(min_psnr)] * len(imgs) if np.isscalar(min_psnr) else [float(t) for t in min_psnr]
        assert len(targets) == len(imgs)
        return [self.error_sum_for_psnr(i.shape[1], i.shape[0], has_alpha, t) for i, t in zip(imgs, targets)]

    def encode_stream_quality_list(self, imgs, has_alpha, max_error_sums=None, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True, min_psnr=None):
        """host uint32 images of ANY shapes, max_error_sums an int or one per image (or min_psnr= in dB, through error_sum_for_psnr per image) -> (list of stream bytes
        (numpy uint8), list of QualityResult), one call"""
        limits, results = self._quality_list(self._quality_limits(imgs, has_alpha, max_error_sums, min_psnr), len(imgs))
        imgs, outs, items = self._stream_items(imgs, 0, None, False)
        self._stream_call("limg_hip_encode_stream_quality_list", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), limits, min_error_factor, max_error_factor, pool_threads,
                          int(fast), results)
        return [o[:results[k].bytes].copy() for k, o in enumerate(outs)], results[:len(imgs)]

    def encode_stream_quality_list_device(self, imgs, has_alpha, max_error_sums=None, min_error_factor=0, max_error_factor=0, outs=None, pool_threads=0, fast=True, min_psnr=None):
        """imgs: list of torch int32 CUDA tensors (h, w) of ANY shapes -> (list of torch uint8 CUDA stream buffers, list of QualityResult).  Waits for torch's current
        stream once per round."""
        limits, results = self._quality_list(self._quality_limits(imgs, has_alpha, max_error_sums, min_psnr), len(imgs))
        imgs, outs, items = self._stream_items(imgs, 0, outs, True)
        self._stream_call("limg_hip_encode_stream_quality_list_device", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), limits, min_error_factor, max_error_factor,
                          pool_threads, int(fast), results, self._stream())
        return outs, results[:len(imgs)]

    # ---- ... to a byte budget per image, and the sizes of every image at a list of error factors (contract: include/limg_hip.h) ----
    def encode_stream_budget_list(self, imgs, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, pool_threads=0, fast=True):
        """host uint32 images of ANY shapes, max_bytes an int or one per image -> (list of stream bytes (numpy uint8), list of BudgetResult), one call"""
        budgets, results = self._budget_list(max_bytes, len(imgs))
        imgs, outs, items = self._stream_items(imgs, 0, None, False)
        self._stream_call("limg_hip_encode_stream_budget_list", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), budgets, min_error_factor, max_error_factor, pool_threads,
                          int(fast), results)
        return [o[:results[k].bytes].copy() for k, o in enumerate(outs)], results[:len(imgs)]

    def encode_stream_budget_list_device(self, imgs, has_alpha, max_bytes, min_error_factor=0, max_error_factor=0, outs=None, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of ANY shapes, max_bytes an int or one per image -> (list of torch uint8 CUDA stream buffers, each of its
        image's worst-case size, list of BudgetResult).  Waits for torch's current stream once per chunk."""
        budgets, results = self._budget_list(max_bytes, len(imgs))
        imgs, outs, items = self._stream_items(imgs, 0, outs, True)
        self._stream_call("limg_hip_encode_stream_budget_list_device", len(imgs), items, C.sizeof(StreamListItem), int(has_alpha), budgets, min_error_factor, max_error_factor,
                          pool_threads, int(fast), results, self._stream())
        return outs, results[:len(imgs)]

    def _sizes_list(self, name, imgs, has_alpha, error_factors, pool_threads, fast, device):
        """one call of a sizes-list entry: items without stream buffers (pStream NULL, capacity 0) -> numpy uint64 (len(imgs), len(error_factors))"""
        if not device:
            imgs = [np.ascontiguousarray(i, dtype=np.uint32) for i in imgs]
        n, m = len(imgs), len(error_factors)
        ptr = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
        items = (StreamListItem * max(n, 1))()
        for k in range(n):
            items[k] = StreamListItem(ptr(imgs[k]), None, 0, imgs[k].shape[1], imgs[k].shape[0], 0, 0)
        efs, sizes = (C.c_uint32 * max(m, 1))(*[int(e) for e in error_factors]), (C.c_size_t * max(n * m, 1))()
        self._stream_call(name, n, items, C.sizeof(StreamListItem), int(has_alpha), efs, m, sizes, pool_threads, int(fast), *([self._stream()] if device else []))
        return np.array(sizes[:n * m], dtype=np.uint64).reshape(n, m)

    def stream_sizes_list(self, imgs, has_alpha, error_factors, pool_threads=0, fast=True):
        """host uint32 images of ANY shapes -> array [i, k] = len(encode_stream(imgs[i], ..., error_factor=error_factors[k])), without encoding"""
        return self._sizes_list("limg_hip_stream_sizes_list", imgs, has_alpha, error_factors, pool_threads, fast, False)

    def stream_sizes_list_device(self, imgs, has_alpha, error_factors, pool_threads=0, fast=True):
        """imgs: list of torch int32 CUDA tensors (h, w) of ANY shapes; waits for torch's current stream"""
        return self._sizes_list("limg_hip_stream_sizes_list_device", imgs, has_alpha, error_factors, pool_threads, fast, True)

    def blocked_stream_bound(self, w, h):
        return self.lib.limg_hip_blocked_stream_bound(w, h)

    def blocked_stream_info(self, stream):
        return blocked_stream_info(stream, self.lib)

    def blocked_encode_stream(self, img, has_alpha, error_factor=100, fast=True):
        """host uint32 image -> version 2 stream bytes (numpy uint8); blocked_regions() / blocked_timing() describe this encode afterwards"""
        return self._encode_stream("limg_hip_blocked_encode_stream", self.blocked_stream_bound, img, has_alpha, (error_factor, int(fast)))

    def blocked_last_stream(self, w, h):
        """the version 2 stream of this context's last merged-block encode (planes or stream), of a w x h image, without encoding again"""
        out = np.zeros(self.blocked_stream_bound(w, h), dtype=np.uint8)
        n = C.c_size_t(0)
        self._stream_call("limg_hip_blocked_last_stream", _np_ptr(out), out.size, C.byref(n))
        return out[:n.value].copy()

    def blocked_decode_stream(self, stream):
        w, h = blocked_stream_info(stream, self.lib)[:2]
        return self._decode_stream("limg_hip_blocked_decode_stream", stream, w, h)

    def blocked_encode_stream_device(self, img, has_alpha, out=None, error_factor=100, fast=True, want_size=True):
        """img: torch int32 CUDA (h, w) -> (torch uint8 CUDA stream buffer of worst-case size, bytes used or None)"""
        return self._encode_stream_device("limg_hip_blocked_encode_stream_device", self.blocked_stream_bound, img, has_alpha, out, want_size, (error_factor, int(fast)))

    def blocked_decode_stream_device(self, stream, nbytes, w, h, out=None):
        return self._decode_stream_device("limg_hip_blocked_decode_stream_device", stream, nbytes, w, h, out)

    # ---- window decode: any pixel rectangle of a stream (contract: include/limg_hip.h) ----
    def _decode_stream_window(self, name, stream, x, y, w, h, out):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        if out is None:
            out = np.zeros((h, w), dtype=np.uint32)
        assert out.dtype == np.uint32 and out.ndim == 2 and out.strides[1] == 4 and out.strides[0] % 4 == 0, "out: uint32 rows, pixels contiguous"
        self._stream_call(name, _np_ptr(stream), stream.size, x, y, w, h, _np_ptr(out), out.strides[0] // 4)
        return out

    def _decode_stream_window_device(self, name, stream, nbytes, W, H, x, y, w, h, out, out_stride):
        import torch
        if out is None:
            out = torch.empty((h, w), dtype=torch.int32, device=stream.device)
        if out_stride is None:
            out_stride = out.stride(0) if out.dim() == 2 else w
        self._stream_call(name, C.c_void_p(stream.data_ptr()), int(nbytes), W, H, x, y, w, h, C.c_void_p(out.data_ptr()), int(out_stride), self._stream())
        return out

    def decode_stream_window(self, stream, x, y, w, h, out=None):
        """host stream bytes -> pixels (x .. x + w - 1, y .. y + h - 1) as numpy uint32 (h, w); `out`: a uint32 view (rows may be strided) that receives them"""
        return self._decode_stream_window("limg_hip_decode_stream_window", stream, x, y, w, h, out)

    def blocked_decode_stream_window(self, stream, x, y, w, h, out=None):
        return self._decode_stream_window("limg_hip_blocked_decode_stream_window", stream, x, y, w, h, out)

    def decode_stream_window_device(self, stream, nbytes, W, H, x, y, w, h, out=None, out_stride=None):
        """stream: torch uint8 CUDA tensor holding a stream of a W x H image; out: torch int32 CUDA tensor whose first element receives pixel (x, y), rows out_stride
        pixels apart (default: out's own row stride); only the window's pixels are written.  Asynchronous on torch's current stream."""
        return self._decode_stream_window_device("limg_hip_decode_stream_window_device", stream, nbytes, W, H, x, y, w, h, out, out_stride)

    def blocked_decode_stream_window_device(self, stream, nbytes, W, H, x, y, w, h, out=None, out_stride=None):
        return self._decode_stream_window_device("limg_hip_blocked_decode_stream_window_device", stream, nbytes, W, H, x, y, w, h, out, out_stride)

    # ---- batched window decode: many windows of many streams per call, into packed RGBA8 or planar float tensors, at full or reduced scale (contract: include/limg_hip.h).
    # The two builders below make every entry's table; `scaled`: a level 0 .. 3 leads the window's (x, y, w, h) and ends its struct; fmt: the tensor format, None for RGBA8.
    def _decode_windows_device(self, name, jobs, scaled, fmt, status):
        import torch
        planar = fmt is not None
        win_t, job_t = _WINDOW_TYPES[scaled, planar]
        dtype = torch.int32 if not planar else torch.float16 if fmt.type == TENSOR_F16 else torch.float32
        table = (job_t * len(jobs))()
        outs = []
        for i, job in enumerate(jobs):  # (a loader calls this per step with thousands of jobs: the four tuple layouts are unpacked by name, everything else is shared)
            if planar:
                if scaled:
                    stream, nbytes, W, H, level, x, y, w, h, out, row, plane = job
                else:
                    stream, nbytes, W, H, x, y, w, h, out, row, plane = job
            elif scaled:
                stream, nbytes, W, H, level, x, y, w, h, out, row = job
            else:
                stream, nbytes, W, H, x, y, w, h, out, row = job
            if out is None:
                out = torch.empty((fmt.planes, h, w) if planar else (h, w), dtype=dtype, device=stream.device)
            if row is None:  # out's own strides where it has the window's shape, else densely packed
                row = out.stride(-2) if out.dim() == 2 + planar else w
            if planar:
                assert out.dtype == dtype, (out.dtype, dtype)
                if plane is None:
                    plane = out.stride(0) if out.dim() == 3 else row * h
                win = win_t(x, y, w, h, out.data_ptr(), int(row), int(plane))
            else:
                win = win_t(x, y, w, h, out.data_ptr(), int(row))
            if scaled:
                win.log2Scale = level
            table[i] = job_t(stream.data_ptr(), int(nbytes), W, H, win)
            outs.append(out)
        self._stream_call(name, table, len(jobs), *([C.byref(fmt)] if planar else []), C.c_void_p(status.data_ptr()) if status is not None else None, self._stream())
        return outs

    def _decode_windows_host(self, name, stream, wins, scaled, fmt, outs):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        planar = fmt is not None
        win_t = _WINDOW_TYPES[scaled, planar][0]
        dtype = np.dtype(np.uint32 if not planar else np.float16 if fmt.type == TENSOR_F16 else np.float32)
        eb = dtype.itemsize
        outs = [None] * len(wins) if outs is None else list(outs)
        table = (win_t * len(wins))()
        for i, win in enumerate(wins):
            x, y, w, h = win[scaled:]
            if outs[i] is None:
                outs[i] = np.zeros((fmt.planes, h, w) if planar else (h, w), dtype=dtype)
            out = outs[i]
            if planar:
                assert out.dtype == dtype and out.ndim == 3 and out.shape[0] >= fmt.planes and out.strides[2] == eb and out.strides[1] % eb == 0 and out.strides[0] % eb == 0, \
                    "out: (planes, h, w) of the format's type, elements of a row contiguous"
            else:
                assert out.dtype == np.uint32 and out.ndim == 2 and out.strides[1] == 4 and out.strides[0] % 4 == 0, "out: uint32 rows, pixels contiguous"
            table[i] = win_t(x, y, w, h, out.ctypes.data, *[s // eb for s in out.strides[-2::-1]], *win[:scaled])  # (strides: of the rows, then of the planes)
        self._stream_call(name, _np_ptr(stream), stream.size, table, len(wins), *([C.byref(fmt)] if planar else []))
        return outs

    def decode_stream_windows_device(self, jobs, status=None):
        """jobs: (stream tensor, nbytes, W, H, x, y, w, h, out, out_stride) each, as the arguments of decode_stream_window_device (out=None allocates, out_stride=None is
        out's own row stride); status: torch int32 CUDA tensor of len(jobs) words or None.  One launch for all of them, asynchronous on torch's current stream.
        Returns the list of output tensors."""
        return self._decode_windows_device("limg_hip_decode_stream_windows_device", jobs, False, None, status)

    def blocked_decode_stream_windows_device(self, jobs, status=None):
        return self._decode_windows_device("limg_hip_blocked_decode_stream_windows_device", jobs, False, None, status)

    def decode_stream_windows(self, stream, wins, outs=None):
        """host stream bytes, wins: (x, y, w, h) each -> the list of numpy uint32 (h, w) arrays; outs: per window a uint32 view that receives it (rows may be strided)
        or None.  The stream is uploaded once."""
        return self._decode_windows_host("limg_hip_decode_stream_windows", stream, wins, False, None, outs)

    def blocked_decode_stream_windows(self, stream, wins, outs=None):
        return self._decode_windows_host("limg_hip_blocked_decode_stream_windows", stream, wins, False, None, outs)

    # ---- stream error inside the decode: windows of streams against originals, a sum per job and no decoded pixel (contract: include/limg_hip.h) ----
    def _decode_windows_error_device(self, name, jobs, sums, status):
        import torch
        table = (ErrorWindowJob * len(jobs))()
        for i, (stream, nbytes, W, H, x, y, w, h, original, stride) in enumerate(jobs):
            if stride is None:  # original's own row stride where it has the window's shape, else densely packed
                stride = original.stride(0) if original.dim() == 2 else w
            table[i] = ErrorWindowJob(stream.data_ptr(), int(nbytes), W, H, ErrorWindow(x, y, w, h, original.data_ptr(), int(stride)))
        if sums is None:
            sums = torch.empty(len(jobs), dtype=torch.int64, device=jobs[0][0].device)
        self._stream_call(name, table, len(jobs), C.c_void_p(sums.data_ptr()), C.c_void_p(status.data_ptr()) if status is not None else None, self._stream())
        return sums

    def _decode_windows_error_host(self, name, stream, wins, originals):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        table = (ErrorWindow * len(wins))()
        for i, ((x, y, w, h), o) in enumerate(zip(wins, originals)):
            assert o.dtype == np.uint32 and o.ndim == 2 and o.shape == (h, w) and o.strides[1] == 4 and o.strides[0] % 4 == 0, "original: uint32 (h, w), pixels contiguous"
            table[i] = ErrorWindow(x, y, w, h, o.ctypes.data, o.strides[0] // 4)
        sums = (C.c_uint64 * max(len(wins), 1))()
        self._stream_call(name, _np_ptr(stream), stream.size, table, len(wins), sums)
        return [int(v) for v in sums[:len(wins)]]

    def decode_stream_windows_error_device(self, jobs, sums=None, status=None):
        """jobs: (stream tensor, nbytes, W, H, x, y, w, h, original, original_stride) each; original: a torch int32 CUDA tensor whose first element is the original's pixel
        for image pixel (x, y), rows original_stride pixels apart (None: its own row stride).  sums: torch int64 CUDA tensor of len(jobs) (None allocates); status as in
        decode_stream_windows_device.  One launch, asynchronous on torch's current stream; nothing but `sums` (and `status`) is written.  Returns sums."""
        return self._decode_windows_error_device("limg_hip_decode_stream_windows_error_device", jobs, sums, status)

    def blocked_decode_stream_windows_error_device(self, jobs, sums=None, status=None):
        return self._decode_windows_error_device("limg_hip_blocked_decode_stream_windows_error_device", jobs, sums, status)

    def decode_stream_windows_error(self, stream, wins, originals):
        """host stream bytes, wins: (x, y, w, h) each, originals: per window a uint32 (h, w) view (rows may be strided) -> the list of error sums (int)"""
        return self._decode_windows_error_host("limg_hip_decode_stream_windows_error", stream, wins, originals)

    def blocked_decode_stream_windows_error(self, stream, wins, originals):
        return self._decode_windows_error_host("limg_hip_blocked_decode_stream_windows_error", stream, wins, originals)

    def stream_compare(self, stream, original):
        """host stream bytes of either version against the host uint32 original -> (psnr, mse) of compare(original, decode_stream(stream)), without the decoded image"""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        original = np.ascontiguousarray(original, dtype=np.uint32)
        mse, mx = C.c_double(), C.c_double()
        p = self.lib.limg_hip_stream_compare(self.ctx, _np_ptr(stream), stream.size, _np_ptr(original), original.size, C.byref(mse), C.byref(mx))
        return p, mse.value

    def error_sum_for_psnr(self, w, h, has_alpha, psnr):
        """the largest error sum over w x h pixels whose PSNR is at least `psnr` dB: what the quality entries take as their limit"""
        return int(self.lib.limg_hip_error_sum_for_psnr(w, h, int(has_alpha), float(psnr)))

    def decode_stream_windows_tensor_device(self, jobs, fmt, status=None):
        """jobs: (stream tensor, nbytes, W, H, x, y, w, h, out, row_stride, plane_stride) each; out: a torch CUDA tensor of fmt's type whose first element receives
        element (0, 0, 0) of the window, rows row_stride and planes plane_stride elements apart (None: out's own strides; out=None allocates (planes, h, w)).
        fmt: tensor_format(...).  status: torch int32 CUDA tensor of len(jobs) words or None.  One launch for all jobs, asynchronous on torch's current stream.
        Returns the list of output tensors."""
        return self._decode_windows_device("limg_hip_decode_stream_windows_tensor_device", jobs, False, fmt, status)

    def blocked_decode_stream_windows_tensor_device(self, jobs, fmt, status=None):
        return self._decode_windows_device("limg_hip_blocked_decode_stream_windows_tensor_device", jobs, False, fmt, status)

    def decode_stream_windows_tensor(self, stream, wins, fmt, outs=None):
        """host stream bytes, wins: (x, y, w, h) each -> the list of numpy (planes, h, w) arrays of fmt's type; outs: per window a view that receives it (rows and
        planes may be strided) or None.  The stream is uploaded once."""
        return self._decode_windows_host("limg_hip_decode_stream_windows_tensor", stream, wins, False, fmt, outs)

    def blocked_decode_stream_windows_tensor(self, stream, wins, fmt, outs=None):
        return self._decode_windows_host("limg_hip_blocked_decode_stream_windows_tensor", stream, wins, False, fmt, outs)

    def _decode_crops(self, jobs, scaled, h, w, dtype, scale, bias, planes, blocked, out):
        import torch
        fmt = tensor_format(dtype, planes, scale, bias)
        if out is None:
            out = torch.empty((len(jobs), planes, h, w), dtype=dtype, device=jobs[0][0].device)
        assert tuple(out.shape) == (len(jobs), planes, h, w) and out.is_contiguous() and out.dtype == dtype
        assert all(len(j) == 6 + scaled for j in jobs)
        table = [(*j, w, h, out[i], w, h * w) for i, j in enumerate(jobs)]
        getattr(self, ("blocked_" if blocked else "") + "decode_stream_windows_" + ("scaled_" if scaled else "") + "tensor_device")(table, fmt)
        return out

    def decode_crops_device(self, jobs, h, w, dtype, scale, bias, planes=3, blocked=False, out=None):
        """The loader step: jobs: (stream tensor, nbytes, W, H, x, y) each -- the h x w crop at (x, y) of each stream -> ONE contiguous (N, planes, h, w) torch tensor
        of `dtype` (torch.float32 / torch.float16), element = byte * scale[c] + bias[c]; job i fills slice i.  out: the tensor to fill.  One call of the version's
        tensor entry, asynchronous on torch's current stream."""
        return self._decode_crops(jobs, False, h, w, dtype, scale, bias, planes, blocked, out)

    # ---- reduced-scale window decode: every job at its own level 0 .. 3, RGBA8 or tensors (contract: include/limg_hip.h) ----
    def decode_stream_windows_scaled_device(self, jobs, status=None):
        """jobs: (stream tensor, nbytes, W, H, level, x, y, w, h, out, out_stride) each: the jobs of decode_stream_windows_device with the level 0 .. 3 behind the image
        size; x, y, w, h are in that level's coordinates, inside (W >> level) x (H >> level).  One launch whatever the mix of levels."""
        return self._decode_windows_device("limg_hip_decode_stream_windows_scaled_device", jobs, True, None, status)

    def blocked_decode_stream_windows_scaled_device(self, jobs, status=None):
        return self._decode_windows_device("limg_hip_blocked_decode_stream_windows_scaled_device", jobs, True, None, status)

    def decode_stream_windows_scaled_tensor_device(self, jobs, fmt, status=None):
        """jobs: (stream tensor, nbytes, W, H, level, x, y, w, h, out, row_stride, plane_stride) each, as decode_stream_windows_tensor_device with the level"""
        return self._decode_windows_device("limg_hip_decode_stream_windows_scaled_tensor_device", jobs, True, fmt, status)

    def blocked_decode_stream_windows_scaled_tensor_device(self, jobs, fmt, status=None):
        return self._decode_windows_device("limg_hip_blocked_decode_stream_windows_scaled_tensor_device", jobs, True, fmt, status)

    def decode_stream_windows_scaled(self, stream, wins, outs=None):
        """host stream bytes, wins: (level, x, y, w, h) each -> the list of numpy uint32 (h, w) arrays; one upload and one batched call for all levels"""
        return self._decode_windows_host("limg_hip_decode_stream_windows_scaled", stream, wins, True, None, outs)

    def blocked_decode_stream_windows_scaled(self, stream, wins, outs=None):
        return self._decode_windows_host("limg_hip_blocked_decode_stream_windows_scaled", stream, wins, True, None, outs)

    def decode_stream_windows_scaled_tensor(self, stream, wins, fmt, outs=None):
        """host stream bytes, wins: (level, x, y, w, h) each -> the list of numpy (planes, h, w) arrays of fmt's type"""
        return self._decode_windows_host("limg_hip_decode_stream_windows_scaled_tensor", stream, wins, True, fmt, outs)

    def blocked_decode_stream_windows_scaled_tensor(self, stream, wins, fmt, outs=None):
        return self._decode_windows_host("limg_hip_blocked_decode_stream_windows_scaled_tensor", stream, wins, True, fmt, outs)

    def decode_crops_scaled_device(self, jobs, h, w, dtype, scale, bias, planes=3, blocked=False, out=None):
        """The loader step where every sample picks its own level: jobs: (stream tensor, nbytes, W, H, level, x, y) each -- the h x w crop at (x, y) of the stream's
        level-`level` image -> ONE contiguous (N, planes, h, w) torch tensor of `dtype`, as decode_crops_device.  One call of the version's scaled tensor entry."""
        return self._decode_crops(jobs, True, h, w, dtype, scale, bias, planes, blocked, out)

    # ---- resized window decode: any source rectangle to any output size, bilinear on a box level, optionally mirrored (contract: include/limg_hip.h) ----
    def _decode_resized_device(self, name, jobs, fmt, status):
        import torch
        planar = fmt is not None
        win_t, job_t = (ResizedTensorWindow, ResizedTensorWindowJob) if planar else (ResizedWindow, ResizedWindowJob)
        dtype = torch.int32 if not planar else torch.float16 if fmt.type == TENSOR_F16 else torch.float32
        table = (job_t * len(jobs))()
        outs = []
        for i, job in enumerate(jobs):
            if planar:
                stream, nbytes, W, H, level, flags, x, y, sw, sh, ow, oh, out, row, plane = job
            else:
                stream, nbytes, W, H, level, flags, x, y, sw, sh, ow, oh, out, row = job
            if out is None:
                out = torch.empty((fmt.planes, oh, ow) if planar else (oh, ow), dtype=dtype, device=stream.device)
            if row is None:
                row = out.stride(-2) if out.dim() == 2 + planar else ow
            level = RESIZE_AUTO if level is None else level
            if planar:
                assert out.dtype == dtype, (out.dtype, dtype)
                if plane is None:
                    plane = out.stride(0) if out.dim() == 3 else row * oh
                win = win_t(x, y, sw, sh, out.data_ptr(), int(row), int(plane), ow, oh, level, flags)
            else:
                win = win_t(x, y, sw, sh, out.data_ptr(), int(row), ow, oh, level, flags)
            table[i] = job_t(stream.data_ptr(), int(nbytes), W, H, win)
            outs.append(out)
        self._stream_call(name, table, len(jobs), *([C.byref(fmt)] if planar else []), C.c_void_p(status.data_ptr()) if status is not None else None, self._stream())
        return outs

    def _decode_resized_host(self, name, stream, wins, fmt, outs):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        planar = fmt is not None
        win_t = ResizedTensorWindow if planar else ResizedWindow
        dtype = np.dtype(np.uint32 if not planar else np.float16 if fmt.type == TENSOR_F16 else np.float32)
        eb = dtype.itemsize
        outs = [None] * len(wins) if outs is None else list(outs)
        table = (win_t * len(wins))()
        for i, (level, flags, x, y, sw, sh, ow, oh) in enumerate(wins):
            if outs[i] is None:
                outs[i] = np.zeros((fmt.planes, oh, ow) if planar else (oh, ow), dtype=dtype)
            out = outs[i]
            if planar:
                assert out.dtype == dtype and out.ndim == 3 and out.shape[0] >= fmt.planes and out.strides[2] == eb and out.strides[1] % eb == 0 and out.strides[0] % eb == 0, \
                    "out: (planes, h, w) of the format's type, elements of a row contiguous"
            else:
                assert out.dtype == np.uint32 and out.ndim == 2 and out.strides[1] == 4 and out.strides[0] % 4 == 0, "out: uint32 rows, pixels contiguous"
            table[i] = win_t(x, y, sw, sh, out.ctypes.data, *[s // eb for s in out.strides[-2::-1]], ow, oh, RESIZE_AUTO if level is None else level, flags)
        self._stream_call(name, _np_ptr(stream), stream.size, table, len(wins), *([C.byref(fmt)] if planar else []))
        return outs

    def decode_stream_windows_resized_device(self, jobs, status=None):
        """jobs: (stream tensor, nbytes, W, H, level, flags, x, y, sw, sh, ow, oh, out, out_stride) each: the source rectangle (x, y, sw, sh) of the W x H image,
        full-resolution pixels, as ow x oh pixels; level 0 .. 3 or None (RESIZE_AUTO); flags: RESIZE_FLIP_X or 0.  out=None allocates (oh, ow) int32.  One launch."""
        return self._decode_resized_device("limg_hip_decode_stream_windows_resized_device", jobs, None, status)

    def blocked_decode_stream_windows_resized_device(self, jobs, status=None):
        return self._decode_resized_device("limg_hip_blocked_decode_stream_windows_resized_device", jobs, None, status)

    def decode_stream_windows_resized_tensor_device(self, jobs, fmt, status=None):
        """jobs: (stream tensor, nbytes, W, H, level, flags, x, y, sw, sh, ow, oh, out, row_stride, plane_stride) each, into planes of fmt's type"""
        return self._decode_resized_device("limg_hip_decode_stream_windows_resized_tensor_device", jobs, fmt, status)

    def blocked_decode_stream_windows_resized_tensor_device(self, jobs, fmt, status=None):
        return self._decode_resized_device("limg_hip_blocked_decode_stream_windows_resized_tensor_device", jobs, fmt, status)

    def decode_stream_windows_resized(self, stream, wins, outs=None):
        """host stream bytes, wins: (level, flags, x, y, sw, sh, ow, oh) each -> the list of numpy uint32 (oh, ow) arrays; one upload and one batched call"""
        return self._decode_resized_host("limg_hip_decode_stream_windows_resized", stream, wins, None, outs)

    def blocked_decode_stream_windows_resized(self, stream, wins, outs=None):
        return self._decode_resized_host("limg_hip_blocked_decode_stream_windows_resized", stream, wins, None, outs)

    def decode_stream_windows_resized_tensor(self, stream, wins, fmt, outs=None):
        """host stream bytes, wins: (level, flags, x, y, sw, sh, ow, oh) each -> the list of numpy (planes, oh, ow) arrays of fmt's type"""
        return self._decode_resized_host("limg_hip_decode_stream_windows_resized_tensor", stream, wins, fmt, outs)

    def blocked_decode_stream_windows_resized_tensor(self, stream, wins, fmt, outs=None):
        return self._decode_resized_host("limg_hip_blocked_decode_stream_windows_resized_tensor", stream, wins, fmt, outs)

    def decode_crops_resized_device(self, jobs, h, w, dtype, scale, bias, planes=3, blocked=False, out=None, level=None):
        """RandomResizedCrop + flip + normalise + layout in one call: jobs: (stream tensor, nbytes, W, H, x, y, sw, sh[, flip]) each -- the source rectangle
        (x, y, sw, sh) of each stream resampled to h x w, mirrored where flip is true -> ONE contiguous (N, planes, h, w) torch tensor of `dtype`, element =
        byte * scale[c] + bias[c]; job i fills slice i.  level: 0 .. 3 for every job, or None: each job's deepest level that keeps a level pixel per output pixel.
        out: the tensor to fill.  One call of the version's resized tensor entry, asynchronous on torch's current stream."""
        import torch
        fmt = tensor_format(dtype, planes, scale, bias)
        if out is None:
            out = torch.empty((len(jobs), planes, h, w), dtype=dtype, device=jobs[0][0].device)
        assert tuple(out.shape) == (len(jobs), planes, h, w) and out.is_contiguous() and out.dtype == dtype
        assert all(len(j) in (8, 9) for j in jobs)
        table = [(*j[:4], level, RESIZE_FLIP_X if len(j) == 9 and j[8] else 0, *j[4:8], w, h, out[i], w, h * w) for i, j in enumerate(jobs)]
        getattr(self, ("blocked_" if blocked else "") + "decode_stream_windows_resized_tensor_device")(table, fmt)
        return out

    # ---- stream splice: a version 1 stream from rectangles of blocks of version 1 streams, copied on the GPU, never decoded (contract: include/limg_hip.h) ----
    # A piece: (stream, src_bx, src_by, dst_bx, dst_by, blocks_w, blocks_h[, src_w, src_h]) in blocks of 8x8; the source's size is its header's unless given.
    # Host form: stream is a numpy uint8 array.  Device form: stream is (torch uint8 CUDA tensor, nbytes) and the source's size must be given.
    @staticmethod
    def _splice_pieces(pieces, device):
        keep, table = [], (SplicePiece * max(1, len(pieces)))()
        for i, pc in enumerate(pieces):
            stream, geometry, size = pc[0], pc[1:7], pc[7:9]
            if device:
                tensor, nbytes = stream
                assert len(size) == 2, "device form: (..., src_w, src_h) ends a piece"
                ptr = C.c_void_p(tensor.data_ptr())
            elif stream is None:  # (a NULL source: the library's to refuse)
                nbytes, ptr = 0, None
            else:
                stream = np.ascontiguousarray(stream, dtype=np.uint8)
                keep.append(stream)
                nbytes, ptr = stream.size, _np_ptr(stream)
                if len(size) != 2:
                    hdr = stream[:STREAM_HEADER_DTYPE.itemsize].view(STREAM_HEADER_DTYPE)[0]
                    size = (int(hdr["sizeX"]), int(hdr["sizeY"]))
            table[i] = SplicePiece(ptr, int(nbytes), size[0], size[1], *[int(v) for v in geometry])
        return table, keep

    def stream_splice(self, pieces, w, h, has_alpha, error_factor=0, flags=0, out=None):
        """host streams -> the stream (numpy uint8) of the w x h image whose block grid the pieces cover exactly once; `out`: a uint8 buffer of the caller's (its
        leading bytes are returned as a view)"""
        table, keep = self._splice_pieces(pieces, False)
        buf = np.zeros(self.stream_bound(w, h), dtype=np.uint8) if out is None else out
        n = C.c_size_t(0)
        self._stream_call("limg_hip_stream_splice", table, len(pieces), C.sizeof(SplicePiece), w, h, int(has_alpha), error_factor, flags, _np_ptr(buf), buf.size, C.byref(n))
        return buf[:n.value].copy() if out is None else buf[:n.value]

    def stream_splice_device(self, pieces, w, h, has_alpha, error_factor=0, flags=0, out=None, want_size=True):
        """-> (torch uint8 CUDA stream buffer of worst-case size, bytes used or None).  Asynchronous on torch's current stream unless the size is wanted."""
        import torch
        table, _ = self._splice_pieces(pieces, True)
        if out is None:
            out = torch.empty(self.stream_bound(w, h), dtype=torch.uint8, device=pieces[0][0][0].device)
        n = C.c_size_t(0)
        self._stream_call("limg_hip_stream_splice_device", table, len(pieces), C.sizeof(SplicePiece), w, h, int(has_alpha), error_factor, flags, C.c_void_p(out.data_ptr()),
                          out.numel(), C.byref(n) if want_size else None, self._stream())
        return out, (n.value if want_size else None)

    def stream_crop(self, stream, x, y, w, h, out=None):
        """host stream bytes -> the stream of its w x h window at (x, y): x, y multiples of 8, x + w and y + h multiples of 8 or the image's edge"""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        buf = np.zeros(max(self.stream_bound(w, h), 64), dtype=np.uint8) if out is None else out
        n = C.c_size_t(0)
        self._stream_call("limg_hip_stream_crop", _np_ptr(stream), stream.size, x, y, w, h, _np_ptr(buf), buf.size, C.byref(n))
        return buf[:n.value].copy() if out is None else buf[:n.value]

    def stream_crop_device(self, stream, nbytes, W, H, has_alpha, x, y, w, h, error_factor=0, flags=0, out=None, want_size=True):
        """stream: torch uint8 CUDA tensor holding a stream of a W x H image -> (stream buffer of the window's image, bytes used or None)"""
        import torch
        if out is None:
            out = torch.empty(max(self.stream_bound(w, h), 64), dtype=torch.uint8, device=stream.device)
        n = C.c_size_t(0)
        self._stream_call("limg_hip_stream_crop_device", C.c_void_p(stream.data_ptr()), int(nbytes), W, H, int(has_alpha), x, y, w, h, error_factor, flags,
                          C.c_void_p(out.data_ptr()), out.numel(), C.byref(n) if want_size else None, self._stream())
        return out, (n.value if want_size else None)

    def join_strip_streams(self, streams, has_alpha=None):
        """The streams of an image's strips, top to bottom (every strip but the last a multiple of 8 rows, one width, one channel count) -> the stream of the image:
        what turns limg_hip_gather_stream's pieces into one stream.  streams: numpy uint8 arrays, or (torch uint8 CUDA tensor, nbytes, w, h) tuples, which are
        joined on the device (has_alpha stated) and give (stream buffer, bytes used).  Error factor and flags are the first strip's (host form) / 0 (device form)."""
        device = not isinstance(streams[0], np.ndarray)
        pieces, y, first = [], 0, None
        for s in streams:
            if device:
                tensor, nbytes, w, h = s
                src = (tensor, nbytes)
            else:
                src = np.ascontiguousarray(s, dtype=np.uint8)
                hdr = src[:STREAM_HEADER_DTYPE.itemsize].view(STREAM_HEADER_DTYPE)[0]
                w, h = int(hdr["sizeX"]), int(hdr["sizeY"])
                first = hdr if first is None else first
            if y % 8 != 0:
                raise ValueError("only the last strip may have a height that is no multiple of 8")
            pieces.append((src, 0, 0, 0, y // 8, (w + 7) // 8, (h + 7) // 8, w, h))
            y += h
        if device:
            assert has_alpha is not None, "device form: the strips' channel count is the caller's to state"
            return self.stream_splice_device(pieces, pieces[0][7], y, has_alpha)
        return self.stream_splice(pieces, pieces[0][7], y, int(first["channels"]) == 4, int(first["errorFactor"]), int(first["flags"]))

    def check(self):
        _check(self.lib.limg_hip_check_device_status(self.ctx), "limg_hip_check_device_status")

    # ---- multi-GPU: RCCL behind the C ABI ---------------------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
        _check(self.lib.limg_hip_comm_unique_id(_np_ptr(buf)), "limg_hip_comm_unique_id")
        return buf

    def comm_init(self, comm_id, rank, world):
        comm_id = np.ascontiguousarray(comm_id, dtype=np.uint8)
        assert comm_id.size == COMM_ID_BYTES
        _check(self.lib.limg_hip_comm_init(self.ctx, _np_ptr(comm_id), rank, world), "limg_hip_comm_init")
        self.comm_rank, self.comm_world = rank, world

    def comm_init_from_torch(self, dist):
        """Create the context's RCCL communicator inside a torch.distributed job: rank 0 makes the id, the process group only carries its 128 bytes."""
        import torch
        rank, world = dist.get_rank(), dist.get_world_size()
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.from_numpy(self.comm_unique_id() if rank == 0 else np.zeros(COMM_ID_BYTES, dtype=np.uint8)).to(dev)
        dist.broadcast(t, src=0)
        self.comm_init(t.cpu().numpy(), rank, world)

    def comm_info(self):
        """What RCCL says about the context's communicator: {"rank", "ranks" (ncclCommCount), "rccl_version"}."""
        r, n, v = C.c_int(-1), C.c_int(0), C.c_int(0)
        _check(self.lib.limg_hip_comm_info(self.ctx, C.byref(r), C.byref(n), C.byref(v)), "limg_hip_comm_info")
        return {"rank": r.value, "ranks": n.value, "rccl_version": v.value}

    def comm_destroy(self):
        _check(self.lib.limg_hip_comm_destroy(self.ctx), "limg_hip_comm_destroy")

    def gather_stream(self, stream, nbytes, root=0, out=None):
        """stream: torch uint8 CUDA tensor holding this rank's LMG3 stream.  On root returns (gathered CUDA tensor, offsets[world + 1]); None elsewhere."""
        import torch
        world = self.comm_world
        offs = np.zeros(world + 1, dtype=np.uint64)
        if self.comm_rank == root and out is None:
            raise ValueError("root needs an output buffer (worst case: the sum of the ranks' stream bounds)")
        _check(self.lib.limg_hip_gather_stream(self.ctx, C.c_void_p(stream.data_ptr()), int(nbytes), root, C.c_void_p(out.data_ptr()) if out is not None else None,
                                               out.numel() if out is not None else 0, _np_ptr(offs), self._stream()), "limg_hip_gather_stream")
        return (out, offs) if self.comm_rank == root else None

    def encode3d_single_chain_device(self, strip, has_alpha, planes, blocks_before, error_factor=100, fast=True):
        h, w = strip.shape
        info = Info(*[planes[k].data_ptr() for k in PLANES])
        _check(self.lib.limg_hip_encode3d_single_chain_device(self.ctx, C.c_void_p(strip.data_ptr()), w, h, int(has_alpha), C.byref(info), error_factor, int(fast),
                                                              int(blocks_before), self._stream()), "limg_hip_encode3d_single_chain_device")

    def encode3d_chain_device(self, strip, has_alpha, planes, phase, calls=None, base=None, blocks_before=0, error_factor=100, fast=True):
        """phase 1: E step + scan, `calls` (torch int64 CUDA, 1 element) receives the strip's dither-call total; phase 2: F step from `base` (same kind of tensor)."""
        h, w = strip.shape
        info = Info(*[planes[k].data_ptr() for k in PLANES])
        _check(self.lib.limg_hip_encode3d_chain_device(self.ctx, C.c_void_p(strip.data_ptr()), w, h, int(has_alpha), C.byref(info), error_factor, int(fast), phase,
                                                       C.c_void_p(calls.data_ptr()) if calls is not None else None, C.c_void_p(base.data_ptr()) if base is not None else None,
                                                       int(blocks_before), self._stream()), "limg_hip_encode3d_chain_device")

    def profile_begin(self):
        _check(self.lib.limg_hip_profile_begin(self.ctx), "limg_hip_profile_begin")

    def profile_end(self, max_encodes=4096):
        """-> float32 array (n, 3): per profiled encode the milliseconds of k_fit_search, k_strip_scan, k_dither_store."""
        buf = np.zeros((max_encodes, 3), dtype=np.float32)
        n = self.lib.limg_hip_profile_end(self.ctx, _np_ptr(buf), max_encodes)
        if n < 0:
            raise LimgHipError("limg_hip_profile_end failed")
        return buf[:n]

    def device_bytes(self):
        return self.lib.limg_hip_context_device_bytes(self.ctx)


def format_stats(counters, pixels):
    """The text limg_encode3d_test prints for these counters (src/limg.cpp:2235-2248), character for character."""
    c = [int(v) for v in counters]
    t = float(pixels)
    out = "\nAverage Block Bits: %5.3f (A: %5.3f | B: %5.3f | C: %5.3f)\n\n" % ((c[0] + c[1] + c[2]) / t, c[0] / t, c[1] / t, c[2] / t)
    out += "".join(" %d bit   " % (8 - i) for i in range(9))
    for f in range(3):
        out += "\n" + "".join("%7.4f  " % (c[3 + f * 9 + j] * 100.0 / t) for j in range(9))
    return out + "\n\n"
