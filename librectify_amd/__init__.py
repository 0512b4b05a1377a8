"""librectify_amd — MI355X-native librectify hot path.

Python host-side mirror of the reference's C API (reference src/librectify.h) over the C-ABI
shared library librectify_amd.so (HIP kernels for gfx950).  This module is plumbing: ctypes
declarations, numpy views of the POD structs, and a thin Context class.  There is NO CPU
fallback: if the library or a GPU is missing, calls raise.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librectify_amd.so")

# reference src/librectify.h:44-54
LINE_DTYPE = np.dtype(
    [("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("weight", "<f4"), ("err", "<f4"), ("group_id", "<i4")]
)


class Point(C.Structure):  # reference src/librectify.h:60-63
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class ImageTransform(C.Structure):  # reference src/librectify.h:79-86
    _fields_ = [
        ("width", C.c_int),
        ("height", C.c_int),
        ("top_left", Point),
        ("top_right", Point),
        ("bottom_left", Point),
        ("bottom_right", Point),
        ("horizontal_vp", Point),
        ("vertical_vp", Point),
    ]

    def as_array(self):
        """rows TL, TR, BL, BR, hvp, vvp"""
        pts = [self.top_left, self.top_right, self.bottom_left, self.bottom_right, self.horizontal_vp, self.vertical_vp]
        return np.array([[p.x, p.y, p.z] for p in pts], np.float32)


ROTATE_H, ROTATE_V, RECTIFY, KEEP = 0, 1, 2, 3  # reference src/librectify.h:126-132


class RectificationConfig(C.Structure):  # reference src/librectify.h:137-150
    _fields_ = [
        ("vertical_vp_angular_tolerance", C.c_float),
        ("vertical_vp_min_distance", C.c_float),
        ("v_strategy", C.c_int),
        ("horizontal_vp_min_distance", C.c_float),
        ("h_strategy", C.c_int),
    ]

    def __init__(self, tol=40.0, vmin=1.5, v_strategy=RECTIFY, hmin=1.5, h_strategy=RECTIFY):
        super().__init__(tol, vmin, v_strategy, hmin, h_strategy)


class Frame(C.Structure):  # lr_frame: a row of the batch detector's frame table (width == 0 && height == 0)
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
                ("min_length", C.c_float)]


class DrawLinesArgs(C.Structure):  # lr_draw_lines_args
    _fields_ = [("lines", C.c_void_p), ("n_lines", C.c_size_t), ("frames", C.c_void_p), ("H", C.c_void_p)]


class JpegArgs(C.Structure):  # lr_jpeg_args
    _fields_ = [("frames", C.c_void_p), ("sizes", C.c_void_p)]


class JpegDecodeArgs(C.Structure):  # lr_jpeg_decode_args
    _fields_ = [("h_src", C.c_void_p), ("frames", C.c_void_p), ("info", C.c_void_p)]


class TensorArgs(C.Structure):  # lr_tensor_args
    _fields_ = [("frames", C.c_void_p), ("n", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("dtype", C.c_int32),
                ("layout", C.c_int32), ("flags", C.c_int32), ("scale", C.c_double * 3), ("bias", C.c_double * 3),
                ("pad", C.c_double * 3)]


BUF_DX, BUF_DY, BUF_DMASK, BUF_LABEL, BUF_SEED_IDX, BUF_SEED_BIN, BUF_SEED_THR, BUF_MAXMAG, BUF_SEED_SIZE = range(9)
BUF_SEED_REC = 9  # uint32 (n_seeds, 4): index, bin, bits of the threshold, 0
BUF_COUNTS = 10  # uint32 (16,): [0] seeds, [1] components, [2] their pixels, [12] components that were fitted, [13] their pixels
T_UPLOAD, T_FILTER, T_SEEDS, T_FLOOD, T_FIT, T_RANSAC, T_TOTAL, T_FILTER_KERNEL, T_COUNT = range(9)
PIX_U8, PIX_U8X3, PIX_F32 = range(3)  # enum lr_pixel_format
WARP_PREPARE = 0x100  # enum lr_warp_option, or-ed into the format of lr_warp_perspective_device
WARP_PACKED = 0x200  # enum lr_warp_layout, likewise: per-frame output sizes and places (warp_table)
WARP_RAGGED = 0x800  # enum lr_warp_sources, likewise: per-frame source sizes and places as well (ragged_table)
WARP_LINES = 0x1000  # enum lr_warp_lines, likewise: lr_draw_lines_device, whose own arguments travel behind M (DrawLinesArgs)
JPEG_OPTIMIZE = 0x10  # enum lr_jpeg_option: added to [7] of a row of jpeg_table (its optimize=), and to lr_jpeg_bound's layout
WARP_JPEG = 0x2000  # enum lr_warp_jpeg, likewise: lr_encode_jpeg_device, whose own arguments travel behind M (JpegArgs)
WARP_CUBIC = 0x8000  # enum lr_warp_sampling, likewise: the warp (plain, WARP_PACKED, WARP_RAGGED) samples 4 x 4 bicubic, not bilinear
JPEG_SCALED = 0x80000  # enum lr_jpeg_decode_option: or-ed into lr_decode_jpeg_device's format, entry [6] of a frame's row is its scale denominator (1, 2, 4, 8)
JPEG_ANY_SAMPLING = 0x20000  # enum lr_jpeg_decode_option: or-ed into lr_decode_jpeg_device's format, it admits every sampling with factors 1, 2, 4
WARP_JPEG_DECODE = 0x4000  # enum lr_warp_jpeg_decode, likewise: lr_decode_jpeg_device, whose own arguments travel behind M (JpegDecodeArgs)
WARP_BORDER = 0x40000  # enum lr_warp_border, likewise: a border word per frame in the warp's table (border_word, border= of the tables)
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101 = 0, 1, 2, 4  # enum lr_border_mode: OpenCV's numbers
WARP_LENS = 0x100000  # enum lr_warp_lens, likewise: nine lens entries per frame at the end of its row of the warp's table (Lens, lens= of the tables)
WARP_LENS_MODEL = 0x800000  # enum lr_warp_lens_model, likewise and with WARP_LENS: seventeen lens entries per frame instead of nine (LensModel, lens= of the tables)
LENS_RATIONAL, LENS_FISHEYE = 0, 1  # enum lr_lens_model: entry [16] of a frame's seventeen lens entries
WARP_AREA = 0x400000  # enum lr_warp_area, likewise: a sampling factor S (1 .. 8) per frame at the very end of its row of the warp's table (area= of the tables)
WARP_TENSOR = 0x10000  # enum lr_warp_tensor, likewise: lr_pack_tensor_device, whose own arguments travel behind M (TensorArgs)
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = range(3)  # enum lr_tensor_dtype
TENSOR_NCHW, TENSOR_NHWC = range(2)  # enum lr_tensor_layout
TENSOR_SWAP, TENSOR_GRAY3 = 1, 2  # enum lr_tensor_flags
JPEG_OK, JPEG_NOT_JPEG, JPEG_UNSUPPORTED, JPEG_SIZE_MISMATCH, JPEG_DAMAGED = range(5)  # info[5] of lr_decode_jpeg_device
FRAMES_U8, FRAMES_U8X3, FRAMES_F32 = 0x100, 0x200, 0x300  # enum lr_frames_option, or-ed into `refine` of the frame entries


def frames_word(fmt, refine=False):
    """The `refine` word of the lr_find_line_segment_groups_* entries for frames of format fmt (PIX_U8, PIX_U8X3,
    PIX_F32): (fmt + 1) << 8 | flag.  PIX_F32 gives the plain flag, 0 or 1, as these calls always passed it."""
    if fmt not in (PIX_U8, PIX_U8X3, PIX_F32):
        raise ValueError("frames_word: fmt is PIX_U8, PIX_U8X3 or PIX_F32")
    flag = 1 if refine else 0
    return flag if fmt == PIX_F32 else ((fmt + 1) << 8) | flag


def split_frames_word(word):
    """(fmt, flag) of a `refine` word, as the library reads it (api.cpp): a format only in the values 256 .. 1023"""
    word = int(word)
    if word >= 0 and 1 <= (word >> 8) <= 3:
        return (word >> 8) - 1, (word & 0xFF) != 0
    return PIX_F32, word != 0

def _schedule_mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def flood_schedule_perm(n, seed, rnd):
    """The permutation of Context.set_flood_schedule(2, seed): a list of n positions, p[i] the position of the OLD list whose
    entry position i of the new list takes in round `rnd` (0-based: the device's count of rounds with work).  The statement of
    csrc/common.h (flood_schedule_coeffs, flood_schedule_perm) again: i -> (a i + b) mod n, a coprime to n and, from n = 8 on,
    neither 1 nor n - 1; a and b from a hash of (seed, rnd, n)."""
    import math

    n, seed, rnd = int(n), int(seed) & 0xFFFFFFFF, int(rnd) & 0xFFFFFFFF
    if n <= 0:
        return []
    h = _schedule_mix(seed ^ _schedule_mix((rnd * 0x9E3779B9 + n) & 0xFFFFFFFF))
    a = 1
    if n >= 5 and n != 6:
        a = 2 + h % (n - 3)
        while math.gcd(a, n) != 1:
            a = 2 if a + 1 > n - 2 else a + 1
    b = _schedule_mix((h + 1) & 0xFFFFFFFF) % n
    return [(a * i + b) % n for i in range(n)]


EXPORTS = [
    "find_line_segment_groups", "release_line_segments", "compute_rectification_transform",
    "compute_rectification_transform_from_vp", "fit_vanishing_point", "assign_to_group",
    "lr_context_create", "lr_context_destroy", "lr_last_error", "lr_synchronize", "lr_set_ransac_seed",
    "lr_set_ransac_iterations", "lr_set_flood_mode", "lr_device_count", "lr_find_line_segment_groups_device",
    "lr_find_line_segment_groups_host", "lr_find_line_segment_groups_batch_device", "lr_stage_filter",
    "lr_stage_filter_host", "lr_stage_seeds", "lr_stage_flood", "lr_stage_fit", "lr_download", "lr_stage_times",
    "lr_stage_counters", "lr_filter_kernel_ms", "lr_ransac_best", "lr_estimate_line_pencils",
    "lr_find_line_segment_groups_batch_host", "lr_find_line_segment_groups_batch_host_ptrs", "lr_host_alloc", "lr_host_free",
    "lr_set_seed_capacity", "lr_set_flood_blind_rounds", "lr_set_flood_staged", "lr_set_batch_streams", "lr_device_malloc", "lr_device_free", "lr_memcpy_h2d", "lr_cht_vanishing_point", "lr_refine_lines", "lr_set_estimator", "lr_ht_weights", "lr_prosac_solve", "lr_estimate_line_pencils_prosac", "lr_direct_solve", "lr_estimate_line_pencils_direct",
    "lr_estimate_line_pencils_cht", "lr_set_stage_timing", "lr_release_thread_context", "lr_set_flood_partial_commits", "lr_set_flood_logs", "lr_set_flood_just_in_time", "lr_set_flood_giant_step", "lr_set_flood_schedule", "lr_context_trim", "lr_trim_thread_context",
    "lr_find_line_segment_groups_batch_host_multi", "lr_memcpy_d2h", "lr_rectification_homography", "lr_warp_perspective_device",
]

_lib = None


class LibrectifyError(RuntimeError):
    pass


def lib():
    """Loads librectify_amd.so; raises if it has not been built (python -m librectify_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibrectifyError(
                "librectify_amd.so is missing: build it with `python -m librectify_amd.build` (hipcc, gfx950); "
                "there is no CPU fallback"
            )
        L = C.CDLL(LIB_PATH)
        L.lr_last_error.restype = C.c_char_p
        L.find_line_segment_groups.restype = C.c_void_p
        L.find_line_segment_groups.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_bool, C.c_int, C.POINTER(C.c_int)]
        L.release_line_segments.argtypes = [C.POINTER(C.c_void_p)]
        L.release_line_segments.restype = None
        L.compute_rectification_transform.restype = ImageTransform
        L.compute_rectification_transform.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RectificationConfig)]
        L.compute_rectification_transform_from_vp.restype = ImageTransform
        L.compute_rectification_transform_from_vp.argtypes = [C.c_int, C.c_int, C.POINTER(Point), C.POINTER(Point)]
        L.fit_vanishing_point.restype = Point
        L.fit_vanishing_point.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.assign_to_group.restype = None
        L.assign_to_group.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float]
        L.lr_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.lr_context_destroy.argtypes = [C.c_void_p]
        L.lr_context_destroy.restype = None
        L.lr_set_ransac_seed.argtypes = [C.c_void_p, C.c_uint64]
        L.lr_set_ransac_seed.restype = None
        L.lr_set_ransac_iterations.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_ransac_iterations.restype = None
        L.lr_set_flood_mode.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_mode.restype = None
        L.lr_synchronize.argtypes = [C.c_void_p]
        L.lr_find_line_segment_groups_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.lr_find_line_segment_groups_host.argtypes = L.lr_find_line_segment_groups_device.argtypes
        L.lr_find_line_segment_groups_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lr_find_line_segment_groups_batch_host.argtypes = L.lr_find_line_segment_groups_batch_device.argtypes
        L.lr_find_line_segment_groups_batch_host_ptrs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lr_find_line_segment_groups_batch_host_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lr_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.lr_host_free.argtypes = [C.c_void_p, C.c_void_p]
        L.lr_stage_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.lr_stage_filter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.lr_stage_seeds.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.lr_stage_flood.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.lr_stage_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.lr_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.lr_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lr_stage_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lr_filter_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.lr_ransac_best.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.lr_estimate_line_pencils.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_uint64]
        L.lr_device_malloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.lr_device_free.argtypes = [C.c_void_p, C.c_void_p]
        L.lr_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.lr_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.lr_rectification_homography.argtypes = [C.POINTER(ImageTransform), C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.lr_warp_perspective_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t]
        L.lr_set_batch_streams.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_batch_streams.restype = None
        L.lr_set_seed_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.lr_set_seed_capacity.restype = None
        L.lr_set_flood_staged.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_staged.restype = None
        L.lr_set_flood_blind_rounds.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_blind_rounds.restype = None
        L.lr_cht_vanishing_point.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Point), C.c_void_p]
        L.lr_refine_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.lr_set_flood_partial_commits.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_partial_commits.restype = None
        L.lr_set_flood_logs.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_logs.restype = None
        L.lr_set_flood_giant_step.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_giant_step.restype = None
        L.lr_set_flood_schedule.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int]
        L.lr_set_flood_schedule.restype = None
        L.lr_set_flood_just_in_time.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_flood_just_in_time.restype = None
        L.lr_release_thread_context.argtypes = []
        L.lr_release_thread_context.restype = None
        L.lr_set_stage_timing.argtypes = [C.c_void_p, C.c_int]
        L.lr_set_stage_timing.restype = None
        L.lr_set_estimator.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lr_set_estimator.restype = None
        L.lr_ht_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lr_prosac_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        L.lr_estimate_line_pencils_prosac.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_uint64]
        L.lr_direct_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lr_estimate_line_pencils_direct.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        L.lr_estimate_line_pencils_cht.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise LibrectifyError(lib().lr_last_error().decode() or "librectify_amd call failed")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    return lib().lr_device_count()


def prepared_size(width, height, max_size):
    """The reference demo's prescale rule (autorectify.cpp:56-68,121-125; examples/rectify_recipe.cpp) in float32:
    scale = min(f32(max_size) / f32(max(width, height)), 1), sizes max(1, w * scale rounded half away from zero);
    max_size < 1 is a fraction of the longer side.  Returns (out_width, out_height, scale as numpy.float32)."""
    f = np.float32
    longer = max(int(width), int(height))
    px = int(f(longer) * f(max_size)) if max_size < 1 else int(f(max_size))
    scale = min(f(max(1, px)) / f(longer), f(1.0))
    if scale == f(1.0):
        return int(width), int(height), scale
    size = lambda n: max(1, int(np.floor(n * float(scale) + 0.5)))  # noqa: E731
    return size(int(width)), size(int(height)), scale


def border_word(border, fmt):
    """A frame's border word of LR_WARP_BORDER, mode + 8 * value, as an int.  border: None (the zero border: word 0), a mode name
    -- "constant", "replicate", "reflect", "reflect101" -- or ("constant", value); value is an integer 0 .. 255 for PIX_U8, a
    triple of them for PIX_U8X3 and a finite number (taken as float32) for PIX_F32.  ValueError for anything the library
    would refuse."""
    if fmt not in (PIX_U8, PIX_U8X3, PIX_F32):
        raise ValueError("border_word: fmt is PIX_U8, PIX_U8X3 or PIX_F32")
    if border is None:
        return 0
    modes = {"constant": BORDER_CONSTANT, "replicate": BORDER_REPLICATE, "reflect": BORDER_REFLECT, "reflect101": BORDER_REFLECT_101,
             "reflect_101": BORDER_REFLECT_101}
    if isinstance(border, str):
        if border not in modes:
            raise ValueError('border_word: a mode is "constant", "replicate", "reflect" or "reflect101", not %r' % (border,))
        return modes[border]
    if not (isinstance(border, (tuple, list)) and len(border) == 2 and isinstance(border[0], str) and border[0] == "constant"):
        raise ValueError('border_word: a border is None, a mode name or ("constant", value), not %r' % (border,))
    value = border[1]
    byte = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and 0 <= int(v) <= 255  # noqa: E731
    if fmt == PIX_U8:
        if not byte(value):
            raise ValueError("border_word: a u8 border value is an integer from 0 to 255")
        bits = int(value)
    elif fmt == PIX_U8X3:
        if not (isinstance(value, (tuple, list, np.ndarray)) and len(value) == 3 and all(byte(v) for v in value)):
            raise ValueError("border_word: a u8x3 border value is three integers from 0 to 255")
        bits = int(value[0]) | int(value[1]) << 8 | int(value[2]) << 16
    else:
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("border_word: an f32 border value is a finite number")
        with np.errstate(all="ignore"):
            f = np.float32(value)
        if not np.isfinite(f):
            raise ValueError("border_word: an f32 border value is a finite float32")
        bits = int(f.view(np.uint32))
    return BORDER_CONSTANT + 8 * bits


Lens = collections.namedtuple("Lens", "fx fy cx cy k1 k2 p1 p2 k3", defaults=(0.0, 0.0, 0.0, 0.0, 0.0))
Lens.__doc__ = """A frame's lens of LR_WARP_LENS: OpenCV's camera matrix (fx, fy, cx, cy) and distortion vector (k1, k2, p1, p2, k3), in the
source frame's pixel units.  All five coefficients zero: no lens, the plain rule."""


class LensModel(collections.namedtuple("LensModel", "fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 model", defaults=(0.0,) * 13)):
    """A frame's lens of LR_WARP_LENS | LR_WARP_LENS_MODEL: the camera matrix (fx, fy, cx, cy) in the source frame's pixel units,
    twelve coefficients and the model.  model = LENS_RATIONAL (0): OpenCV's distCoeffs of cv::calibrateCamera in OpenCV's order,
    k1, k2, p1, p2, k3, k4, k5, k6 (CALIB_RATIONAL_MODEL), s1, s2, s3, s4 (CALIB_THIN_PRISM_MODEL); all twelve zero: no lens.
    model = LENS_FISHEYE (1): the entries named k1, k2, p1, p2 are cv::fisheye's k1, k2, k3, k4 and the other eight are zero
    (LensModel.fisheye builds it); all four zero: the pure equidistant lens."""
    __slots__ = ()

    @classmethod
    def fisheye(cls, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0):
        """cv::fisheye's model: camera matrix and D = (k1, k2, k3, k4)"""
        return cls(fx, fy, cx, cy, k1, k2, k3, k4, model=LENS_FISHEYE)


def _is_lens_model(lens):
    """lens (not None) has seventeen entries: a LensModel, or a plain sequence longer than a Lens"""
    if isinstance(lens, LensModel):
        return True
    try:
        return not isinstance(lens, Lens) and len(lens) > 9
    except TypeError:
        return False


def _lens_row(lens, what):
    """the nine doubles of one frame's lens, or the seventeen of a LensModel (None: nine zeros, with fx = fy = 1), checked as
    the library checks them"""
    if lens is None:
        return [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    model = _is_lens_model(lens)
    try:
        row = [float(v) for v in (LensModel(*lens) if model else Lens(*lens))]
    except (TypeError, ValueError):
        raise ValueError("%s: a lens is a Lens(fx, fy, cx, cy, k1, k2, p1, p2, k3), a LensModel or None, not %r" % (what, lens)) from None
    if not all(np.isfinite(row)):
        raise ValueError("%s: a lens entry is not finite" % what)
    if row[0] <= 0.0 or row[1] <= 0.0:
        raise ValueError("%s: a lens has fx <= 0 or fy <= 0" % what)
    if model and row[16] not in (LENS_RATIONAL, LENS_FISHEYE):
        raise ValueError("%s: a lens model is LENS_RATIONAL (0) or LENS_FISHEYE (1)" % what)
    if model and row[16] == LENS_FISHEYE and any(v != 0.0 for v in row[8:16]):
        raise ValueError("%s: a fisheye lens has a non-zero entry among k3 .. s4 (its four coefficients are k1, k2, p1, p2)" % what)
    return row


def _lens_rows(lens, count, what):
    """float64 (count, 9): the lens entries of `count` frames from lens=: one Lens for all, or a list of one per frame (None:
    zeros); (count, 17) where a LensModel is among them: a Lens then fills the first nine entries of a LENS_RATIONAL row"""
    if lens is None or isinstance(lens, (Lens, LensModel)):
        specs = [lens] * count
    else:
        specs = list(lens)
        if len(specs) != count:
            raise ValueError("%s: as many lenses as frames (%d), not %d" % (what, count, len(specs)))
    rows = []
    for b, v in enumerate(specs):
        try:
            rows.append(_lens_row(v, what))
        except ValueError as e:
            raise ValueError("%s (frame %d)" % (e, b)) from None
    width = 17 if any(len(r) == 17 for r in rows) else 9
    return np.array([r + [0.0] * (width - len(r)) for r in rows], np.float64).reshape(count, width)


def _lens_bits(rows):
    """WARP_LENS, with WARP_LENS_MODEL for _lens_rows' rows of seventeen"""
    return WARP_LENS | (WARP_LENS_MODEL if rows.shape[1] == 17 else 0)


_ATAN_TABLE = np.array([float.fromhex(v) for v in (
    "0x0.0p+0", "0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2", "0x1.1e00babdefeb4p-1",
    "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")], np.float64)  # atan(i / 8)
_PI_2 = float.fromhex("0x1.921fb54442d18p+0")


def lens_atan(r):
    """lr_lens_atan of include/librectify_amd.h restated operation for operation in float64: LR_WARP_LENS_MODEL's arctangent of
    r >= 0 (an array or a number), within 2^-52 of atan.  Needs no GPU."""
    r = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        big = r > 1.0
        t = np.where(big, 1.0 / np.where(big, r, 1.0), r)
        n = np.rint(8.0 * t)
        i = np.where((n >= 0.0) & (n <= 8.0), n, 0.0).astype(np.int64)
        c = i.astype(np.float64) / 8.0
        z = (t - c) / (1.0 + t * c)
        z2 = z * z
        p = -1.0 / 3.0 + z2 * (1.0 / 5.0 + z2 * (-1.0 / 7.0 + z2 * (1.0 / 9.0 + z2 * (-1.0 / 11.0 + z2 * (1.0 / 13.0 + z2 * (-1.0 / 15.0))))))
        at = _ATAN_TABLE[i] + (z + z * (z2 * p))
        return np.where(big, _PI_2 - at, at)


def lens_distort(lens, points):
    """lr_lens_distort of include/librectify_amd.h (for a LensModel: lr_lens_distort_model) restated operation for operation in
    float64: the pixels of the stored photograph that show the ideal points.  lens: a Lens or a LensModel; points: (..., 2)
    array of (u, v).  Returns float64 of the same shape.  It takes detected lines, which are in ideal coordinates, back onto
    the photograph (after rectify(lens_scale=s): lens_scale_map(lens, s) first).  Needs no GPU."""
    pts = np.asarray(points, np.float64)
    if pts.shape[-1:] != (2,):
        raise ValueError("lens_distort: points is (..., 2)")
    if _is_lens_model(lens):
        return _lens_distort_model(LensModel(*lens), pts)
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(v) for v in Lens(*lens))
    with np.errstate(all="ignore"):
        U, V = 32.0 * pts[..., 0], 32.0 * pts[..., 1]
        a, b = (U * 0.03125 - cx) / fx, (V * 0.03125 - cy) / fy
        r2 = a * a + b * b
        rad = r2 * (k1 + r2 * (k2 + r2 * k3))
        ta = (2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))
        tb = p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)
        du, dv = fx * (a * rad + ta), fy * (b * rad + tb)
        return np.stack([(U + 32.0 * du) / 32.0, (V + 32.0 * dv) / 32.0], axis=-1)


def _lens_distort_model(lens, pts):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model = (np.float64(v) for v in lens)
    with np.errstate(all="ignore"):
        U, V = 32.0 * pts[..., 0], 32.0 * pts[..., 1]
        a, b = (U * 0.03125 - cx) / fx, (V * 0.03125 - cy) / fy
        r2 = a * a + b * b
        if model == 1.0:  # (the fisheye: k1, k2, p1, p2 are its k1 .. k4)
            r = np.sqrt(r2)
            th = lens_atan(r)
            t2 = th * th
            thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (p1 + t2 * p2))))
            sc = np.where(r != 0.0, thd / np.where(r != 0.0, r, 1.0), 1.0)
            X, Y = 32.0 * (fx * (a * sc) + cx), 32.0 * (fy * (b * sc) + cy)
        elif any(float(v) != 0.0 for v in lens[4:16]):
            radn = r2 * (k1 + r2 * (k2 + r2 * k3))
            radd = r2 * (k4 + r2 * (k5 + r2 * k6))
            rad = (radn - radd) / (1.0 + radd)
            ta = ((2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))) + r2 * (s1 + r2 * s2)
            tb = (p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)) + r2 * (s3 + r2 * s4)
            du, dv = fx * (a * rad + ta), fy * (b * rad + tb)
            X, Y = U + 32.0 * du, V + 32.0 * dv
        else:
            X, Y = U, V
        return np.stack([X / 32.0, Y / 32.0], axis=-1)


def _check_lens_scale(what, s):
    if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)) or not np.isfinite(s) or not s > 0:
        raise ValueError("%s: lens_scale is a finite number greater than 0" % what)
    return float(s)


def lens_scale_map(lens, s):
    """The map from the ideal picture scaled by s about the lens's centre (cx, cy) to the ideal picture, float64 (3, 3):
    [[1/s, 0, cx (1 - 1/s)], [0, 1/s, cy (1 - 1/s)], [0, 0, 1]].  A fisheye's ideal picture at the source's own camera matrix
    shows only the middle of the view; s < 1 brings more of it into the frame's size.  undistort(lens_scale=s) warps with this
    map, rectify(lens_scale=s) with lens_scale_map(lens, s) @ M (lens_scale_compose); points of the scaled ideal picture go through it (homogeneous:
    p' = map @ (x, y, 1)) and then through lens_distort back onto the photograph.  lens: a Lens or a LensModel.  Needs no GPU."""
    s = _check_lens_scale("lens_scale_map", s)
    row = _lens_row(lens if lens is not None else Lens(1.0, 1.0, 0.0, 0.0), "lens_scale_map")
    cx, cy = row[2], row[3]
    q = 1.0 / s
    return np.array([[q, 0.0, cx * (1.0 - q)], [0.0, q, cy * (1.0 - q)], [0.0, 0.0, 1.0]], np.float64)


def lens_scale_compose(S, M):
    """lens_scale_map(lens, s) @ M as rectify(lens_scale=s) and the recipe compute it, every product and sum rounded on its
    own: rows q M[0] + tx M[2], q M[1] + ty M[2] and M[2], with q = S[0][0], tx = S[0][2], ty = S[1][2].  Needs no GPU."""
    S, M = np.asarray(S, np.float64).reshape(3, 3), np.asarray(M, np.float64).reshape(3, 3)
    return np.stack([S[0, 0] * M[0] + S[0, 2] * M[2], S[0, 0] * M[1] + S[1, 2] * M[2], M[2]])


_LensPlan = collections.namedtuple("_LensPlan", "rows maps")  # rectify_batch's lenses: _lens_rows' rows, and lens_scale_map per frame ((B, 3, 3)) or None for lens_scale 1


def _area_col(area, count, what):
    """float64 (count, 1): the sampling factors of `count` frames from area=: one integer from 1 to 8 for all, or a list of one per frame"""
    one = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and 1 <= int(v) <= 8  # noqa: E731
    if isinstance(area, (int, np.integer, bool, np.bool_, float, np.floating, str)):
        factors = [area] * count
    else:
        try:
            factors = list(area)
        except TypeError:
            raise ValueError("%s: area is an integer from 1 to 8 or a list of one per frame" % what) from None
        if len(factors) != count:
            raise ValueError("%s: as many sampling factors as frames (%d), not %d" % (what, count, len(factors)))
    if not all(one(v) for v in factors):
        raise ValueError("%s: a sampling factor (area=) is an integer from 1 to 8" % what)
    return np.array(factors, np.float64).reshape(count, 1)


def area_fine_map(M, S):
    """lr_area_fine_map of include/librectify_amd.h restated operation for operation in float64: LR_WARP_AREA's fine map F of
    the map M (3 x 3, destination to source) and the sampling factor S, the map of a picture S times as large whose pixel
    (S x + i, S y + j) is sub-sample (i, j) of destination pixel (x, y).  Returns float64 (3, 3).  Needs no GPU."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    S = int(S)
    if not 1 <= S <= 8:
        raise ValueError("area_fine_map: S is an integer from 1 to 8")
    F = np.zeros((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for k in range(3):
            F[k, 0] = M[k, 0] / np.float64(S)
            F[k, 1] = M[k, 1] / np.float64(S)
            F[k, 2] = M[k, 2] - ((M[k, 0] + M[k, 1]) * np.float64(S - 1)) / np.float64(2 * S)
    return F


def shrink_homography(H, M, out_size, max_size):
    """A rectified picture of bounded size (lr_shrink_homography of include/librectify_amd.h, restated operation for operation
    in float64; host only): H, M, out_size = (width, height) are what rectification_homography or crop_homography returned;
    either of H and M may be None.  Returns (H_out, M_out, (new_width, new_height), S): the warp with M_out into the new
    size, which is at most max_size on its longer side, with WARP_AREA and the sampling factor S (area=S) is the picture
    shrunk without aliasing.  A picture that fits already comes back as it is, with S = 1.  ValueError for what the header
    refuses."""
    f8 = np.float64
    try:
        h = None if H is None else np.array(H, f8).reshape(9)
        m = None if M is None else np.array(M, f8).reshape(9)
        ow, oh, max_size = int(out_size[0]), int(out_size[1]), int(max_size)
    except (TypeError, ValueError):
        raise ValueError("shrink_homography: H and M are 3 x 3 or None, out_size two integers and max_size one") from None
    if h is None and m is None:
        raise ValueError("shrink_homography: H and M are both None")
    if ow < 1 or oh < 1 or max_size < 1:
        raise ValueError("shrink_homography: a size or max_size below 1")
    if not all(v is None or np.isfinite(v).all() for v in (h, m)):
        raise ValueError("shrink_homography: a non-finite input")
    longer, nw, nh, S = max(ow, oh), ow, oh, 1
    if longer > max_size:
        nw, nh = max(1, ow * max_size // longer), max(1, oh * max_size // longer)
        sx, sy = f8(ow) / f8(nw), f8(oh) / f8(nh)
        tx, ty = (sx - f8(1.0)) / f8(2.0), (sy - f8(1.0)) / f8(2.0)
        with np.errstate(all="ignore"):
            if h is not None:
                for i in range(3):
                    h[i] = (h[i] - tx * h[6 + i]) / sx
                    h[3 + i] = (h[3 + i] - ty * h[6 + i]) / sy
            if m is not None:
                for k in range(3):
                    m0, m1 = m[3 * k], m[3 * k + 1]
                    m[3 * k] = m0 * sx
                    m[3 * k + 1] = m1 * sy
                    m[3 * k + 2] = m[3 * k + 2] + (m0 * tx + m1 * ty)
        S = min(8, int(np.ceil(max(sx, sy))))
    return (None if h is None else h.reshape(3, 3)), (None if m is None else m.reshape(3, 3)), (nw, nh), S


def _is_border_spec(border):
    return border is None or isinstance(border, str) or (isinstance(border, tuple) and len(border) == 2 and isinstance(border[0], str))


def _border_words(border, count, fmt, what):
    """the border words of `count` frames from border=: one spec for all, or a list of one spec per frame"""
    try:
        if _is_border_spec(border):
            return [border_word(border, fmt)] * count
        specs = list(border)
        if len(specs) != count:
            raise ValueError("border_word: as many borders as frames (%d), not %d" % (count, len(specs)))
        return [border_word(b, fmt) for b in specs]
    except ValueError as e:
        raise ValueError(str(e).replace("border_word", what)) from None
    except TypeError:
        raise ValueError('%s: border is None, a mode name, ("constant", value) or a list of those' % what) from None


_FMT_OF_BPP = {1: PIX_U8, 3: PIX_U8X3, 4: PIX_F32}


def crop_homography(H, M, width, height, out_size, margin=0, aspect=None):
    """The constrained crop of a rectified picture (lr_crop_homography of include/librectify_amd.h, restated operation for
    operation in float64; host only): the largest upright rectangle of the given aspect (width / height; None: the source's),
    centred on the image of the source's centre, that contains no border.  H, M, out_size: what rectification_homography
    returned for a source of width x height; margin: 0 for interp="linear", 1 for "cubic".  Returns (H_out, M_out, (x0, y0,
    crop_width, crop_height)): the warp with M_out into crop_width x crop_height is the crop.  Raises LibrectifyError whose
    `code` is the header's: 1 non-finite or absent input, 2 a source too small for the margin, 3 a denominator that is zero or
    changes sign, 4 a quadrilateral that is not strictly convex, 5 a crop below 1 x 1."""
    def fail(code, why):
        e = LibrectifyError("crop_homography: " + why)
        e.code = code
        raise e

    f8 = np.float64
    try:
        H = np.asarray(H, f8).reshape(9)
        M = np.asarray(M, f8).reshape(9)
        width, height, margin = int(width), int(height), int(margin)
        out_width, out_height = int(out_size[0]), int(out_size[1])
        aspect = f8(0.0 if aspect is None else aspect)
    except (TypeError, ValueError):
        fail(1, "H and M are 3 x 3, sizes and margin integers")
    if width < 1 or height < 1 or out_width < 1 or out_height < 1 or margin < 0:
        fail(1, "a size below 1 or a margin below 0")
    if not (np.isfinite(H).all() and np.isfinite(M).all() and np.isfinite(aspect)):
        fail(1, "a non-finite input")
    if width > 2 ** 30 or height > 2 ** 30 or margin > 2 ** 30:
        fail(1, "a size or margin above 2^30")
    if width - 1 - 2 * margin < 1 or height - 1 - 2 * margin < 1:
        fail(2, "the source is too small for the margin")
    a = aspect if aspect > 0.0 else f8(width) / f8(height)
    m = margin
    px = [f8(m), f8(width - 1 - m), f8(width - 1 - m), f8(m), f8(width - 1) / f8(2.0)]
    py = [f8(m), f8(m), f8(height - 1 - m), f8(height - 1 - m), f8(height - 1) / f8(2.0)]
    qx, qy, pos, neg = [], [], 0, 0
    with np.errstate(all="ignore"):
        for x, y in zip(px, py):
            d = (H[6] * x + H[7] * y) + H[8]
            if d > 0.0:
                pos += 1
            elif d < 0.0:
                neg += 1
            else:
                fail(3, "a zero denominator")
            qx.append(((H[0] * x + H[1] * y) + H[2]) / d)
            qy.append(((H[3] * x + H[4] * y) + H[5]) / d)
        if pos and neg:
            fail(3, "denominators of mixed sign")
        cx, cy = qx[4], qy[4]
        area2 = f8(0.0)
        for i in range(4):
            j = (i + 1) & 3
            area2 = area2 + (qx[i] * qy[j] - qx[j] * qy[i])
        if not np.isfinite(area2) or area2 == 0.0:
            fail(4, "the quadrilateral has no area")
        for i in range(4):
            j, k = (i + 1) & 3, (i + 2) & 3
            turn = (qx[j] - qx[i]) * (qy[k] - qy[j]) - (qy[j] - qy[i]) * (qx[k] - qx[j])
            if not (turn > 0.0 if area2 > 0.0 else turn < 0.0):
                fail(4, "the quadrilateral is not strictly convex")
        s = cx / a
        if (f8(out_width - 1) - cx) / a < s:
            s = (f8(out_width - 1) - cx) / a
        if cy < s:
            s = cy
        if f8(out_height - 1) - cy < s:
            s = f8(out_height - 1) - cy
        for i in range(4):
            j = (i + 1) & 3
            ex, ey = qx[j] - qx[i], qy[j] - qy[i]
            nx, ny = (-ey, ex) if area2 > 0.0 else (ey, -ex)
            den = abs(nx) * a + abs(ny)
            bound = (nx * (cx - qx[i]) + ny * (cy - qy[i])) / den
            if not bound >= s:
                s = bound
        if not s >= 0.0:
            fail(5, "the crop is below 1 x 1")
        lo_x, hi_x = np.ceil(cx - s * a), np.floor(cx + s * a)
        lo_y, hi_y = np.ceil(cy - s), np.floor(cy + s)
        if not (hi_x >= lo_x and hi_y >= lo_y) or lo_x < 0.0 or lo_y < 0.0 or hi_x > f8(out_width - 1) or hi_y > f8(out_height - 1):
            fail(5, "the crop is below 1 x 1")
        H_out, M_out = np.zeros(9, f8), np.zeros(9, f8)
        for i in range(3):
            H_out[i] = H[i] - lo_x * H[6 + i]
            H_out[3 + i] = H[3 + i] - lo_y * H[6 + i]
            H_out[6 + i] = H[6 + i]
            M_out[3 * i] = M[3 * i]
            M_out[3 * i + 1] = M[3 * i + 1]
            M_out[3 * i + 2] = (M[3 * i] * lo_x + M[3 * i + 1] * lo_y) + M[3 * i + 2]
    return H_out.reshape(3, 3), M_out.reshape(3, 3), (int(lo_x), int(lo_y), int(hi_x - lo_x) + 1, int(hi_y - lo_y) + 1)


def warp_table(Ms, sizes, bpp, align=4, border=None, lens=None, area=None):
    """The table of a packed warp (lr_warp_perspective_device with LR_WARP_PACKED) for frames laid out one after the
    other in frame order.  Ms: (B, 3, 3) destination-to-source maps; sizes: B pairs (out_width, out_height); bpp: bytes
    per pixel (1 u8, 3 u8x3, 4 f32); every row stride and every frame's start is rounded up to `align` bytes (for f32 a
    multiple of 4).  Returns (table, total_bytes): table float64 (B, 13) -- the map, width, height, byte offset, row
    stride -- and the bytes of the destination, which end with the last frame's last pixel.  Needs no GPU.
    border (not None): the table of LR_WARP_PACKED | LR_WARP_BORDER, (B, 14), whose column 13 is every frame's border word:
    one spec for all frames (border_word's) or a list of one per frame.
    lens (not None): the table of LR_WARP_PACKED | LR_WARP_LENS, (B, 22) or with border (B, 23), whose last nine columns are
    every frame's lens: one Lens for all frames or a list of one per frame, in which None means zeros.  With a LensModel for
    all frames or among the list's (Lens, LensModel and None mix) the columns are seventeen, (B, 30) or (B, 31): the table of
    LR_WARP_PACKED | LR_WARP_LENS | LR_WARP_LENS_MODEL.
    area (not None): the table of LR_WARP_PACKED | LR_WARP_AREA, one more column at the very end, every frame's sampling
    factor S: one integer from 1 to 8 for all frames or a list of one per frame."""
    Ms = np.asarray(Ms, np.float64)
    if Ms.ndim == 2 and Ms.shape == (3, 3):
        Ms = Ms[None]
    if Ms.ndim != 3 or Ms.shape[1:] != (3, 3):
        raise ValueError("warp_table: Ms is (B, 3, 3)")
    if not np.isfinite(Ms).all():
        raise ValueError("warp_table: M is not finite")
    sz = np.asarray(sizes)
    if sz.shape != (len(Ms), 2) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError("warp_table: sizes is B pairs of integers (out_width, out_height)")
    if len(sz) and int(sz.min()) < 1:
        raise ValueError("warp_table: an output size below 1")
    if bpp not in (1, 3, 4):
        raise ValueError("warp_table: bpp is 1, 3 or 4")
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or align < 1 or (bpp == 4 and align % 4):
        raise ValueError("warp_table: align is an integer >= 1, for f32 a multiple of 4")
    align = int(align)
    up = lambda v: (v + align - 1) // align * align  # noqa: E731
    table = np.zeros((len(Ms), 13), np.float64)
    table[:, :9] = Ms.reshape(-1, 9)
    end = 0
    for b, (ow, oh) in enumerate(sz.tolist()):
        start, row = up(end), up(ow * bpp)
        end = start + (oh - 1) * row + ow * bpp
        table[b, 9:] = (ow, oh, start, row)
    if end > 2 ** 53:
        raise ValueError("warp_table: the destination is larger than 2^53 bytes")
    if border is not None:
        words = _border_words(border, len(Ms), _FMT_OF_BPP[bpp], "warp_table")
        table = np.concatenate([table, np.array(words, np.float64).reshape(-1, 1)], axis=1)
    if lens is not None:  # (nine columns, or seventeen where a LensModel is given: WARP_LENS | WARP_LENS_MODEL)
        table = np.concatenate([table, _lens_rows(lens, len(Ms), "warp_table")], axis=1)
    if area is not None:
        table = np.concatenate([table, _area_col(area, len(Ms), "warp_table")], axis=1)
    return table, end


def ragged_table(Ms, out_sizes, sources, bpp, out_bpp=None, align=4, border=None, lens=None, area=None):
    """The table of a ragged call (lr_warp_perspective_device with LR_WARP_RAGGED): warp_table's layout for the outputs plus
    the four source columns.  Ms: (B, 3, 3) destination-to-source maps, or None (identity: the prepare step ignores them);
    out_sizes: B pairs (out_width, out_height); sources: B rows (width, height, byte_offset, row_bytes) of the frames in
    the source region; bpp: bytes per source pixel (1 u8, 3 u8x3, 4 f32); out_bpp: bytes per output pixel (default bpp;
    4 for the prepare step, whose output is f32 gray).  Outputs lie one after the other in frame order, every row stride
    and start rounded up to `align` bytes (a multiple of 4 for 4-byte outputs).  Returns (table, dst_bytes): table
    float64 (B, 18).  Needs no GPU.
    border (not None): the table of LR_WARP_RAGGED | LR_WARP_BORDER, whose column 17 is every frame's border word: one spec
    for all frames (border_word's) or a list of one per frame.
    lens (not None): the table of LR_WARP_RAGGED | LR_WARP_LENS, (B, 27), whose last nine columns are every frame's lens: one
    Lens for all frames or a list of one per frame, in which None means zeros.  With a LensModel for all frames or among the
    list's (Lens, LensModel and None mix) the columns are seventeen, (B, 35): LR_WARP_RAGGED | LR_WARP_LENS | LR_WARP_LENS_MODEL.
    area (not None): the table of LR_WARP_RAGGED | LR_WARP_AREA, (B, 19) or with lens (B, 28), whose last column is every
    frame's sampling factor S: one integer from 1 to 8 for all frames or a list of one per frame."""
    if bpp not in (1, 3, 4):
        raise ValueError("ragged_table: bpp is 1, 3 or 4")
    out_bpp = bpp if out_bpp is None else out_bpp
    if out_bpp not in (1, 3, 4):
        raise ValueError("ragged_table: out_bpp is 1, 3 or 4")
    src = np.asarray(sources)
    if src.ndim != 2 or src.shape[1] != 4 or not np.issubdtype(src.dtype, np.integer):
        raise ValueError("ragged_table: sources is B rows of integers (width, height, byte_offset, row_bytes)")
    B = len(src)
    if Ms is None:
        Ms = np.broadcast_to(np.eye(3), (B, 3, 3))
    try:
        packed, total = warp_table(Ms, out_sizes, out_bpp, align)
    except ValueError as e:
        raise ValueError(str(e).replace("warp_table", "ragged_table")) from None
    if len(packed) != B:
        raise ValueError("ragged_table: as many sources as maps")
    for w, h, off, row in src.tolist():
        if w < 1 or h < 1:
            raise ValueError("ragged_table: a source size below 1")
        if off < 0 or row < w * bpp:
            raise ValueError("ragged_table: a source offset below 0 or a row stride shorter than a row")
        if bpp == 4 and (off % 4 or row % 4):
            raise ValueError("ragged_table: f32 source offsets and strides are multiples of 4")
        if off + (h - 1) * row + w * bpp > 2 ** 53:
            raise ValueError("ragged_table: the source region is larger than 2^53 bytes")
    table = np.zeros((B, 18), np.float64)
    table[:, :13] = packed
    table[:, 13:17] = src
    if border is not None:
        table[:, 17] = _border_words(border, B, _FMT_OF_BPP[bpp], "ragged_table")
    if lens is not None:  # (nine columns, or seventeen where a LensModel is given: WARP_LENS | WARP_LENS_MODEL)
        table = np.concatenate([table, _lens_rows(lens, B, "ragged_table")], axis=1)
    if area is not None:
        table = np.concatenate([table, _area_col(area, B, "ragged_table")], axis=1)
    return table, total


def draw_table(sizes, sources, outputs, segments):
    """The table of lr_draw_lines_device: sizes: B pairs (width, height); sources: B pairs (byte_offset, row_bytes) of the
    frames in the source region, or None (in place: zeros); outputs: B pairs (byte_offset, row_bytes) of the u8x3 outputs
    in the destination region; segments: B pairs (first, count) into the lines array.  Returns float64 (B, 8): width,
    height, source offset and stride, output offset and stride, first segment and count.  Needs no GPU."""
    sz = np.asarray(sizes)
    if sz.ndim != 2 or sz.shape[1] != 2 or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError("draw_table: sizes is B pairs of integers (width, height)")
    B = len(sz)
    cols = [sz]
    for name, a in (("sources", sources), ("outputs", outputs), ("segments", segments)):
        a = np.zeros((B, 2), np.int64) if a is None and name == "sources" else np.asarray(a)
        if a.shape != (B, 2) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("draw_table: %s is B pairs of integers" % name)
        cols.append(a)
    table = np.concatenate([c.astype(np.int64) for c in cols], axis=1)
    if B and (table.min() < 0 or table.max() > 2 ** 53):
        raise ValueError("draw_table: an entry below 0 or above 2^53")
    if B and int(sz.min()) < 1:
        raise ValueError("draw_table: a size below 1")
    return table.astype(np.float64)


def jpeg_bound(width, height, fmt, layout=0, optimize=False):
    """lr_jpeg_bound: the longest stream lr_encode_jpeg_device can produce for a width x height frame of format fmt (PIX_U8,
    PIX_U8X3) and chroma layout (0 = 4:2:0, 1 = 4:4:4; 0 for PIX_U8): 416 bytes a block (1660 bits of code, every byte
    stuffed), 2 per restart interval, 640 for the headers and the EOI.  0 for a size outside 1 .. 65535 or another format.
    optimize=True (LR_JPEG_OPTIMIZE): 418 bytes a block, a DC code of the frame's own tables having up to 16 bits (1665)."""
    width, height = int(width), int(height)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        return 0
    if fmt == PIX_U8 and layout == 0:
        mcu, bpm, ri = 8, 1, 96
    elif fmt == PIX_U8X3 and layout == 0:
        mcu, bpm, ri = 16, 6, 16
    elif fmt == PIX_U8X3 and layout == 1:
        mcu, bpm, ri = 8, 3, 32
    else:
        return 0
    mcus = ((width + mcu - 1) // mcu) * ((height + mcu - 1) // mcu)
    return 640 + 2 * ((mcus + ri - 1) // ri) + (418 if optimize else 416) * mcus * bpm


def jpeg_table(sizes, sources, outputs, quality, layout=0, optimize=False):
    """The table of lr_encode_jpeg_device: sizes: B pairs (width, height); sources: B pairs (byte_offset, row_bytes) of the
    frames in the source region; outputs: B pairs (byte_offset, capacity) of the streams' extents in the destination
    region; quality (1 .. 100) and layout (0 = 4:2:0, 1 = 4:4:4): one value for all frames, or B values; optimize: one bool
    or B of them, the frames whose streams get Huffman tables of their own (JPEG_OPTIMIZE added to their [7]).  Returns float64
    (B, 8).  Rejects what can be seen without the regions: sizes outside 1 .. 65535, entries below 0 or above 2^53, a
    quality outside 1 .. 100, a layout other than 0 or 1, extents that overlap.  Needs no GPU."""
    sz = np.asarray(sizes)
    if sz.ndim != 2 or sz.shape[1] != 2 or not np.issubdtype(sz.dtype, np.integer) or len(sz) < 1:
        raise ValueError("jpeg_table: sizes is B pairs of integers (width, height), B >= 1")
    B = len(sz)
    cols = [sz]
    for name, a in (("sources", sources), ("outputs", outputs)):
        a = np.asarray(a)
        if a.shape != (B, 2) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("jpeg_table: %s is B pairs of integers" % name)
        cols.append(a)
    for name, a in (("quality", quality), ("layout", layout)):
        a = np.asarray(a)
        if not np.issubdtype(a.dtype, np.integer) or a.shape not in ((), (B,)):
            raise ValueError("jpeg_table: %s is an integer, or B integers" % name)
        cols.append(np.broadcast_to(a, (B,)).reshape(B, 1))
    table = np.concatenate([c.astype(np.int64) for c in cols], axis=1)
    if table.min() < 0 or table.max() > 2 ** 53:
        raise ValueError("jpeg_table: an entry below 0 or above 2^53")
    if int(sz.min()) < 1 or int(sz.max()) > 65535:
        raise ValueError("jpeg_table: a size outside 1 .. 65535")
    if int(table[:, 6].min()) < 1 or int(table[:, 6].max()) > 100:
        raise ValueError("jpeg_table: a quality outside 1 .. 100")
    if int(table[:, 7].max()) > 1:
        raise ValueError("jpeg_table: a layout other than 0 (4:2:0) or 1 (4:4:4)")
    ext = sorted((int(o), int(o) + int(c)) for o, c in table[:, 4:6].tolist())
    if any(b[0] < a[1] for a, b in zip(ext, ext[1:])):
        raise ValueError("jpeg_table: two frames' extents overlap")
    opt = np.asarray(optimize)
    if opt.dtype != np.bool_ or opt.shape not in ((), (B,)):
        raise ValueError("jpeg_table: optimize is True, False or B of them")
    table[:, 7] += JPEG_OPTIMIZE * np.broadcast_to(opt, (B,)).astype(np.int64)
    return table.astype(np.float64)


def _three(v, what):
    a = np.asarray(v, np.float64)
    if a.shape not in ((), (3,)):
        raise ValueError("TensorSpec: %s is one number or three" % what)
    return np.broadcast_to(a, (3,)).astype(np.float64)


class TensorSpec:
    """What lr_pack_tensor_device makes of 8-bit pictures (lr_tensor_args without the frame table): size = (H, W) of a slot;
    dtype "f32", "f16" or "bf16"; layout "nchw" or "nhwc"; mean and std per channel (one number or three) in units of 1,
    torchvision's ToTensor followed by Normalize as TWO operations: scale_c = 1.0 / (255.0 * std_c) and bias_c = -mean_c /
    std_c in float64, so that an element is (float)(v * scale_c + bias_c); scale= / bias= give the two directly instead;
    pad: the LEVEL (integer 0 .. 255, one or three) of elements outside the picture; bgr: channel c comes from source channel
    2 - c (LR_TENSOR_SWAP); gray3: a gray source into three channels (LR_TENSOR_GRAY3); place: "center" or "topleft", where
    tensor_table puts a picture in its slot.  Needs no GPU."""
    _DTYPES = {"f32": (TENSOR_F32, np.float32), "f16": (TENSOR_F16, np.float16), "bf16": (TENSOR_BF16, np.uint16)}
    _LAYOUTS = {"nchw": TENSOR_NCHW, "nhwc": TENSOR_NHWC}

    def __init__(self, size, dtype="f32", layout="nchw", mean=(0, 0, 0), std=(1, 1, 1), pad=0, bgr=False, gray3=False,
                 place="center", scale=None, bias=None):
        try:
            self.height, self.width = int(size[0]), int(size[1])
            ok = len(size) == 2 and self.height == size[0] and self.width == size[1]
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok or self.height < 1 or self.width < 1 or max(self.height, self.width) > 2 ** 30:
            raise ValueError("TensorSpec: size is (H, W), two integers from 1 to 2^30")
        if dtype not in self._DTYPES:
            raise ValueError('TensorSpec: dtype is "f32", "f16" or "bf16"')
        if layout not in self._LAYOUTS:
            raise ValueError('TensorSpec: layout is "nchw" or "nhwc"')
        if place not in ("center", "topleft"):
            raise ValueError('TensorSpec: place is "center" or "topleft"')
        self.size, self.dtype, self.layout, self.place = (self.height, self.width), dtype, layout, place
        self.bgr, self.gray3 = bool(bgr), bool(gray3)
        mean, std = _three(mean, "mean"), _three(std, "std")
        if not (np.isfinite(mean).all() and np.isfinite(std).all()) or (std == 0).any():
            raise ValueError("TensorSpec: mean and std are finite, std not 0")
        self.scale = np.float64(1.0) / (np.float64(255.0) * std) if scale is None else _three(scale, "scale")
        self.bias = -mean / std if bias is None else _three(bias, "bias")
        if not (np.isfinite(self.scale).all() and np.isfinite(self.bias).all()):
            raise ValueError("TensorSpec: a non-finite scale or bias")
        pad = _three(pad, "pad")
        if not (np.isfinite(pad).all() and (pad == np.floor(pad)).all() and pad.min() >= 0 and pad.max() <= 255):
            raise ValueError("TensorSpec: pad is an integer level from 0 to 255, one or three")
        self.pad = pad

    @property
    def np_dtype(self):
        """The NumPy type of the tensor's elements (uint16 bit patterns for "bf16")"""
        return self._DTYPES[self.dtype][1]

    def channels(self, fmt):
        """C for a source of format fmt (PIX_U8, PIX_U8X3); ValueError for what the header refuses"""
        if fmt not in (PIX_U8, PIX_U8X3):
            raise ValueError("TensorSpec: the source is PIX_U8 or PIX_U8X3")
        if self.gray3 and fmt != PIX_U8:
            raise ValueError("TensorSpec: gray3 takes a gray source (PIX_U8)")
        C_ = 3 if (fmt == PIX_U8X3 or self.gray3) else 1
        if self.bgr and C_ == 1:
            raise ValueError("TensorSpec: bgr needs three channels")
        return C_

    def shape(self, n, fmt):
        """The tensor's shape for n slots and a source of format fmt"""
        C_ = self.channels(fmt)
        return (n, C_, self.height, self.width) if self.layout == "nchw" else (n, self.height, self.width, C_)

    def args(self, table, n):
        """lr_tensor_args for a frame table (which must stay alive during the call) and n slots"""
        return TensorArgs(_ptr(table), n, self.height, self.width, self._DTYPES[self.dtype][0], self._LAYOUTS[self.layout],
                          (TENSOR_SWAP if self.bgr else 0) | (TENSOR_GRAY3 if self.gray3 else 0),
                          (C.c_double * 3)(*self.scale.tolist()), (C.c_double * 3)(*self.bias.tolist()), (C.c_double * 3)(*self.pad.tolist()))


def fit_box(out_size, box):
    """The bound N for which shrink_homography makes a picture of out_size = (ow, oh) fit a box = (W, H): the largest integer
    N <= max(ow, oh) whose size rule (max(1, ow * N // longer), max(1, oh * N // longer)) lies inside W x H.  A picture that
    fits already gives N = max(ow, oh): pictures are never enlarged.  Integer arithmetic only.
    (ow * N // longer <= W exactly when N <= ((W + 1) * longer - 1) // ow.)"""
    ow, oh, W, H = int(out_size[0]), int(out_size[1]), int(box[0]), int(box[1])
    if ow < 1 or oh < 1 or W < 1 or H < 1:
        raise ValueError("fit_box: a size below 1")
    longer = max(ow, oh)
    return min(longer, ((W + 1) * longer - 1) // ow, ((H + 1) * longer - 1) // oh)


def tensor_table(sizes, sources, slots, spec):
    """The table of lr_pack_tensor_device: sizes: B pairs (width, height) of the pictures; sources: B pairs (byte_offset,
    row_bytes) of the pictures in the source region; slots: B slot numbers, no two alike; spec: the TensorSpec, whose place
    puts a picture in its slot ("center": left = (W - w) // 2, top = (H - h) // 2; "topleft": 0, 0).  Returns float64 (B, 8):
    width, height, source offset and stride, slot, left, top, 0.  Rejects what can be seen without the regions: a picture
    below 1 or larger than the slot, entries below 0 or above 2^53, a slot named twice.  Needs no GPU."""
    sz = np.asarray(sizes)
    if sz.ndim != 2 or sz.shape[1] != 2 or not np.issubdtype(sz.dtype, np.integer) or len(sz) < 1:
        raise ValueError("tensor_table: sizes is B pairs of integers (width, height), B >= 1")
    B = len(sz)
    src, sl = np.asarray(sources), np.asarray(slots)
    if src.shape != (B, 2) or not np.issubdtype(src.dtype, np.integer):
        raise ValueError("tensor_table: sources is B pairs of integers")
    if sl.shape != (B,) or not np.issubdtype(sl.dtype, np.integer):
        raise ValueError("tensor_table: slots is B integers")
    sz, src, sl = sz.astype(np.int64), src.astype(np.int64), sl.astype(np.int64)
    if min(int(src.min()), int(sl.min())) < 0 or max(int(src.max()), int(sl.max())) > 2 ** 53:
        raise ValueError("tensor_table: an entry below 0 or above 2^53")
    if int(sz.min()) < 1:
        raise ValueError("tensor_table: a size below 1")
    if int(sz[:, 0].max()) > spec.width or int(sz[:, 1].max()) > spec.height:
        raise ValueError("tensor_table: a picture larger than the slot")
    if len(set(sl.tolist())) != B:
        raise ValueError("tensor_table: two frames in one slot")
    table = np.zeros((B, 8), np.int64)
    table[:, 0:2], table[:, 2:4], table[:, 4] = sz, src, sl
    if spec.place == "center":
        table[:, 5], table[:, 6] = (spec.width - sz[:, 0]) // 2, (spec.height - sz[:, 1]) // 2
    return table.astype(np.float64)


def tensor_map(M, left, top):
    """The tensor map of a picture that the warp wrote with the destination-to-source map M (3 x 3) and that lies at (left,
    top) of its slot: the map from a tensor pixel (x, y) of the slot to the coordinates the warp read from, M composed with
    the translation by (-left, -top).  float64."""
    T = np.array([[1.0, 0.0, -float(left)], [0.0, 1.0, -float(top)], [0.0, 0.0, 1.0]], np.float64)
    return np.asarray(M, np.float64).reshape(3, 3) @ T


def jpeg_decode_table(streams, outputs=None, sizes=None, orient=False, scale=None):
    """The table of lr_decode_jpeg_device: streams: B pairs (byte_offset, length) of the streams in the source region;
    outputs: B pairs (byte_offset, row_bytes) of the pictures in the destination region; sizes: B pairs (width, height)
    the caller allocated for.  outputs and sizes None: probe mode's table (zeros).  orient: True, False or B of them:
    entry [7], the file's EXIF orientation is applied (sizes are then those of the upright picture, as probe mode with
    the same orient tells them).  scale: None, or an int or B ints out of 1, 2, 4, 8: entry [6], the frame's scale
    denominator for a call that carries JPEG_SCALED (sizes are then those of the reduced picture, ceil(w / N) x ceil(h / N),
    as probe mode with the same scale tells them); None leaves [6] 0.  Returns float64 (B, 8).  Rejects what can be seen without the regions: entries below 0
    or above 2^53, a length of 2^31 - 16 or more, sizes outside 1 .. 65535.  Needs no GPU."""
    st = np.asarray(streams)
    if st.ndim != 2 or st.shape[1] != 2 or not np.issubdtype(st.dtype, np.integer) or len(st) < 1:
        raise ValueError("jpeg_decode_table: streams is B pairs of integers (byte_offset, length), B >= 1")
    B = len(st)
    if (outputs is None) != (sizes is None):
        raise ValueError("jpeg_decode_table: outputs and sizes go together")
    cols = [st]
    for name, a in (("outputs", outputs), ("sizes", sizes)):
        a = np.zeros((B, 2), np.int64) if a is None else np.asarray(a)
        if a.shape != (B, 2) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("jpeg_decode_table: %s is B pairs of integers" % name)
        cols.append(a)
    flags = np.asarray(orient)
    if flags.dtype != np.bool_ or flags.shape not in ((), (B,)):
        raise ValueError("jpeg_decode_table: orient is True, False or B of them")
    table = np.concatenate([c.astype(np.int64) for c in cols] + [np.zeros((B, 2), np.int64)], axis=1)
    table[:, 7] = flags
    if scale is not None:
        table[:, 6] = _scales(scale, B, "jpeg_decode_table")
    if table.min() < 0 or table.max() > 2 ** 53:
        raise ValueError("jpeg_decode_table: an entry below 0 or above 2^53")
    if int(table[:, 1].max()) > 2 ** 31 - 16:
        raise ValueError("jpeg_decode_table: a stream longer than 2^31 - 16 bytes")
    if sizes is not None and (int(table[:, 4:6].min()) < 1 or int(table[:, 4:6].max()) > 65535):
        raise ValueError("jpeg_decode_table: a size outside 1 .. 65535")
    return table.astype(np.float64)


def _stream_region(streams):
    """(the streams one behind the other as uint8, their (byte_offset, length) pairs)"""
    streams = [bytes(s) for s in streams]
    if not streams:
        raise ValueError("no streams")
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    region = np.frombuffer(b"".join(streams) or b"\0", np.uint8)
    return np.ascontiguousarray(region), np.stack([offs, lens], axis=1)


def _decode_call(handle, d_src, region, fmt, table, d_dst, dst_bytes):
    table = np.ascontiguousarray(table, np.float64)
    if table.ndim != 2 or table.shape[1] != 8 or len(table) < 1:
        raise ValueError("decode_jpeg_device: the table has 8 values per frame")
    region = np.ascontiguousarray(region, np.uint8)
    info = np.zeros((len(table), 8), np.int32)
    args = JpegDecodeArgs(_ptr(region), _ptr(table), _ptr(info))
    _check(lib().lr_warp_perspective_device(handle, C.c_void_p(d_src) if d_src else None, region.nbytes, len(table), 0, 0, 0,
                                            fmt | WARP_JPEG_DECODE, C.cast(C.byref(args), C.c_void_p),
                                            C.c_void_p(d_dst) if d_dst else None, dst_bytes, 0, 0, 0))
    return info


def _scales(scale, B, what):
    """scale= as B scale denominators"""
    n = np.asarray(scale)
    if not np.issubdtype(n.dtype, np.integer) or n.shape not in ((), (B,)) or not np.isin(n, (1, 2, 4, 8)).all():
        raise ValueError(what + ": scale is None, or one or B of 1, 2, 4, 8")
    return np.broadcast_to(n, (B,)).astype(np.int64)


def _scaled_bit(scale):
    return 0 if scale is None else JPEG_SCALED


def jpeg_scale_for(sizes, max_size):
    """decode_max_size's choice (PIL's Image.draft rule): per (width, height) the largest N of 1, 2, 4, 8 whose reduced
    picture's longer side, ceil(max(w, h) / N), is still at least max_size; 1 if none is"""
    if int(max_size) != max_size or max_size < 1:
        raise ValueError("decode_max_size is an integer of at least 1")
    return [max([1] + [n for n in (2, 4, 8) if -(-max(int(w), int(h)) // n) >= max_size]) for w, h in sizes]


def jpeg_info(streams, orient=False, any_sampling=False, scale=None):
    """lr_jpeg_info (lr_decode_jpeg_device's probe mode): of every JPEG file in the list (bytes) width, height, components,
    layout (0 = 4:2:0 or one component, 1 = 4:4:4, 2 = 4:2:2), restart interval and status (JPEG_OK, ...), from the headers
    alone.  orient=True: width and height are the upright picture's (swapped for the EXIF orientations 5 .. 8) and the
    last column is the orientation, 1 .. 8 (1: the file tells none).  any_sampling=True (LR_JPEG_ANY_SAMPLING): a
    three-component file of any sampling with factors 1, 2 or 4, the luminance's the largest and at most 10 blocks to the
    MCU, is status 0 as well, its layout column being the luminance's sampling byte (0x12 = 18 for 4:4:0, 0x41 = 65 for
    4:1:1).  scale (None, an int or B ints out of 1, 2, 4, 8; LR_JPEG_SCALED): width and height are those of the picture
    reduced to 1/N, ceil(w / N) x ceil(h / N), what a decode with the same scale writes.  Returns int32 (B, 8).  No
    context, no GPU."""
    region, extents = _stream_region(streams)
    return _decode_call(None, None, region, PIX_U8X3 | _any_sampling_bit(any_sampling) | _scaled_bit(scale),
                        jpeg_decode_table(extents, orient=orient, scale=scale), None, 0)


def _any_sampling_bit(any_sampling):
    return JPEG_ANY_SAMPLING if any_sampling else 0


def _check_jpeg_optimize(what, jpeg, jpeg_optimize):
    if jpeg_optimize and jpeg is None:
        raise ValueError(what + ": jpeg_optimize=True goes with jpeg=Q; without it nothing is encoded")


def _all_streams(frames, what, orient=False, any_sampling=False, decode_scale=None, decode_max_size=None):
    """True if `frames` is a list of JPEG files (bytes), False if it holds none; a mixture is refused, and so are orient
    with arrays, which carry no EXIF tag, any_sampling with arrays, which have no sampling, and decode_scale or
    decode_max_size with arrays, which are not decoded (and the two together)"""
    n = sum(isinstance(f, (bytes, bytearray, memoryview)) for f in frames) if isinstance(frames, (list, tuple)) else 0
    if n and n != len(frames):
        raise ValueError(what + ": the list is all JPEG files (bytes) or all arrays")
    if orient and not n:
        raise ValueError(what + ": orient=True goes with JPEG files (bytes); arrays carry no EXIF orientation")
    if any_sampling and not n:
        raise ValueError(what + ": any_sampling=True goes with JPEG files (bytes); arrays have no chroma sampling")
    if decode_scale is not None and decode_max_size is not None:
        raise ValueError(what + ": decode_scale and decode_max_size are two ways to say one thing; give one")
    if (decode_scale is not None or decode_max_size is not None) and not n:
        raise ValueError(what + ": decode_scale and decode_max_size go with JPEG files (bytes); arrays are not decoded")
    return n > 0


def _source_extent(sources, bpp):
    """bytes of the region that holds the sources (width, height, byte_offset, row_bytes)"""
    return max(off + (h - 1) * row + w * bpp for w, h, off, row in sources)


def _sampling_bit(interp, what):
    """the format word's bit for interp= of the calls that end in a warp: WARP_CUBIC for "cubic", 0 for "linear" (anything else: ValueError)"""
    if isinstance(interp, str) and interp in ("linear", "cubic"):
        return WARP_CUBIC if interp == "cubic" else 0
    raise ValueError('%s: interp is "linear" or "cubic", not %r' % (what, interp))


def _frame_format(a, what):
    """(format, bytes per pixel) of one 8-bit or f32 frame as the warp and the prepare step take it"""
    if a.dtype == np.uint8 and a.ndim == 2:
        return PIX_U8, 1
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        return PIX_U8X3, 3
    if a.dtype == np.float32 and a.ndim == 2:
        return PIX_F32, 4
    raise ValueError(what + ": a 2-D uint8 or float32 frame, or an H x W x 3 uint8 frame")


def _host_frame(a, what):
    """a host frame as the detector's entries take it: (array, format, bytes per pixel, stride in pixels); float32 for
    everything that is not uint8, as ever"""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        a = np.asarray(a, np.float32)
    fmt, bpp = _frame_format(a, what)
    if fmt == PIX_U8X3:
        assert a.strides[2] == 1 and a.strides[1] == 3 and a.strides[0] % 3 == 0
    else:
        assert a.strides[1] == bpp and a.strides[0] % bpp == 0
    return a, fmt, bpp, a.strides[0] // bpp


def _rectified_map(t, clip, crop, cubic):
    """(M, (out_width, out_height), crop rectangle or None) of a frame's transform: rectification_homography, and with crop
    the constrained crop's map and size (crop_homography; margin 1 for the bicubic rule)"""
    H, M, size = rectification_homography(t, clip)
    if not crop:
        return M, size, None
    _, M, rect = crop_homography(H, M, int(t.width), int(t.height), size, 1 if cubic else 0)
    return M, rect[2:], rect


def _bounded_map(M, size, out_max_size):
    """(M, size, S) of a rectified picture with out_max_size= of the rectify calls: shrink_homography's map, size and sampling
    factor (None: the picture as it is, S None)"""
    if out_max_size is None:
        return M, size, None
    if isinstance(out_max_size, _FitBox):  # (tensor= of the rectify calls: the bound is the frame's own, fit_box of its size)
        out_max_size = fit_box(size, out_max_size)
    _, M, size, S = shrink_homography(None, M, size, out_max_size)
    return M, size, S


_FitBox = collections.namedtuple("_FitBox", "width height")  # in place of out_max_size inside the rectify calls: a box (W, H) that bounds every frame by fit_box


def _check_tensor(what, tensor, tensor_out, out_max_size):
    """tensor= and tensor_out= of the rectify calls: the bound that stands in for out_max_size (None without tensor=)"""
    if tensor is None:
        if tensor_out is not None:
            raise ValueError("%s: tensor_out goes with tensor=" % what)
        return out_max_size
    if not isinstance(tensor, TensorSpec):
        raise ValueError("%s: tensor is a TensorSpec" % what)
    if out_max_size is not None:
        raise ValueError("%s: out_max_size together with tensor= (the tensor's box is the bound)" % what)
    return _FitBox(tensor.width, tensor.height)


def _check_out_max_size(what, out_max_size):
    if isinstance(out_max_size, _FitBox):
        return
    if out_max_size is not None and (isinstance(out_max_size, (bool, np.bool_)) or not isinstance(out_max_size, (int, np.integer)) or out_max_size < 1):
        raise ValueError("%s: out_max_size is None or an integer >= 1" % what)


def _border_bit_and_map(border, fmt, M, what, lens=None, area=None):
    """(WARP_BORDER, WARP_LENS, WARP_AREA or 0, M or M's nine values with the border word, the nine lens entries and the
    sampling factor behind them) for a single-frame warp with border=, lens= and area="""
    if border is None and lens is None and area is None:
        return 0, M
    row, bits = [np.asarray(M, np.float64).reshape(9)], 0
    if border is not None:
        row.append([float(_border_words(border, 1, fmt, what)[0])])
        bits |= WARP_BORDER
    if lens is not None:
        rows = _lens_rows(lens, 1, what)
        row.append(rows[0])
        bits |= _lens_bits(rows)
    if area is not None:
        row.append(_area_col(area, 1, what)[0])
        bits |= WARP_AREA
    return bits, np.concatenate(row)


class Context:
    """One device, one stream, one workspace (include/librectify_amd.h)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().lr_context_create(device, C.byref(self._h)))
        self.device = device
        self.shape = None

    def close(self):
        if self._h:
            lib().lr_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_seed(self, seed):
        lib().lr_set_ransac_seed(self._h, C.c_uint64(seed))

    def set_iterations(self, n):
        lib().lr_set_ransac_iterations(self._h, int(n))

    def set_flood_mode(self, mode):
        lib().lr_set_flood_mode(self._h, int(mode))

    def synchronize(self):
        _check(lib().lr_synchronize(self._h))

    # ---- stage API ----
    def stage_filter_host(self, img):
        img = np.ascontiguousarray(img, np.float32)
        h, w = img.shape
        self.shape = (h, w)
        _check(lib().lr_stage_filter_host(self._h, _ptr(img), w, h, w))

    def stage_filter_device(self, dptr, w, h, stride=None):
        self.shape = (h, w)
        _check(lib().lr_stage_filter(self._h, C.c_void_p(dptr), w, h, stride or w))

    def stage_seeds(self):
        n = C.c_int(0)
        _check(lib().lr_stage_seeds(self._h, C.byref(n)))
        self.n_seeds = n.value
        return n.value

    def stage_flood(self):
        n = C.c_int(0)
        _check(lib().lr_stage_flood(self._h, C.byref(n)))

    def stage_fit(self):
        h, w = self.shape
        cap = h * w // 6 + 16
        out = np.zeros(cap, LINE_DTYPE)
        n = C.c_int(0)
        _check(lib().lr_stage_fit(self._h, _ptr(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def download(self, buf):
        h, w = self.shape
        if buf in (BUF_DX, BUF_DY):
            a = np.zeros((h, w), np.float32)
        elif buf == BUF_DMASK:
            a = np.zeros((h, w), np.uint8)
        elif buf == BUF_LABEL:
            a = np.zeros((h, w), np.int32)
        elif buf in (BUF_SEED_IDX, BUF_SEED_BIN, BUF_SEED_SIZE):
            a = np.zeros(self.n_seeds, np.int32)
        elif buf == BUF_SEED_THR:
            a = np.zeros(self.n_seeds, np.float32)
        elif buf == BUF_MAXMAG:
            a = np.zeros(1, np.float32)
        elif buf == BUF_SEED_REC:
            a = np.zeros((self.n_seeds, 4), np.uint32)
        elif buf == BUF_COUNTS:
            a = np.zeros(16, np.uint32)
        else:
            raise ValueError(buf)
        if a.nbytes:
            _check(lib().lr_download(self._h, buf, _ptr(a), a.nbytes))
        return a

    def stage_times(self):
        t = np.zeros(T_COUNT, np.float32)
        _check(lib().lr_stage_times(self._h, _ptr(t), T_COUNT))
        return t

    def stage_times_partial(self):
        """ms of the last filter kernel alone (valid right after stage_filter_*)."""
        ms = C.c_float(0)
        _check(lib().lr_filter_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def stage_counters(self):
        c = np.zeros(16, np.int64)
        _check(lib().lr_stage_counters(self._h, _ptr(c), 16))
        return dict(seeds=int(c[0]), components=int(c[1]), flood_rounds=int(c[2]), labelled_px=int(c[3]),
                    second_tier_seeds=int(c[4]), slabs=int(c[5]), ordered_tail_seeds=int(c[6]), frame_laps=int(c[7]),
                    walked_px=int(c[8]), walk_steps=int(c[9]), scheduled_rounds=int(c[10]), log_rewalks=int(c[11]), log_give_ups=int(c[12]), giants_held=int(c[13]), giant_steps=int(c[14]),
                    quiet_round_misses=int(c[15]))

    # ---- full path ----
    def find_line_segment_groups(self, img, min_length, refine=False, num_threads=-1, capacity=None):
        """img: 2-D float32 numpy array (host), or an 8-bit frame: 2-D uint8, or H x W x 3 uint8 (interleaved; the
        detector runs on luma / 256, exactly what it gives on that float32 frame)."""
        img, fmt, _, stride = _host_frame(img, "find_line_segment_groups")
        h, w = img.shape[:2]
        cap = capacity or (h * w // 6 + 16)
        out = np.zeros(cap, LINE_DTYPE)
        n = C.c_int(0)
        self.shape = (h, w)
        _check(lib().lr_find_line_segment_groups_host(self._h, _ptr(img), w, h, stride, min_length, frames_word(fmt, refine), num_threads, _ptr(out), cap, C.byref(n)))
        return out[: min(n.value, cap)].copy()

    def find_line_segment_groups_device(self, dptr, w, h, min_length, refine=False, stride=None, capacity=None, out=None, fmt=PIX_F32):
        """fmt: the resident frame's format (PIX_F32, PIX_U8, PIX_U8X3); stride in pixels of it"""
        cap = capacity or (h * w // 6 + 16)
        if out is None:
            out = np.zeros(cap, LINE_DTYPE)
        n = C.c_int(0)
        self.shape = (h, w)
        _check(lib().lr_find_line_segment_groups_device(self._h, C.c_void_p(dptr), w, h, stride or w, min_length, frames_word(fmt, refine), -1, _ptr(out), cap, C.byref(n)))
        return out[: min(n.value, cap)]

    def device_upload(self, array):
        """Copies a contiguous numpy array to a fresh device buffer; returns its address (free with device_free)."""
        a = np.ascontiguousarray(array)
        p = C.c_void_p()
        _check(lib().lr_device_malloc(self._h, a.nbytes, C.byref(p)))
        _check(lib().lr_memcpy_h2d(self._h, p, _ptr(a), a.nbytes))
        return p.value

    def device_free(self, ptr):
        _check(lib().lr_device_free(self._h, C.c_void_p(ptr)))

    def device_download(self, ptr, shape, dtype):
        """Copies a device buffer into a new numpy array of that shape and dtype, once the context's stream is done."""
        a = np.empty(shape, dtype)
        if a.nbytes:
            _check(lib().lr_memcpy_d2h(self._h, _ptr(a), C.c_void_p(ptr), a.nbytes))
        return a

    # ---- rectified images ----
    def warp_perspective_device(self, d_src, src_image_bytes, batch, width, height, src_row_bytes, fmt, M, d_dst,
                                dst_image_bytes, out_width, out_height, dst_row_bytes):
        """lr_warp_perspective_device: one launch for `batch` device frames, enqueued on the context's stream.  M: 9
        doubles per frame ((batch, 3, 3) or (3, 3)), the destination-to-source map.  fmt: PIX_U8, PIX_U8X3, PIX_F32, with
        WARP_CUBIC or-ed in for the bicubic sampling rule and WARP_BORDER for a border rule per frame (M then has 10 doubles
        per frame, the tenth the frame's border_word), and WARP_LENS for a lens per frame (nine more doubles per frame at the
        end: a Lens; seventeen with WARP_LENS_MODEL as well: a LensModel), and WARP_AREA for S x S samples per destination pixel (one more double at the very end of every frame's
        row: its sampling factor S, 1 .. 8)."""
        M = np.ascontiguousarray(M, np.float64).reshape(-1)
        per_frame = (10 if fmt & WARP_BORDER else 9) + ((17 if fmt & WARP_LENS_MODEL else 9) if fmt & WARP_LENS else 0) + (1 if fmt & WARP_AREA else 0)
        if M.size < per_frame * max(int(batch), 1):
            raise ValueError("warp_perspective_device: M needs %d values per frame" % per_frame)
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_image_bytes, batch, width, height, src_row_bytes, fmt, _ptr(M), C.c_void_p(d_dst), dst_image_bytes, out_width, out_height, dst_row_bytes))

    def warp_perspective_packed_device(self, d_src, src_image_bytes, batch, width, height, src_row_bytes, fmt, table, d_dst,
                                       dst_bytes):
        """lr_warp_perspective_device with LR_WARP_PACKED: one launch for `batch` device frames of one size whose outputs
        have their own sizes and places in the dst_bytes at d_dst.  table: 13 doubles per frame (warp_table).  fmt may carry
        WARP_CUBIC, WARP_BORDER with a table of 14 doubles per frame (warp_table's border=), and WARP_LENS with nine more, or
        with WARP_LENS_MODEL seventeen more (warp_table's lens=), and WARP_AREA with one more (warp_table's area=)."""
        table = np.ascontiguousarray(table, np.float64).reshape(-1)
        cols = (14 if fmt & WARP_BORDER else 13) + ((17 if fmt & WARP_LENS_MODEL else 9) if fmt & WARP_LENS else 0) + (1 if fmt & WARP_AREA else 0)
        if table.size != cols * int(batch) or batch < 1:
            raise ValueError("warp_perspective_packed_device: the table has %d values per frame" % cols)
        out_w, out_h = (int(min(max(v, 1), 2 ** 31 - 1)) for v in np.nan_to_num(table.reshape(-1, cols)[:, 9:11]).max(axis=0))
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_image_bytes, batch, width, height, src_row_bytes, fmt | WARP_PACKED, _ptr(table), C.c_void_p(d_dst), dst_bytes, out_w, out_h, 0))

    def warp_perspective(self, array, M, out_size, interp="linear", border=None, lens=None, area=None):
        """Warps one host frame (2-D uint8 or float32, or H x W x 3 uint8) by M (3x3, destination -> source) into an image
        of out_size = (width, height) on the GPU: upload, one launch, download.  Returns the (height, width[, 3]) array.
        interp: "linear" (bilinear) or "cubic" (WARP_CUBIC: 4 x 4 bicubic, cv::warpPerspective's INTER_CUBIC).
        border: None (the zero border) or border_word's spec -- "replicate", "reflect", "reflect101", ("constant", value):
        cv::warpPerspective's borderMode and borderValue (WARP_BORDER).
        lens: None or the frame's Lens (WARP_LENS) or LensModel (WARP_LENS | WARP_LENS_MODEL): M then maps into the ideal picture, and the lens model takes the point to the
        pixel of `array` that is sampled -- undistortion and warp in one resampling.
        area: None or the sampling factor S, an integer from 1 to 8 (WARP_AREA): every pixel is the mean of S x S samples spread
        over its footprint, for a map that shrinks (shrink_homography gives map, size and S for a bound on the size)."""
        cubic = _sampling_bit(interp, "warp_perspective")
        a = np.ascontiguousarray(array)
        fmt, bpp = _frame_format(a, "warp_perspective")
        bbit, M = _border_bit_and_map(border, fmt, M, "warp_perspective", lens, area)
        h, w = a.shape[:2]
        ow, oh = int(out_size[0]), int(out_size[1])
        d_src = self.device_upload(a)
        d_dst = C.c_void_p()
        try:
            _check(lib().lr_device_malloc(self._h, ow * oh * bpp, C.byref(d_dst)))
            self.warp_perspective_device(d_src, a.nbytes, 1, w, h, w * bpp, fmt | cubic | bbit, M, d_dst.value, ow * oh * bpp, ow, oh, ow * bpp)
            return self.device_download(d_dst.value, (oh, ow) + a.shape[2:], a.dtype)
        finally:
            self.device_free(d_src)
            if d_dst.value:
                self.device_free(d_dst.value)

    def undistort(self, image, lens, interp="linear", border=None, lens_scale=1):
        """The frame without its lens distortion (cv::undistort with the frame's own camera matrix): warp_perspective with the
        identity map, the lens (a Lens or a LensModel) and the source's size.  lens_scale=s: with lens_scale_map(lens, s) in
        place of the identity, the ideal picture scaled by s about (cx, cy): s < 1 shows more of a fisheye's view."""
        a = np.asarray(image)
        if a.ndim < 2:
            raise ValueError("undistort: a 2-D uint8 or float32 frame, or an H x W x 3 uint8 frame")
        s = _check_lens_scale("undistort", lens_scale)
        M = np.eye(3) if s == 1.0 else lens_scale_map(lens, s)
        return self.warp_perspective(a, M, (a.shape[1], a.shape[0]), interp=interp, border=border, lens=lens)

    # ---- the lines picture ----
    def draw_lines_device(self, d_src, src_bytes, fmt, lines, table, d_dst, dst_bytes, H=None):
        """lr_draw_lines_device (lr_warp_perspective_device with LR_WARP_LINES): one launch, enqueued on the context's stream, that draws every frame's segments (the demo's
        draw_lines) on its u8 or u8x3 source into its u8x3 output.  lines: a LINE_DTYPE array on the host (or None);
        table: 8 doubles per frame (draw_table); H: (B, 3, 3) or None; d_src None (or 0): in place on d_dst."""
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != 8:
            raise ValueError("draw_lines_device: the table has 8 values per frame")
        if lines is not None:
            lines = np.ascontiguousarray(lines, LINE_DTYPE).reshape(-1)
        if H is not None:
            H = np.ascontiguousarray(H, np.float64).reshape(-1)
            if H.size != 9 * len(table):
                raise ValueError("draw_lines_device: H needs 9 values per frame")
        args = DrawLinesArgs(_ptr(lines), 0 if lines is None else len(lines), _ptr(table), _ptr(H))
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src) if d_src else None, src_bytes, len(table), 0, 0, 0,
                                                fmt | WARP_LINES, C.cast(C.byref(args), C.c_void_p), C.c_void_p(d_dst),
                                                dst_bytes, 0, 0, 0))

    def draw_lines_batch(self, frames, lines_list, Hs=None, jpeg=None, orient=False, jpeg_optimize=False, any_sampling=False,
                         decode_scale=None, decode_max_size=None):
        """The demo's lines picture for a list of 8-bit frames of different shapes (all gray H x W, or all H x W x 3) and
        their segments (one LINE_DTYPE array per frame; Hs: one 3x3 per frame, or None): one upload, one
        lr_draw_lines_device call, one download.  Returns the list of H x W x 3 uint8 pictures: a loop of draw_lines.
        jpeg=Q: the pictures stay in HBM, are encoded there (lr_encode_jpeg_device, quality Q, 4:2:0) and come back as JPEG files
        (bytes): exactly the encoder's stream of the picture that jpeg=None returns.
        jpeg_optimize=True (with jpeg=Q, else ValueError): the files are coded with Huffman tables of their own
        (LR_JPEG_OPTIMIZE): the same pixels in fewer bytes.
        orient=True (JPEG files only): the files' EXIF orientations are applied, the call on decode_jpeg_batch(files,
        orient=True)'s arrays.
        any_sampling=True (JPEG files only, else ValueError): files of any sampling are decoded (decode_jpeg_batch).
        decode_scale=N (JPEG files only, else ValueError; None, an int or one per file out of 1, 2, 4, 8): the files are
        decoded at 1/N of their size (LR_JPEG_SCALED): the call on decode_jpeg_batch(files, scale=N)'s arrays, every later
        stage working on 1/N^2 of the pixels.  decode_max_size=M instead (both: ValueError): per file the largest N whose
        longer side ceil(max(w, h) / N) is still at least M (jpeg_scale_for, PIL's Image.draft rule).  Segments, transforms
        and homographies that come back are in the DECODED picture's coordinates: multiply by N for the file's.  The segments
        given here are drawn as they are, so they are in the decoded picture's coordinates too."""
        _check_jpeg_optimize("draw_lines_batch", jpeg, jpeg_optimize)
        if _all_streams(frames, "draw_lines_batch", orient, any_sampling, decode_scale, decode_max_size):
            return self._draw_lines_streams([bytes(f) for f in frames], lines_list, Hs, jpeg, orient, jpeg_optimize, any_sampling, decode_scale,
                                            decode_max_size)
        frames = [np.ascontiguousarray(f) for f in frames]
        if not frames or len(lines_list) != len(frames) or (Hs is not None and len(Hs) != len(frames)):
            raise ValueError("draw_lines_batch: as many line arrays (and Hs) as frames, at least one")
        formats = [_frame_format(f, "draw_lines") for f in frames]
        fmt, bpp = formats[0]
        if fmt == PIX_F32 or any(f != formats[0] for f in formats):
            raise ValueError("draw_lines_batch: uint8 frames, all H x W or all H x W x 3")
        info, src_end = [], 0
        for f in frames:
            h, w = f.shape[:2]
            info.append((w, h, src_end, w * bpp))
            src_end = (src_end + h * w * bpp + 3) // 4 * 4  # (every frame starts at a multiple of 4)
        region = np.zeros(src_end, np.uint8)
        for f, (_, _, off, _) in zip(frames, info):
            region[off:off + f.size] = f.reshape(-1)
        return self._draw_resident(self.device_upload(region), src_end, fmt, info, lines_list, Hs, jpeg, jpeg_optimize)

    def _draw_resident(self, d_src, src_bytes, fmt, frames, lines_list, Hs, jpeg, jpeg_optimize=False):
        """draw_lines_batch for frames (width, height, byte_offset, row_bytes) that lie in the src_bytes at d_src, which is
        freed here: one lr_draw_lines_device call into a fresh buffer, then the download, or with jpeg the encoder"""
        d_dst = C.c_void_p()
        try:
            lines_list = [np.ascontiguousarray(l, LINE_DTYPE).reshape(-1) for l in lines_list]
            sizes, outputs, segments = [], [], []
            dst_end = first = 0
            for (w, h, _, _), l in zip(frames, lines_list):
                sizes.append((w, h))
                outputs.append((dst_end, w * 3))
                segments.append((first, len(l)))
                dst_end = (dst_end + h * w * 3 + 3) // 4 * 4
                first += len(l)
            table = draw_table(sizes, [f[2:] for f in frames], outputs, segments)
            _check(lib().lr_device_malloc(self._h, dst_end, C.byref(d_dst)))
            self.draw_lines_device(d_src, src_bytes, fmt, np.concatenate(lines_list), table, d_dst.value, dst_end, H=Hs)
            if jpeg is not None:
                return self._encode_resident(d_dst.value, dst_end, PIX_U8X3, [(w, h, off, row) for (w, h), (off, row) in zip(sizes, outputs)], jpeg, 0, jpeg_optimize)
            out = self.device_download(d_dst.value, (dst_end,), np.uint8)
        finally:
            self.device_free(d_src)
            if d_dst.value:
                self.device_free(d_dst.value)
        return [out[off:off + w * h * 3].reshape(h, w, 3).copy() for (w, h), (off, _) in zip(sizes, outputs)]

    def _draw_lines_streams(self, streams, lines_list, Hs, jpeg, orient=False, jpeg_optimize=False, any_sampling=False, decode_scale=None,
                            decode_max_size=None):
        """draw_lines_batch for JPEG files (bytes): decoded in HBM, drawn on where they lie"""
        if len(lines_list) != len(streams) or (Hs is not None and len(Hs) != len(streams)):
            raise ValueError("draw_lines_batch: as many line arrays (and Hs) as frames, at least one")
        d_src, src_bytes, fmt, frames = self._decode_resident(streams, None, "draw_lines_batch", orient, any_sampling, decode_scale, decode_max_size)
        return self._draw_resident(d_src, src_bytes, fmt, frames, lines_list, Hs, jpeg, jpeg_optimize)

    def draw_lines(self, image_u8, lines, H=None):
        """The demo's lines picture of one 8-bit frame (H x W gray or H x W x 3) and the detector's segments, drawn through
        H (3x3) if given: upload, one launch, download.  Returns H x W x 3 uint8."""
        return self.draw_lines_batch([image_u8], [lines], None if H is None else [H])[0]

    # ---- JPEG streams ----
    jpeg_first_capacity = None  # test hook: bytes of every frame's extent in the first pass of _encode_resident

    def encode_jpeg_device(self, d_src, src_bytes, fmt, table, d_dst, dst_bytes):
        """lr_encode_jpeg_device (lr_warp_perspective_device with LR_WARP_JPEG): baseline JPEG streams of the table's 8-bit
        frames (fmt PIX_U8 or PIX_U8X3) in the src_bytes at d_src, each into its extent of the dst_bytes at d_dst.
        table: 8 doubles per frame (jpeg_table).  Synchronous.  Returns the streams' lengths (uint64, one per frame), a
        length above its frame's capacity meaning that the stream did not fit and the extent's content is unspecified."""
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != 8 or len(table) < 1:
            raise ValueError("encode_jpeg_device: the table has 8 values per frame")
        sizes = np.zeros(len(table), np.uint64)
        args = JpegArgs(_ptr(table), _ptr(sizes))
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_bytes, len(table), 0, 0, 0, fmt | WARP_JPEG,
                                                C.cast(C.byref(args), C.c_void_p), C.c_void_p(d_dst), dst_bytes, 0, 0, 0))
        return sizes

    def _encode_resident(self, d_src, src_bytes, fmt, frames, quality, layout, optimize=False):
        """JPEG streams (bytes) of resident frames (width, height, byte_offset, row_bytes): one call with a modest extent per
        frame (half the frame's bytes, or its bound if that is less), a second one with jpeg_bound for the frames whose
        streams did not fit, and a download of the streams alone.  optimize: LR_JPEG_OPTIMIZE for every frame."""
        bpp = 3 if fmt == PIX_U8X3 else 1
        out = [None] * len(frames)
        todo = list(range(len(frames)))
        for attempt in (0, 1):
            caps = []
            for b in todo:
                w, h = frames[b][:2]
                bound = jpeg_bound(w, h, fmt, layout, optimize)
                first = w * h * bpp // 2 + 1024 if self.jpeg_first_capacity is None else int(self.jpeg_first_capacity)
                caps.append(bound if attempt else min(bound, first))
            offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
            table = jpeg_table(np.array([frames[b][:2] for b in todo], np.int64), np.array([frames[b][2:] for b in todo], np.int64),
                               np.stack([offs[:-1], np.array(caps, np.int64)], axis=1), int(quality), int(layout), bool(optimize))
            d_dst = C.c_void_p()
            _check(lib().lr_device_malloc(self._h, int(offs[-1]), C.byref(d_dst)))
            try:
                sizes = self.encode_jpeg_device(d_src, src_bytes, fmt, table, d_dst.value, int(offs[-1]))
                left = []
                for b, off, cap, n in zip(todo, offs[:-1].tolist(), caps, sizes.tolist()):
                    if n <= cap:
                        out[b] = self.device_download(d_dst.value + off, (n,), np.uint8).tobytes()
                    else:
                        left.append(b)
            finally:
                self.device_free(d_dst.value)
            todo = left
            if not todo:
                break
        if todo:
            raise LibrectifyError("encode_jpeg: a stream longer than jpeg_bound")
        return out

    def encode_jpeg_batch(self, frames, quality=95, layout=0, optimize=False):
        """Baseline JPEG files of a list of 8-bit frames of any sizes (all H x W, or all H x W x 3 with c0 red): one upload,
        one lr_encode_jpeg_device call (a second for frames whose streams outgrow half their pixels' bytes), and a download
        of the streams only.  layout: 0 = 4:2:0, 1 = 4:4:4 (colour frames).  optimize=True: every file is coded with Huffman
        tables made from its own symbols (LR_JPEG_OPTIMIZE; PIL's optimize=True): the same pixels in fewer bytes.  Returns a
        list of bytes."""
        frames = [np.ascontiguousarray(f) for f in frames]
        if not frames:
            raise ValueError("encode_jpeg_batch: no frames")
        formats = [_frame_format(f, "encode_jpeg") for f in frames]
        fmt, bpp = formats[0]
        if fmt == PIX_F32 or any(f != formats[0] for f in formats):
            raise ValueError("encode_jpeg_batch: uint8 frames, all H x W or all H x W x 3")
        info, end = [], 0
        for f in frames:
            h, w = f.shape[:2]
            info.append((w, h, end, w * bpp))
            end += f.nbytes
        region = np.concatenate([f.reshape(-1) for f in frames])
        d_src = self.device_upload(region)
        try:
            return self._encode_resident(d_src, end, fmt, info, quality, layout, optimize)
        finally:
            self.device_free(d_src)

    def encode_jpeg(self, image_u8, quality=95, layout=0, optimize=False):
        """The baseline JPEG file (bytes) of one 8-bit frame, H x W or H x W x 3 (c0 red), encoded on the GPU; optimize=True:
        with Huffman tables of its own (LR_JPEG_OPTIMIZE)."""
        return self.encode_jpeg_batch([image_u8], quality, layout, optimize)[0]

    # ---- network input tensors ----
    def pack_tensor_device(self, d_src, src_bytes, fmt, table, spec, n, d_dst, dst_bytes):
        """lr_pack_tensor_device (lr_warp_perspective_device with LR_WARP_TENSOR): the table's 8-bit pictures (fmt PIX_U8 or
        PIX_U8X3) in the src_bytes at d_src, each letterboxed into its slot of the n-slot tensor of `spec` in the dst_bytes at
        d_dst.  table: 8 doubles per frame (tensor_table).  Synchronous: on return the tensor may be read from any stream."""
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != 8 or len(table) < 1:
            raise ValueError("pack_tensor_device: the table has 8 values per frame")
        args = spec.args(table, int(n))
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_bytes, len(table), 0, 0, 0, fmt | WARP_TENSOR,
                                                C.cast(C.byref(args), C.c_void_p), C.c_void_p(d_dst), dst_bytes, 0, 0, 0))

    @staticmethod
    def _pad_slot(spec, fmt):
        """A slot of nothing but pad, by the rule restated in NumPy (the slot of a frame that has no picture)"""
        C_ = spec.channels(fmt)
        y = (spec.pad[:C_] * spec.scale[:C_] + spec.bias[:C_]).astype(np.float32)
        if spec.dtype == "f16":
            y = y.astype(np.float16)
        elif spec.dtype == "bf16":
            bits = y.view(np.uint32)
            y = ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
        shape = spec.shape(1, fmt)[1:]
        return np.ascontiguousarray(np.broadcast_to(y.reshape((C_, 1, 1) if spec.layout == "nchw" else (1, 1, C_)), shape))

    def _pack_resident(self, d_src, src_bytes, fmt, frames, spec, out=None):
        """The tensor of resident pictures: frames[b] is (width, height, byte_offset, row_bytes) or None (a slot of pad), frame b
        goes into slot b.  One lr_pack_tensor_device call; with out=None the tensor is downloaded (NumPy), otherwise `out` (an
        object with data_ptr(), shape, dtype and is_contiguous(): a torch tensor on the context's device) is written in place
        and returned."""
        n = len(frames)
        shape = spec.shape(n, fmt)
        elem = np.dtype(spec.np_dtype).itemsize
        total = int(np.prod(shape, dtype=np.int64)) * elem
        if out is not None:
            want = {"f32": "float32", "f16": "float16", "bf16": "bfloat16"}[spec.dtype]
            if (not all(hasattr(out, a) for a in ("data_ptr", "shape", "dtype", "is_contiguous")) or tuple(out.shape) != shape
                    or str(out.dtype).split(".")[-1] != want or not out.is_contiguous() or not getattr(out, "is_cuda", True)):
                raise ValueError("pack_tensor: out is a contiguous device tensor of shape %r and dtype %s" % (shape, want))
        named = [b for b in range(n) if frames[b] is not None]
        d_dst = C.c_void_p(out.data_ptr()) if out is not None else C.c_void_p()
        if out is None:
            _check(lib().lr_device_malloc(self._h, total, C.byref(d_dst)))
        try:
            if named:
                table = tensor_table(np.array([frames[b][:2] for b in named], np.int64), np.array([frames[b][2:] for b in named], np.int64),
                                     np.array(named, np.int64), spec)
                self.pack_tensor_device(d_src, src_bytes, fmt, table, spec, n, d_dst.value, total)
            if len(named) < n:
                slot = self._pad_slot(spec, fmt)
                for b in range(n):
                    if frames[b] is None:
                        _check(lib().lr_memcpy_h2d(self._h, C.c_void_p(d_dst.value + b * slot.nbytes), _ptr(slot), slot.nbytes))
            if out is not None:
                return out
            return self.device_download(d_dst.value, shape, spec.np_dtype)
        finally:
            if out is None:
                self.device_free(d_dst.value)

    def pack_tensor(self, pictures, spec, out=None, fmt=None):
        """The network input tensor of a list of 8-bit pictures (all H x W, or all H x W x 3), each no larger than the slot of
        `spec` (a TensorSpec): one upload, one lr_pack_tensor_device call, one download.  Picture b goes into slot b, placed as
        spec.place says; an entry None gives a slot of nothing but pad (fmt= names the format when every entry is None).
        Returns a NumPy array of the tensor's shape: float32, float16, or uint16 bit patterns for "bf16".  out=: a contiguous
        torch tensor of that shape and dtype on the context's device (any object with data_ptr(), shape, dtype and
        is_contiguous()) is written in place and returned, and nothing is downloaded; work that torch has enqueued on `out`
        must be complete, since the pack runs on the context's stream."""
        pics = [None if p is None else np.ascontiguousarray(p) for p in pictures]
        if not pics:
            raise ValueError("pack_tensor: no pictures")
        formats = [_frame_format(p, "pack_tensor") for p in pics if p is not None]
        if formats:
            if formats[0][0] == PIX_F32 or any(f != formats[0] for f in formats) or (fmt is not None and fmt != formats[0][0]):
                raise ValueError("pack_tensor: uint8 pictures, all H x W or all H x W x 3")
            fmt = formats[0][0]
        elif fmt is None:
            raise ValueError("pack_tensor: no picture and no fmt=")
        bpp = 3 if fmt == PIX_U8X3 else 1
        spec.channels(fmt)
        info, end = [], 0
        for p in pics:
            if p is None:
                info.append(None)
                continue
            h, w = p.shape[:2]
            if h > spec.height or w > spec.width:
                raise ValueError("pack_tensor: a picture larger than the slot")
            info.append((w, h, end, w * bpp))
            end += p.nbytes
        region = np.concatenate([p.reshape(-1) for p in pics if p is not None]) if formats else np.zeros(1, np.uint8)
        d_src = self.device_upload(region)
        try:
            return self._pack_resident(d_src, max(end, 1), fmt, info, spec, out)
        finally:
            self.device_free(d_src)

    def decode_jpeg_device(self, d_src, h_src, fmt, table, d_dst, dst_bytes):
        """lr_decode_jpeg_device (lr_warp_perspective_device with LR_WARP_JPEG_DECODE): the table's baseline JPEG streams in
        the region at d_src (h_src: the same bytes on the host, a uint8 array; only the headers are read from it) become
        8-bit pictures (fmt PIX_U8: luminance, PIX_U8X3: RGB) in the dst_bytes at d_dst.  table: 8 doubles per frame
        (jpeg_decode_table).  Synchronous.  Returns info, int32 (B, 8): width, height, components, layout, restart
        interval, status, decodes of the most often decoded part, and 0 -- or, for a frame whose entry [7] is 1
        (jpeg_decode_table's orient), the EXIF orientation applied, 1 .. 8, width and height being the upright picture's.
        JPEG_ANY_SAMPLING or-ed into fmt admits every sampling with factors 1, 2 or 4 (jpeg_info); the layout column of
        such a frame is its luminance's sampling byte.  JPEG_SCALED or-ed into fmt makes entry [6] of a frame's row its
        scale denominator (jpeg_decode_table's scale): the picture is written at 1/2, 1/4 or 1/8 of its size, and width and
        height are the reduced picture's.  d_dst None: probe mode."""
        return _decode_call(self._h, d_src, h_src, fmt, table, d_dst, dst_bytes)

    def _decode_resident(self, streams, fmt, what, orient=False, any_sampling=False, scale=None, max_size=None):
        """The JPEG files decoded into one fresh device buffer: one upload of the files, one lr_decode_jpeg_device call.
        fmt None: PIX_U8 if every file has one component, else PIX_U8X3.  Returns (d_dst, total_bytes, fmt, frames) with
        frames[b] = (width, height, byte_offset, row_bytes), every picture at a multiple of 4; the caller frees d_dst.
        orient: the files' EXIF orientations are applied, and the sizes are the upright pictures'.
        any_sampling: both calls carry JPEG_ANY_SAMPLING.
        scale (None, an int or B ints out of 1, 2, 4, 8): both calls carry JPEG_SCALED, and the sizes are the reduced
        pictures'.  max_size (instead of scale): the scales are jpeg_scale_for's choice from one more probe.
        Raises LibrectifyError naming the first frame whose status is not 0."""
        region, extents = _stream_region(streams)
        if max_size is not None:  # (a file that the probe refuses keeps scale 1 and is named below)
            scale = jpeg_scale_for(_decode_call(None, None, region, PIX_U8X3 | _any_sampling_bit(any_sampling), jpeg_decode_table(extents), None, 0)[:, :2].tolist(),
                                   max_size)
        orient, bit = bool(orient), _any_sampling_bit(any_sampling) | _scaled_bit(scale)
        info = _decode_call(None, None, region, PIX_U8X3 | bit, jpeg_decode_table(extents, orient=orient, scale=scale), None, 0)
        bad = np.flatnonzero(info[:, 5])
        if len(bad):
            jpeg_info([streams[bad[0]]], any_sampling=any_sampling)  # (once more alone: lr_last_error then tells why)
            raise LibrectifyError("%s: frame %d: status %d: %s" % (what, bad[0], info[bad[0], 5], lib().lr_last_error().decode().split(": ", 2)[-1]))
        if fmt is None:
            fmt = PIX_U8 if int(info[:, 2].max()) == 1 else PIX_U8X3
        bpp = 3 if fmt == PIX_U8X3 else 1
        frames, end = [], 0
        for w, h in info[:, :2].tolist():
            start = (end + 3) // 4 * 4
            frames.append((w, h, start, w * bpp))
            end = start + w * h * bpp
        table = jpeg_decode_table(extents, np.array([f[2:] for f in frames], np.int64), np.array([f[:2] for f in frames], np.int64), orient, scale)
        d_src = self.device_upload(region)
        d_dst = C.c_void_p()
        try:
            _check(lib().lr_device_malloc(self._h, end, C.byref(d_dst)))
            info = self.decode_jpeg_device(d_src, region, fmt | bit, table, d_dst.value, end)
            bad = np.flatnonzero(info[:, 5])
            if len(bad):
                raise LibrectifyError("%s: frame %d: status %d: %s" % (what, bad[0], info[bad[0], 5], lib().lr_last_error().decode()))
            res, d_dst = d_dst.value, C.c_void_p()
            return res, end, fmt, frames
        finally:
            self.device_free(d_src)
            if d_dst.value:
                self.device_free(d_dst.value)

    def decode_jpeg_batch(self, streams, fmt=PIX_U8X3, orient=False, any_sampling=False, scale=None):
        """A list of baseline JPEG files (bytes) of any sizes and samplings decoded on the GPU: one upload of the files, one
        lr_decode_jpeg_device call, one download.  fmt PIX_U8X3: H x W x 3 RGB pictures (a one-component file replicated);
        PIX_U8: H x W luminance.  orient=True: every file's EXIF orientation (tag 0x0112 of its first Exif segment) is
        applied in the decoder's output pass and the pictures come out upright, what PIL's ImageOps.exif_transpose makes of
        them; a file that tells none comes out as stored.  any_sampling=True (LR_JPEG_ANY_SAMPLING): files of 4:4:0, 4:1:1 and
        every other sampling with factors 1, 2 or 4 (jpeg_info) are decoded too, not refused with status 2.
        scale (None, an int or B ints out of 1, 2, 4, 8; LR_JPEG_SCALED): file b comes out at 1/N of its size, ceil(w / N) x
        ceil(h / N), averaged from the blocks' samples inside the decoder (within a few levels of the N x N box average of the
        full decode); coordinates in it are the file's divided by N.  Returns a list of uint8 arrays.  Raises LibrectifyError naming the frame on a status
        other than 0 (jpeg_info tells the statuses beforehand)."""
        if fmt not in (PIX_U8, PIX_U8X3):
            raise ValueError("decode_jpeg_batch: fmt is PIX_U8 or PIX_U8X3")
        d_dst, total, fmt, frames = self._decode_resident(streams, fmt, "decode_jpeg_batch", orient, any_sampling, scale)
        try:
            out = self.device_download(d_dst, (total,), np.uint8)
        finally:
            self.device_free(d_dst)
        tail = (3,) if fmt == PIX_U8X3 else ()
        return [out[off:off + h * row].reshape((h, w) + tail).copy() for w, h, off, row in frames]

    def decode_jpeg(self, data, fmt=PIX_U8X3, orient=False, any_sampling=False, scale=None):
        """One baseline JPEG file (bytes) decoded on the GPU: H x W x 3 RGB (PIX_U8X3) or H x W luminance (PIX_U8);
        orient=True: upright, by the file's EXIF orientation; any_sampling=True: of any sampling; scale=2, 4 or 8: at 1/N of
        its size (decode_jpeg_batch)."""
        return self.decode_jpeg_batch([data], fmt, orient, any_sampling, scale)[0]

    def _rectify_streams(self, streams, min_length, refine, cfg, clip, max_size, capacity, jpeg, orient=False, interp="linear", jpeg_optimize=False,
                         any_sampling=False, border=None, crop=False, decode_scale=None, decode_max_size=None, lens=None, out_max_size=None, tensor=None):
        """rectify_batch for JPEG files: the files go up and are decoded in HBM, the pictures are handed to
        rectify_frames_device where they lie; with jpeg=Q no pixel crosses the link in either direction"""
        d_src, _, fmt, sources = self._decode_resident(streams, None, "rectify_batch", orient, any_sampling, decode_scale, decode_max_size)
        return self._rectify_resident(d_src, sources, fmt, min_length, refine, cfg, clip, max_size, capacity, jpeg, interp, jpeg_optimize, border, crop, lens, out_max_size, tensor)

    def prepare_device(self, d_src, src_image_bytes, batch, width, height, src_row_bytes, fmt, d_dst, dst_image_bytes,
                       out_width, out_height, dst_row_bytes):
        """lr_warp_perspective_device with LR_WARP_PREPARE: `batch` device frames of format fmt (PIX_U8, PIX_U8X3,
        PIX_F32) become f32 gray frames of out_width x out_height, luma / 256 area-averaged; one launch on the context's
        stream."""
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_image_bytes, batch, width, height, src_row_bytes, fmt | WARP_PREPARE, None, C.c_void_p(d_dst), dst_image_bytes, out_width, out_height, dst_row_bytes))

    def prepare(self, frames_u8, max_size):
        """The demo's first step on the GPU: uploads 8-bit frames (H x W, H x W x 3, or either with a leading batch
        axis), prepares them to prepared_size(W, H, max_size) and downloads the float32 result ((B,) H' x W')."""
        a = np.ascontiguousarray(frames_u8)
        if a.dtype != np.uint8 or a.ndim not in (2, 3, 4) or (a.ndim == 4 and a.shape[3] != 3):
            raise ValueError("prepare: uint8 frames, H x W or H x W x 3, or a batch of either")
        batched = a.ndim == 4 or (a.ndim == 3 and a.shape[2] != 3)
        frames = a if batched else a[None]
        fmt, bpp = _frame_format(frames[0], "prepare")
        batch, h, w = frames.shape[:3]
        ow, oh, _ = prepared_size(w, h, max_size)
        d_src = self.device_upload(frames)
        d_dst = C.c_void_p()
        try:
            _check(lib().lr_device_malloc(self._h, batch * ow * oh * 4, C.byref(d_dst)))
            self.prepare_device(d_src, h * w * bpp, batch, w, h, w * bpp, fmt, d_dst.value, ow * oh * 4, ow, oh, ow * 4)
            out = self.device_download(d_dst.value, (batch, oh, ow), np.float32)
        finally:
            self.device_free(d_src)
            if d_dst.value:
                self.device_free(d_dst.value)
        return out if batched else out[0]

    def _rectify_prepared(self, img, max_size, min_length, refine, cfg, clip, cubic=0, border=None, crop=False, out_max_size=None):
        """rectify with the demo's prescale: the 8-bit frame goes up once; the prepare step, the detector and the warp all
        read it in HBM"""
        fmt, bpp = _frame_format(img, "rectify")
        h, w = img.shape[:2]
        ow, oh, scale = prepared_size(w, h, max_size)
        d_src = self.device_upload(img)
        d_small, d_dst = C.c_void_p(), C.c_void_p()
        try:
            _check(lib().lr_device_malloc(self._h, ow * oh * 4, C.byref(d_small)))
            self.prepare_device(d_src, img.nbytes, 1, w, h, w * bpp, fmt, d_small.value, ow * oh * 4, ow, oh, ow * 4)
            if min_length is None:
                min_length = max(ow, oh) / 100.0
            lines = self.find_line_segment_groups_device(d_small.value, ow, oh, min_length, refine=refine).copy()
            for k in ("x1", "y1", "x2", "y2"):  # back to the coordinates of the full frame, in float32 as the demo
                lines[k] = lines[k] / scale
            t = compute_rectification_transform(lines, w, h, cfg)
            M, (rw, rh), rect = _rectified_map(t, clip, crop, cubic)
            M, (rw, rh), S = _bounded_map(M, (rw, rh), out_max_size)
            bbit, M = _border_bit_and_map(border, fmt, M, "rectify", None, S)
            _check(lib().lr_device_malloc(self._h, rw * rh * bpp, C.byref(d_dst)))
            self.warp_perspective_device(d_src, img.nbytes, 1, w, h, w * bpp, fmt | cubic | bbit, M, d_dst.value, rw * rh * bpp, rw, rh, rw * bpp)
            return (lines, t, self.device_download(d_dst.value, (rh, rw) + img.shape[2:], np.uint8)) + ((rect,) if crop else ())
        finally:
            self.device_free(d_src)
            for p in (d_small, d_dst):
                if p.value:
                    self.device_free(p.value)

    def rectify(self, image_u8, min_length=None, refine=False, cfg=None, clip=3.0, max_size=None, jpeg=None, orient=False,
                interp="linear", jpeg_optimize=False, any_sampling=False, border=None, crop=False, decode_scale=None, decode_max_size=None,
                lens=None, out_max_size=None, lens_scale=1, tensor=None, tensor_out=None):
        """The reference demo's pipeline (autorectify.cpp) on an 8-bit frame (H x W gray or H x W x 3 RGB): luma
        (4899 R + 9617 G + 1868 B + 8192) >> 14, / 256, find_line_segment_groups with min_length max(w, h) / 100 by
        default, compute_rectification_transform (cfg: the demo's, horizontal_vp_min_distance = 2),
        rectification_homography(clip) and the warp of the original frame.  Returns (lines, transform, warped).
        max_size=None: without the demo's prescale -- the 8-bit frame is uploaded once, the detector reads it where it lies
        (frames_word: luma and / 256 happen on the device, exactly) and the warp reads the same resident frame.  max_size=N (the
        demo's default is 1200; below 1 a fraction of the longer side): with it -- the 8-bit frame is uploaded once,
        prepared on the device (prepare_device) to prepared_size(w, h, max_size), the detector runs on that with
        min_length max(w', h') / 100, the endpoints are divided by the scale, the transform is the full frame's and the
        warp reads the same resident frame.
        jpeg=Q: `warped` is the rectified picture's JPEG file (bytes, quality Q, 4:2:0), encoded in HBM: rectify_batch's
        path for one frame.  jpeg_optimize=True (with jpeg=Q, else ValueError): the file is coded with Huffman tables of its
        own (LR_JPEG_OPTIMIZE), the same pixels in fewer bytes.
        orient=True (a JPEG file only): the file's EXIF orientation is applied as it is decoded, as the demo's imread
        does: the call on decode_jpeg(file, orient=True).
        any_sampling=True (a JPEG file only): a file of any sampling is decoded (LR_JPEG_ANY_SAMPLING): the call on
        decode_jpeg(file, any_sampling=True).
        decode_scale=N (a JPEG file only, else ValueError; None, an int or one per file out of 1, 2, 4, 8): the files are
        decoded at 1/N of their size (LR_JPEG_SCALED): the call on decode_jpeg_batch(files, scale=N)'s arrays, every later
        stage working on 1/N^2 of the pixels.  decode_max_size=M instead (both: ValueError): per file the largest N whose
        longer side ceil(max(w, h) / N) is still at least M (jpeg_scale_for, PIL's Image.draft rule).  Segments, transforms
        and homographies that come back are in the DECODED picture's coordinates: multiply by N for the file's.
        interp="cubic": the warp samples 4 x 4 bicubic (WARP_CUBIC) instead of bilinear, on every path above; lines,
        transform, homography and size are those of interp="linear", only the picture (or its JPEG file) differs.
        border: None (the zero border: the demo's black wedges) or border_word's spec -- "replicate", "reflect", "reflect101",
        ("constant", value) -- for what lies outside the source (WARP_BORDER); only the picture differs.
        crop=True: the picture (or its JPEG file) is the constrained crop, the largest upright rectangle of the source's aspect
        around the image of the source's centre that contains no border (crop_homography; the margin follows interp), and the
        call returns (lines, transform, warped, (x0, y0, width, height)), the rectangle in the uncropped picture.
        lens: the frame's Lens (WARP_LENS), for a photograph that is no pinhole picture; it refers to the frame as uploaded or
        decoded.  The frame goes up (or is decoded) once; one WARP_LENS launch with the identity map, bilinear, zero border,
        writes it without its distortion in HBM; luma, the prepare step and the detector run on that, so lines, transform
        and homography are in IDEAL coordinates (lens_distort takes them back onto the photograph); the final warp reads
        the ORIGINAL frame with WARP_LENS, the homography and the call's interp and border: one resampling.  The lines and the
        transform are those of rectify(undistort(image, lens)), the picture is warp_perspective(image, M, lens=lens).
        With crop=True: ValueError (the crop's rectangle assumes straight source edges).  A LensModel in place of the Lens
        (WARP_LENS | WARP_LENS_MODEL on both launches): OpenCV's rational and thin-prism model, or LensModel.fisheye's.
        lens_scale=s (with lens=, else ValueError; a finite number above 0): the detector sees the ideal picture scaled by s
        about the lens's (cx, cy) -- s < 1 brings more of a fisheye's view into the frame's size -- and the final map is
        lens_scale_map(lens, s) @ M.  Lines, transform and homography are then in the SCALED ideal picture's coordinates:
        lens_scale_map(lens, s) takes a point of it to the ideal picture, lens_distort from there onto the photograph.
        out_max_size=N: the picture (or its JPEG file) is at most N pixels on its longer side.  The final warp carries
        WARP_AREA with shrink_homography's map, size and sampling factor S (applied after the crop where crop=True, whose
        rectangle stays in the uncropped full-size picture): every pixel is the mean of S x S samples over its footprint, taken
        from the stored frame in the one resampling there is, with the call's lens, interp and border; no full-size picture
        exists in HBM.  Lines and transform do not change.  None: the call as it was.
        tensor=spec (a TensorSpec; with out_max_size=: ValueError): rectify_batch's tensor= for one frame.  The call returns
        (result, tensor): result is the call's with out_max_size=fit_box(size, (W, H)) and the tensor map at its end, tensor
        the one-slot tensor (pack_tensor's return; tensor_out= is its out=)."""
        _check_tensor("rectify", tensor, tensor_out, out_max_size)
        if tensor is not None:
            batch = [bytes(image_u8)] if isinstance(image_u8, (bytes, bytearray, memoryview)) else np.asarray(image_u8)[None]
            res, packed = self.rectify_batch(batch, min_length=min_length, refine=refine, cfg=cfg, clip=clip, max_size=max_size, jpeg=jpeg, orient=orient, interp=interp, jpeg_optimize=jpeg_optimize, any_sampling=any_sampling, border=border, crop=crop,
                                             decode_scale=decode_scale, decode_max_size=decode_max_size, lens=lens, lens_scale=lens_scale, tensor=tensor, tensor_out=tensor_out)
            if res[0][2] is None:
                _rectified_map(res[0][1], clip, crop, _sampling_bit(interp, "rectify"))  # (raises what rectify raises for such a frame)
            return res[0], packed
        cubic = _sampling_bit(interp, "rectify")
        _check_jpeg_optimize("rectify", jpeg, jpeg_optimize)
        _check_out_max_size("rectify", out_max_size)
        if lens is not None:
            if crop:
                raise ValueError("rectify: crop=True together with lens= (the crop's rectangle assumes straight source edges)")
            row = _lens_row(lens, "rectify")
            lens = LensModel(*row) if len(row) == 17 else Lens(*row)
        if _check_lens_scale("rectify", lens_scale) != 1.0 and lens is None:
            raise ValueError("rectify: lens_scale goes with lens=")
        if isinstance(image_u8, (bytes, bytearray, memoryview)):  # a JPEG file: decoded in HBM, rectify_batch's path for one frame
            res = self.rectify_batch([bytes(image_u8)], min_length=min_length, refine=refine, cfg=cfg, clip=clip, max_size=max_size, jpeg=jpeg, orient=orient, interp=interp, jpeg_optimize=jpeg_optimize, any_sampling=any_sampling, border=border, crop=crop,
                                     decode_scale=decode_scale, decode_max_size=decode_max_size, lens=lens, out_max_size=out_max_size, lens_scale=lens_scale)[0]
            if res[2] is None:
                _rectified_map(res[1], clip, crop, cubic)  # (raises what rectify raises for such a frame)
            return res
        if orient:
            raise ValueError("rectify: orient=True goes with a JPEG file (bytes); an array carries no EXIF orientation")
        if any_sampling:
            raise ValueError("rectify: any_sampling=True goes with a JPEG file (bytes); an array has no chroma sampling")
        if decode_scale is not None or decode_max_size is not None:
            raise ValueError("rectify: decode_scale and decode_max_size go with a JPEG file (bytes); an array is not decoded")
        img = np.ascontiguousarray(image_u8)
        if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
            raise ValueError("rectify: an H x W or H x W x 3 uint8 frame")
        if jpeg is not None or lens is not None:  # (with a lens: the mixed-size pipeline for one frame, which has the undistorting launch)
            res = self.rectify_batch(img[None], min_length=min_length, refine=refine, cfg=cfg, clip=clip, max_size=max_size, jpeg=jpeg, interp=interp, jpeg_optimize=jpeg_optimize, border=border, crop=crop, lens=lens, out_max_size=out_max_size, lens_scale=lens_scale)[0]
            if res[2] is None:
                _rectified_map(res[1], clip, crop, cubic)  # (raises what rectify raises for such a frame)
            return res
        fmt, bpp = _frame_format(img, "rectify")
        _border_words(border, 1, fmt, "rectify")  # (a bad spec: ValueError before anything is launched)
        if max_size is not None:
            return self._rectify_prepared(img, max_size, min_length, refine, cfg or RectificationConfig(hmin=2.0), clip, cubic, border, crop, out_max_size)
        h, w = img.shape[:2]
        if min_length is None:
            min_length = max(w, h) / 100.0
        if cfg is None:
            cfg = RectificationConfig(hmin=2.0)
        d_src = self.device_upload(img)
        d_dst = C.c_void_p()
        try:
            lines = self.find_line_segment_groups_device(d_src, w, h, min_length, refine=refine, fmt=fmt).copy()
            t = compute_rectification_transform(lines, w, h, cfg)
            M, (rw, rh), rect = _rectified_map(t, clip, crop, cubic)
            M, (rw, rh), S = _bounded_map(M, (rw, rh), out_max_size)
            bbit, M = _border_bit_and_map(border, fmt, M, "rectify", None, S)
            _check(lib().lr_device_malloc(self._h, rw * rh * bpp, C.byref(d_dst)))
            self.warp_perspective_device(d_src, img.nbytes, 1, w, h, w * bpp, fmt | cubic | bbit, M, d_dst.value, rw * rh * bpp, rw, rh, rw * bpp)
            return (lines, t, self.device_download(d_dst.value, (rh, rw) + img.shape[2:], np.uint8)) + ((rect,) if crop else ())
        finally:
            self.device_free(d_src)
            if d_dst.value:
                self.device_free(d_dst.value)

    def rectify_batch_device(self, d_frames, batch, width, height, fmt, src_row_bytes=None, src_image_bytes=None,
                             min_length=None, refine=False, cfg=None, clip=3.0, max_size=None, capacity=4096, interp="linear",
                             border=None, crop=False, out_max_size=None):
        """rectify for `batch` 8-bit frames (fmt PIX_U8 or PIX_U8X3) of one width x height that are resident in HBM, frame
        b at d_frames + b * src_image_bytes: with max_size one batched prepare_device, then the batch detector
        (lr_find_line_segment_groups_batch_device on the 8-bit frames, or on the prepared ones; its own transforms are not
        asked for), on the host what rectify does per frame (endpoints / scale, compute_rectification_transform for the
        full size, rectification_homography), and the packed warp into one allocation: one launch when every frame has an
        image, else one per run of consecutive frames that have one (a launch's source frames are consecutive), all into
        the same region.  Returns (lines_list, transforms, table, d_out, total_bytes): row b of table (warp_table's layout,
        rows and frames aligned to 4 bytes) says where frame b's image lies in the total_bytes at d_out, which stay on the
        device and are the caller's to free (None when no frame has an image).  A frame whose homography cannot be formed
        has an all-zero row and no bytes in d_out; its lines and transform are returned all the same.
        capacity: lines per frame of the first detector pass.  A frame that has more makes the WHOLE batch's detector pass
        run once more with room for the longest list, so no frame's lines are ever cut, at twice the detector's cost for
        such a batch; a caller who expects more than 4096 lines in a frame passes a larger capacity.
        interp: "linear" or "cubic", the packed warp's sampling rule (WARP_CUBIC); nothing else changes.
        border: None, one border_word spec for all frames or a list of one per frame (WARP_BORDER: the table then has 14
        columns).  crop=True: every picture is its constrained crop (rectify's crop=; a frame whose crop cannot be formed
        has no image) and a sixth value is returned: the list of the frames' rectangles (x0, y0, width, height), None for a
        frame without an image.  out_max_size=N: every picture is at most N pixels on its longer side (rectify's out_max_size=:
        WARP_AREA on the packed warp; the table then has one more column at its end, the frames' sampling factors)."""
        cubic = _sampling_bit(interp, "rectify_batch_device")
        _check_out_max_size("rectify_batch_device", out_max_size)
        if fmt not in (PIX_U8, PIX_U8X3):
            raise ValueError("rectify_batch_device: 8-bit frames, PIX_U8 or PIX_U8X3")
        batch, w, h = int(batch), int(width), int(height)
        if batch < 1:
            raise ValueError("rectify_batch_device: batch < 1")
        words = None if border is None else _border_words(border, batch, fmt, "rectify_batch_device")
        bpp = 3 if fmt == PIX_U8X3 else 1
        srow = w * bpp if src_row_bytes is None else int(src_row_bytes)
        simg = h * srow if src_image_bytes is None else int(src_image_bytes)
        if cfg is None:
            cfg = RectificationConfig(hmin=2.0)
        d_small, d_out = C.c_void_p(), C.c_void_p()
        try:
            if max_size is not None:
                pw, ph, scale = prepared_size(w, h, max_size)
                _check(lib().lr_device_malloc(self._h, batch * pw * ph * 4, C.byref(d_small)))
                self.prepare_device(d_frames, simg, batch, w, h, srow, fmt, d_small.value, pw * ph * 4, pw, ph, pw * 4)
                self.synchronize()  # (the batch detector reads the frames on its lanes' streams, not after this one's work)
                det = dict(dptr=d_small.value, image_stride=pw * ph, w=pw, h=ph, fmt=PIX_F32, stride=pw)
            else:
                if srow % bpp or simg % bpp:
                    raise ValueError("rectify_batch_device: the detector takes strides in whole pixels")
                pw, ph, scale = w, h, None
                det = dict(dptr=d_frames, image_stride=simg // bpp, w=w, h=h, fmt=fmt, stride=srow // bpp)
            if min_length is None:
                min_length = max(pw, ph) / 100.0
            capacity = max(int(capacity), 1)
            n = np.zeros(batch, np.int32)
            self.shape = (det["h"], det["w"])
            while True:
                out = np.zeros((batch, capacity), LINE_DTYPE)
                # (no transforms: the library's would be the prepared size's; the full size's are computed below)
                _check(lib().lr_find_line_segment_groups_batch_device(self._h, C.c_void_p(det["dptr"]), det["image_stride"], batch, det["w"], det["h"], det["stride"], min_length, frames_word(det["fmt"], refine), -1, _ptr(out), capacity, _ptr(n), C.byref(cfg), None))
                if int(n.max()) <= capacity:
                    break
                capacity = int(n.max())  # (a frame's lines were cut: once more, with room for the longest list)
            lines_list, transforms, good, Ms, sizes, rects, factors = [], [], [], [], [], [None] * batch, []
            for b in range(batch):
                lines = out[b][: n[b]].copy()
                if scale is not None:
                    for k in ("x1", "y1", "x2", "y2"):  # back to the coordinates of the full frame, in float32 as the demo
                        lines[k] = lines[k] / scale
                t = compute_rectification_transform(lines, w, h, cfg)
                lines_list.append(lines)
                transforms.append(t)
                try:
                    M, size, rects[b] = _rectified_map(t, clip, crop, cubic)
                except LibrectifyError:
                    continue  # (collinear corners, a size below 1, ...: this frame has no image)
                M, size, S = _bounded_map(M, size, out_max_size)
                good.append(b)
                Ms.append(M)
                sizes.append(size)
                factors.append(S)
            table = np.zeros((batch, (13 if words is None else 14) + (0 if out_max_size is None else 1)), np.float64)
            more = (rects,) if crop else ()
            if not good:
                return (lines_list, transforms, table, None, 0) + more
            table[good, :13], total = warp_table(np.stack(Ms), np.array(sizes, np.int64), bpp, 4)
            if words is not None:
                table[good, 13] = [words[b] for b in good]
            if out_max_size is not None:
                table[good, -1] = factors
            _check(lib().lr_device_malloc(self._h, total, C.byref(d_out)))
            # one launch; a frame without an image splits it, as a launch's frames are consecutive in the source
            runs = np.split(np.array(good), np.flatnonzero(np.diff(good) != 1) + 1)
            for run in runs:
                b0 = int(run[0])
                self.warp_perspective_packed_device(d_frames + b0 * simg, simg, len(run), w, h, srow, fmt | cubic | (0 if words is None else WARP_BORDER) | (0 if out_max_size is None else WARP_AREA), table[run], d_out.value, total)
            res, d_out = d_out.value, C.c_void_p()
            return (lines_list, transforms, table, res, total) + more
        finally:
            for p in (d_small, d_out):
                if p.value:
                    self.device_free(p.value)

    def _ragged_call(self, d_src, src_bytes, fmt_word, table, d_dst, dst_bytes, what):
        table = np.ascontiguousarray(table, np.float64)
        cols = 18 + ((17 if fmt_word & WARP_LENS_MODEL else 9) if fmt_word & WARP_LENS else 0) + (1 if fmt_word & WARP_AREA else 0)
        if table.ndim != 2 or table.shape[1] != cols or len(table) < 1:
            raise ValueError(what + ": the table has %d values per frame" % cols)
        bound = lambda col: int(min(max(np.nan_to_num(table[:, col]).max(), 1), 2 ** 31 - 1))  # noqa: E731
        _check(lib().lr_warp_perspective_device(self._h, C.c_void_p(d_src), src_bytes, len(table), bound(13), bound(14), 0, fmt_word, _ptr(table), C.c_void_p(d_dst), dst_bytes, bound(9), bound(10), 0))

    def warp_perspective_ragged_device(self, d_src, src_bytes, fmt, table, d_dst, dst_bytes):
        """lr_warp_perspective_device with LR_WARP_RAGGED: one launch for frames that have their own source size and place
        in the src_bytes at d_src and their own output size and place in the dst_bytes at d_dst.  table: 18 doubles per
        frame (ragged_table).  fmt may carry WARP_CUBIC, WARP_BORDER, and WARP_LENS with a table of 27 doubles per frame, or
        with WARP_LENS_MODEL 35 (ragged_table's lens=), and WARP_AREA with one more (ragged_table's area=)."""
        self._ragged_call(d_src, src_bytes, fmt | WARP_RAGGED, table, d_dst, dst_bytes, "warp_perspective_ragged_device")

    def prepare_ragged_device(self, d_src, src_bytes, fmt, table, d_dst, dst_bytes):
        """lr_warp_perspective_device with LR_WARP_RAGGED | LR_WARP_PREPARE: one launch that prepares every frame of the
        table from its own source size to its own output size (f32 gray; ragged_table with out_bpp=4; the maps are
        ignored)."""
        self._ragged_call(d_src, src_bytes, fmt | WARP_RAGGED | WARP_PREPARE, table, d_dst, dst_bytes, "prepare_ragged_device")

    def _find_frames(self, table, fmt, min_length, refine, capacity, cfg):
        """the batch detector on a frame table ((Frame * B) array): (out [B, capacity], n [B], transforms)"""
        batch = len(table)
        out = np.zeros((batch, capacity), LINE_DTYPE)
        n = np.zeros(batch, np.int32)
        tf = (ImageTransform * batch)()
        cfg = cfg or RectificationConfig()
        _check(lib().lr_find_line_segment_groups_batch_device(self._h, C.cast(table, C.c_void_p), C.sizeof(Frame), batch, 0, 0, 0, min_length, frames_word(fmt, refine), -1, _ptr(out), capacity, _ptr(n), C.byref(cfg), C.byref(tf)))
        return out, n, tf

    def find_line_segment_groups_frames_device(self, frames, fmt, min_length, refine=False, capacity=4096, cfg=None):
        """The batch detector on resident frames that each have their own size (lr_find_line_segment_groups_batch_device
        with a frame table).  frames: a (Frame * B) array, or B tuples (device address, width, height, stride in pixels of
        fmt[, min_length]); a frame's min_length below 0 (the default) is the call's.  Returns (lines_list, transforms):
        frame b's lines (at most `capacity` of them) and its ImageTransform for its own size."""
        if not isinstance(frames, C.Array):
            rows = [tuple(f) for f in frames]
            frames = (Frame * len(rows))(*[Frame(int(f[0]), int(f[1]), int(f[2]), int(f[3]), float(f[4]) if len(f) > 4 else -1.0) for f in rows])
        if len(frames) < 1:
            raise ValueError("find_line_segment_groups_frames_device: no frames")
        out, n, tf = self._find_frames(frames, fmt, min_length, refine, capacity, cfg)
        return [out[b][: min(int(n[b]), capacity)].copy() for b in range(len(frames))], tf

    def rectify_frames_device(self, d_base, sources, fmt, min_length=None, refine=False, cfg=None, clip=3.0, max_size=None,
                              capacity=4096, interp="linear", border=None, crop=False, out_max_size=None):
        """rectify for 8-bit frames (fmt PIX_U8 or PIX_U8X3) that are resident in HBM and have their OWN sizes: frame b is
        sources[b] = (width, height, byte_offset from d_base, row_bytes).  With max_size one ragged prepare
        (prepare_ragged_device) to prepared_size(w_b, h_b, max_size) per frame, one detector call with a frame table (on
        the 8-bit frames, or on the prepared ones; min_length float32(max(pw_b, ph_b) / 100) per frame unless given), on
        the host what rectify does per frame, and the ragged warp into one allocation: one launch per run of consecutive
        frames that have an image.  Returns (lines_list, transforms, table, d_out, total_bytes) like rectify_batch_device;
        table is ragged_table's (18 columns; an all-zero row for a frame without an image).  capacity and interp: as
        there (the ragged warp's sampling rule); border and crop likewise (the border words are the table's column 17; with
        crop=True the frames' rectangles are a sixth value).  out_max_size=N: every picture is at most N pixels on its longer
        side (rectify's out_max_size=: WARP_AREA on the ragged warp, the sampling factors behind the launch's rows; the table
        that comes back keeps its 18 columns, with the shrunk maps and sizes)."""
        return self._rectify_frames(d_base, sources, fmt, min_length, refine, cfg, clip, max_size, capacity, interp, border, crop, None, out_max_size)

    def _rectify_frames(self, d_base, sources, fmt, min_length, refine, cfg, clip, max_size, capacity, interp, border, crop, lens_rows=None, out_max_size=None):
        """rectify_frames_device; lens_rows (a _LensPlan, rectify_batch's lens= and lens_scale=): one WARP_LENS launch with the
        identity map (the plan's maps: lens_scale_map per frame), bilinear, zero border, writes every frame without its
        distortion into a second region of the sources' layout; the prepare step and the detector read that one, so lines and
        transforms are in (scaled) ideal coordinates; the warp reads the ORIGINAL frames with WARP_LENS and the plan's map @ M:
        one resampling.  Rows of seventeen (a LensModel among the lenses) add WARP_LENS_MODEL to both launches."""
        cubic = _sampling_bit(interp, "rectify_frames_device")
        _check_out_max_size("rectify_frames_device", out_max_size)
        if fmt not in (PIX_U8, PIX_U8X3):
            raise ValueError("rectify_frames_device: 8-bit frames, PIX_U8 or PIX_U8X3")
        sources = [tuple(int(v) for v in s) for s in sources]
        batch = len(sources)
        if batch < 1 or any(len(s) != 4 for s in sources):
            raise ValueError("rectify_frames_device: sources is B rows (width, height, byte_offset, row_bytes)")
        words = None if border is None else _border_words(border, batch, fmt, "rectify_frames_device")
        bpp = 3 if fmt == PIX_U8X3 else 1
        src_bytes = _source_extent(sources, bpp)
        if cfg is None:
            cfg = RectificationConfig(hmin=2.0)
        d_small, d_out, d_ideal = C.c_void_p(), C.c_void_p(), C.c_void_p()
        d_seen = d_base  # what the prepare step and the detector read
        try:
            frames = (Frame * batch)()
            if lens_rows is not None:
                lens_rows, lens_maps = lens_rows
                itable = np.zeros((batch, 18 + lens_rows.shape[1]), np.float64)
                itable[:, :9] = np.eye(3).reshape(9) if lens_maps is None else lens_maps.reshape(batch, 9)
                itable[:, 9:13] = itable[:, 13:17] = np.array(sources, np.float64)
                itable[:, 18:] = lens_rows
                _check(lib().lr_device_malloc(self._h, src_bytes, C.byref(d_ideal)))
                self.warp_perspective_ragged_device(d_base, src_bytes, fmt | _lens_bits(lens_rows), itable, d_ideal.value, src_bytes)
                self.synchronize()  # (the batch detector reads the frames on its lanes' streams, not after this one's work)
                d_seen = d_ideal.value
            if max_size is not None:
                prepared = [prepared_size(w, h, max_size) for w, h, _, _ in sources]
                ptable, small_bytes = ragged_table(None, np.array([p[:2] for p in prepared], np.int64), np.array(sources, np.int64), bpp, out_bpp=4)
                _check(lib().lr_device_malloc(self._h, small_bytes, C.byref(d_small)))
                self.prepare_ragged_device(d_seen, src_bytes, fmt, ptable, d_small.value, small_bytes)
                self.synchronize()  # (the batch detector reads the frames on its lanes' streams, not after this one's work)
                det_fmt = PIX_F32
                for b, (pw, ph, _) in enumerate(prepared):
                    frames[b] = Frame(d_small.value + int(ptable[b, 11]), pw, ph, int(ptable[b, 12]) // 4, -1.0)
                scales = [p[2] for p in prepared]
            else:
                if any(row % bpp for _, _, _, row in sources):
                    raise ValueError("rectify_frames_device: the detector takes strides in whole pixels")
                det_fmt = fmt
                for b, (w, h, off, row) in enumerate(sources):
                    frames[b] = Frame(d_seen + off, w, h, row // bpp, -1.0)
                scales = [None] * batch
            for f in frames:
                f.min_length = float(np.float32(max(f.width, f.height) / 100.0)) if min_length is None else float(min_length)
            capacity = max(int(capacity), 1)
            while True:
                # (the library's transforms would be the prepared sizes'; the full sizes' are computed below)
                out, n, _ = self._find_frames(frames, det_fmt, 0.0, refine, capacity, cfg)
                if int(n.max()) <= capacity:
                    break
                capacity = int(n.max())  # (a frame's lines were cut: once more, with room for the longest list)
            lines_list, transforms, good, Ms, sizes, rects, factors = [], [], [], [], [], [None] * batch, np.zeros((batch, 1), np.float64)
            for b, (w, h, _, _) in enumerate(sources):
                lines = out[b][: n[b]].copy()
                if scales[b] is not None:
                    for k in ("x1", "y1", "x2", "y2"):  # back to the coordinates of the full frame, in float32 as the demo
                        lines[k] = lines[k] / scales[b]
                t = compute_rectification_transform(lines, w, h, cfg)
                lines_list.append(lines)
                transforms.append(t)
                try:
                    M, size, rects[b] = _rectified_map(t, clip, crop, cubic)
                except LibrectifyError:
                    continue  # (collinear corners, a size below 1, ...: this frame has no image)
                M, size, S = _bounded_map(M, size, out_max_size)
                if lens_rows is not None and lens_maps is not None:
                    M = lens_scale_compose(lens_maps[b], M)  # (from the scaled ideal picture, where the detector saw the lines, to the ideal one)
                good.append(b)
                Ms.append(M)
                sizes.append(size)
                factors[b] = S or 0
            table = np.zeros((batch, 18), np.float64)
            more = (rects,) if crop else ()
            if not good:
                return (lines_list, transforms, table, None, 0) + more
            table[good], total = ragged_table(np.stack(Ms), np.array(sizes, np.int64), np.array([sources[b] for b in good], np.int64), bpp, align=4)
            if words is not None:
                table[good, 17] = [words[b] for b in good]
            _check(lib().lr_device_malloc(self._h, total, C.byref(d_out)))
            bits = cubic | (0 if words is None else WARP_BORDER) | (0 if lens_rows is None else _lens_bits(lens_rows)) | (0 if out_max_size is None else WARP_AREA)
            for run in np.split(np.array(good), np.flatnonzero(np.diff(good) != 1) + 1):
                rows = table[run] if lens_rows is None else np.concatenate([table[run], lens_rows[run]], axis=1)
                if out_max_size is not None:
                    rows = np.concatenate([rows, factors[run]], axis=1)
                self.warp_perspective_ragged_device(d_base, src_bytes, fmt | bits, rows, d_out.value, total)
            res, d_out = d_out.value, C.c_void_p()
            return (lines_list, transforms, table, res, total) + more
        finally:
            for p in (d_small, d_out, d_ideal):
                if p.value:
                    self.device_free(p.value)

    def _jpeg_results(self, d_out, total, fmt, table, quality, optimize=False):
        """the warped pictures at d_out (rows of `table`: columns 9..12 width, height, offset, stride) as JPEG files"""
        good = [b for b in range(len(table)) if table[b, 9]]
        streams = self._encode_resident(d_out, total, fmt, [tuple(int(v) for v in table[b, 9:13]) for b in good], quality, 0, optimize) if good else []
        out = [None] * len(table)
        for b, s in zip(good, streams):
            out[b] = s
        return out

    def _tensor_of_warped(self, d_out, total, fmt, table, spec, tensor_out):
        """tensor= of the rectify calls: the warped pictures at d_out (rows of `table`: columns 0..8 the launch's map, 9..12
        width, height, offset, stride) packed where they lie, frame b into slot b (a frame without a picture: pad).  Returns
        (tensor, maps): pack_tensor's return and per frame the tensor map (None without a picture)."""
        frames = [tuple(int(v) for v in table[b, 9:13]) if table[b, 9] else None for b in range(len(table))]
        packed = self._pack_resident(d_out or 0, total, fmt, frames, spec, tensor_out)
        maps = []
        for b, f in enumerate(frames):
            if f is None:
                maps.append(None)
                continue
            left, top = ((spec.width - f[0]) // 2, (spec.height - f[1]) // 2) if spec.place == "center" else (0, 0)
            maps.append(tensor_map(table[b, :9], left, top))
        return packed, maps

    def _rectify_mixed(self, frames, min_length, refine, cfg, clip, max_size, capacity, jpeg=None, interp="linear", jpeg_optimize=False, border=None, crop=False,
                       lens=None, out_max_size=None, tensor=None):
        """rectify_batch for a list of 8-bit frames of different shapes: all frames in one host buffer, one upload,
        rectify_frames_device, one download"""
        frames = [np.ascontiguousarray(f) for f in frames]
        if any(f.dtype != np.uint8 or not (f.ndim == 2 or (f.ndim == 3 and f.shape[2] == 3)) for f in frames):
            raise ValueError("rectify_batch: uint8 frames, H x W or H x W x 3")
        if len({f.ndim for f in frames}) != 1:
            raise ValueError("rectify_batch: the frames are all H x W or all H x W x 3")
        fmt, bpp = _frame_format(frames[0], "rectify_batch")
        sources, end = [], 0
        for f in frames:
            start = (end + 3) // 4 * 4
            sources.append((f.shape[1], f.shape[0], start, f.shape[1] * bpp))
            end = start + f.nbytes
        host = np.zeros(end, np.uint8)
        for f, (_, _, start, _) in zip(frames, sources):
            host[start: start + f.nbytes] = f.reshape(-1)
        _border_words(border, len(frames), fmt, "rectify_batch")  # (a bad spec: ValueError before anything goes up)
        return self._rectify_resident(self.device_upload(host), sources, fmt, min_length, refine, cfg, clip, max_size, capacity, jpeg, interp, jpeg_optimize, border, crop, lens, out_max_size, tensor)

    def _rectify_resident(self, d_src, sources, fmt, min_length, refine, cfg, clip, max_size, capacity, jpeg, interp="linear", jpeg_optimize=False, border=None, crop=False,
                          lens=None, out_max_size=None, tensor=None):
        """rectify_batch for 8-bit frames (width, height, byte_offset, row_bytes) that lie at d_src, which is freed here:
        rectify_frames_device, then one download of the pictures, or with jpeg the encoder and the streams alone; with tensor
        (the TensorSpec and tensor_out) the pictures are packed where they lie as well, every result gets its tensor map and
        the return is (results, tensor)"""
        bpp = 3 if fmt == PIX_U8X3 else 1
        d_out = None
        try:
            lines, tfs, table, d_out, total, *more = self._rectify_frames(d_src, sources, fmt, min_length, refine, cfg, clip, max_size, capacity, interp, border, crop, lens, out_max_size)
            rect = (lambda b: (more[0][b],)) if crop else (lambda b: ())
            with_tensor = lambda results: results  # noqa: E731
            if tensor is not None:
                packed_tensor, maps = self._tensor_of_warped(d_out, total, fmt, table, *tensor)
                crop_rect, rect = rect, lambda b: crop_rect(b) + (maps[b],)
                with_tensor = lambda results: (results, packed_tensor)  # noqa: E731
            if jpeg is not None:
                streams = self._jpeg_results(d_out, total, fmt, table, jpeg, jpeg_optimize) if d_out else [None] * len(sources)
                return with_tensor([(lines[b], tfs[b], streams[b]) + rect(b) for b in range(len(sources))])
            packed = self.device_download(d_out, (total,), np.uint8) if d_out else None
        finally:
            self.device_free(d_src)
            if d_out:
                self.device_free(d_out)
        res = []
        for b in range(len(sources)):
            ow, oh, off, row = (int(v) for v in table[b, 9:13])
            img = None
            if ow:
                rows = np.lib.stride_tricks.as_strided(packed[off:], (oh, ow * bpp), (row, 1))
                img = np.ascontiguousarray(rows).reshape((oh, ow) + ((3,) if bpp == 3 else ()))
            res.append((lines[b], tfs[b], img) + rect(b))
        return with_tensor(res)

    def rectify_batch(self, frames_u8, min_length=None, refine=False, cfg=None, clip=3.0, max_size=None, capacity=4096, jpeg=None,
                      orient=False, interp="linear", jpeg_optimize=False, any_sampling=False, border=None, crop=False, decode_scale=None,
                      decode_max_size=None, lens=None, out_max_size=None, lens_scale=1, tensor=None, tensor_out=None):
        """Context.rectify for a batch: frames_u8 is a uint8 array [B, H, W] or [B, H, W, 3], or a list of such frames of one
        shape.  One upload, rectify_batch_device (one detector batch, the packed warp), one download.  Returns a
        list of (lines, transform, warped), frame by frame what rectify returns for it; warped is None for a frame whose
        homography cannot be formed.  A list of frames of DIFFERENT shapes (all H x W or all H x W x 3) takes the
        mixed-size pipeline: all frames in one host buffer, one upload, rectify_frames_device (one ragged prepare, one
        detector call with a frame table, one ragged warp launch), one download -- frame by frame what rectify returns.
        jpeg=Q (1 .. 100): the warped pictures stay in HBM and are encoded there (lr_encode_jpeg_device, quality Q, 4:2:0 for
        colour frames); `warped` is then the JPEG file as bytes -- exactly the encoder's stream of the picture that jpeg=None
        returns -- and only the streams' lengths and the streams cross the link.  A frame whose stream outgrows a first
        extent of half its pixels' bytes is encoded again with room for jpeg_bound, so nothing is ever cut.
        jpeg_optimize=True (with jpeg=Q, else ValueError): every file is coded with Huffman tables made from its own symbols
        (LR_JPEG_OPTIMIZE): the same pixels, about 15 % fewer bytes at quality 95.
        A list of JPEG files (bytes; all of them, else ValueError) in place of the frames: the files are uploaded and
        decoded in HBM (lr_decode_jpeg_device; u8x3, or u8 if every file has one component) and handed to
        rectify_frames_device where they lie -- bit for bit the call on decode_jpeg_batch's arrays (decode_jpeg_batch(files,
        PIX_U8)'s for a list of one-component files); with jpeg=Q no pixel crosses the link in either direction.
        orient=True (JPEG files only, else ValueError): the files' EXIF orientations are applied in the decoder's output
        pass, as the demo's imread applies them -- bit for bit the call on decode_jpeg_batch(files, orient=True)'s arrays.
        any_sampling=True (JPEG files only, else ValueError): the decoder call carries LR_JPEG_ANY_SAMPLING, so that files of
        4:4:0 (a losslessly rotated 4:2:2 photograph), 4:1:1 and every other sampling with factors 1, 2 or 4 are decoded --
        bit for bit the call on decode_jpeg_batch(files, any_sampling=True)'s arrays.  Without it the first such file raises
        LibrectifyError (status 2) for the whole batch.
        decode_scale=N (JPEG files only, else ValueError; None, an int or one per file out of 1, 2, 4, 8): the files are
        decoded at 1/N of their size (LR_JPEG_SCALED): the call on decode_jpeg_batch(files, scale=N)'s arrays, every later
        stage working on 1/N^2 of the pixels.  decode_max_size=M instead (both: ValueError): per file the largest N whose
        longer side ceil(max(w, h) / N) is still at least M (jpeg_scale_for, PIL's Image.draft rule).  Segments, transforms
        and homographies that come back are in the DECODED picture's coordinates: multiply by N for the file's.
        interp="cubic": the warp launch of whichever path is taken samples 4 x 4 bicubic (WARP_CUBIC); detector, transforms,
        sizes and the encoder are untouched -- frame by frame what rectify(interp="cubic") returns.
        border: None, one border_word spec for all frames or a list of one per frame (WARP_BORDER on the warp launch of
        whichever path is taken); crop=True: every picture, or JPEG file, is its constrained crop and every result has a fourth
        entry, the rectangle (x0, y0, width, height) -- frame by frame what rectify(border=, crop=) returns.
        lens: None, one Lens for all frames or a list of one per frame, in which None means no lens (WARP_LENS): frame by frame
        what rectify(lens=) returns.  Arrays and files alike then take the mixed-size pipeline, with one WARP_LENS launch in
        front of it that writes the frames without their distortion for the detector, and the final warp reading the frames
        as they were uploaded or decoded.  With crop=True: ValueError.  A LensModel for all frames, or Lens, LensModel and
        None mixed in the list: both launches then carry WARP_LENS_MODEL as well.  lens_scale=s (with lens=, else ValueError):
        rectify's, for every frame whose lens is not None.
        out_max_size=N: every picture, or JPEG file, is at most N pixels on its longer side (WARP_AREA on the warp launch of
        whichever path is taken, after the crop and in front of the encoder) -- frame by frame what rectify(out_max_size=N)
        returns.  The full-size pictures never exist: HBM holds, the link carries and the encoder reads the small ones.
        tensor=spec (a TensorSpec; with out_max_size=: ValueError, the tensor's box is the bound): the pictures become a
        network's input in HBM as well.  After the crop every frame is bounded as out_max_size=fit_box(size_b, (W, H)) bounds
        it, so that it fits the spec's H x W slot; the pictures stay in HBM, and one lr_pack_tensor_device call packs frame b
        into slot b of a B-slot tensor (a frame without a picture: a slot of pad); jpeg=Q still encodes the same pictures.
        The call then returns (results, tensor): results[b] is what rectify(frame_b, ..., out_max_size=fit_box(...)) returns
        with one more entry at its end, the 3 x 3 float64 TENSOR MAP (None without a picture), which takes a tensor pixel (x,
        y) of slot b to the coordinates the warp launch read from (that launch's map composed with the translation by
        (-left, -top): tensor_map), so a network's boxes go back onto the photograph; tensor is pack_tensor's return, with
        tensor_out= as its out= (a torch tensor on the context's device, written in place; nothing of it is downloaded)."""
        out_max_size = _check_tensor("rectify_batch", tensor, tensor_out, out_max_size)
        _sampling_bit(interp, "rectify_batch")
        _check_out_max_size("rectify_batch", out_max_size)
        packing = None if tensor is None else (tensor, tensor_out)
        _check_jpeg_optimize("rectify_batch", jpeg, jpeg_optimize)
        if lens is not None:
            if crop:
                raise ValueError("rectify_batch: crop=True together with lens= (the crop's rectangle assumes straight source edges)")
            s = _check_lens_scale("rectify_batch", lens_scale)
            rows = _lens_rows(lens, len(frames_u8), "rectify_batch")
            maps = None
            if s != 1.0:
                given = [True] * len(rows) if isinstance(lens, (Lens, LensModel)) else [v is not None for v in lens]
                maps = np.stack([lens_scale_map(Lens(*r[:9]), s) if g else np.eye(3) for r, g in zip(rows, given)])
            lens = _LensPlan(rows, maps)
        elif _check_lens_scale("rectify_batch", lens_scale) != 1.0:
            raise ValueError("rectify_batch: lens_scale goes with lens=")
        if _all_streams(frames_u8, "rectify_batch", orient, any_sampling, decode_scale, decode_max_size):
            try:  # (the files' format is known once they are decoded: a spec that suits neither 8-bit format fails here)
                _border_words(border, len(frames_u8), PIX_U8X3, "rectify_batch")
            except ValueError:
                _border_words(border, len(frames_u8), PIX_U8, "rectify_batch")
            return self._rectify_streams([bytes(f) for f in frames_u8], min_length, refine, cfg, clip, max_size, capacity, jpeg, orient, interp, jpeg_optimize,
                                         any_sampling, border, crop, decode_scale, decode_max_size, lens, out_max_size, packing)
        if lens is not None:
            return self._rectify_mixed(list(frames_u8), min_length, refine, cfg, clip, max_size, capacity, jpeg, interp, jpeg_optimize, border, crop, lens, out_max_size, packing)
        if not isinstance(frames_u8, np.ndarray):
            frames_u8 = [np.asarray(f) for f in frames_u8]
            if len({f.shape for f in frames_u8}) > 1:
                return self._rectify_mixed(frames_u8, min_length, refine, cfg, clip, max_size, capacity, jpeg, interp, jpeg_optimize, border, crop, None, out_max_size, packing)
        a = np.ascontiguousarray(frames_u8 if isinstance(frames_u8, np.ndarray) else np.stack([np.asarray(f) for f in frames_u8]))
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or (a.ndim == 4 and a.shape[3] != 3) or a.shape[0] < 1:
            raise ValueError("rectify_batch: uint8 frames [B, H, W] or [B, H, W, 3]")
        fmt, bpp = _frame_format(a[0], "rectify_batch")
        batch, h, w = a.shape[:3]
        _border_words(border, batch, fmt, "rectify_batch")  # (a bad spec: ValueError before anything goes up)
        d_src = self.device_upload(a)
        d_out = None
        try:
            lines, tfs, table, d_out, total, *more = self.rectify_batch_device(d_src, batch, w, h, fmt, min_length=min_length, refine=refine, cfg=cfg, clip=clip, max_size=max_size, capacity=capacity, interp=interp, border=border, crop=crop, out_max_size=out_max_size)
            rect = (lambda b: (more[0][b],)) if crop else (lambda b: ())
            with_tensor = lambda results: results  # noqa: E731
            if tensor is not None:
                packed_tensor, maps = self._tensor_of_warped(d_out, total, fmt, table, tensor, tensor_out)
                crop_rect, rect = rect, lambda b: crop_rect(b) + (maps[b],)
                with_tensor = lambda results: (results, packed_tensor)  # noqa: E731
            if jpeg is not None:
                streams = self._jpeg_results(d_out, total, fmt, table, jpeg, jpeg_optimize) if d_out else [None] * batch
                return with_tensor([(lines[b], tfs[b], streams[b]) + rect(b) for b in range(batch)])
            packed = self.device_download(d_out, (total,), np.uint8) if d_out else None
        finally:
            self.device_free(d_src)
            if d_out:
                self.device_free(d_out)
        res = []
        for b in range(batch):
            ow, oh, off, row = (int(v) for v in table[b, 9:13])
            img = None
            if ow:
                rows = np.lib.stride_tricks.as_strided(packed[off:], (oh, ow * bpp), (row, 1))
                img = np.ascontiguousarray(rows).reshape((oh, ow) + a.shape[3:])
            res.append((lines[b], tfs[b], img) + rect(b))
        return with_tensor(res)

    def set_seed_capacity(self, cap):
        lib().lr_set_seed_capacity(self._h, int(cap))

    def set_flood_staged(self, on):
        lib().lr_set_flood_staged(self._h, int(bool(on)))

    def set_flood_blind_rounds(self, rounds):
        lib().lr_set_flood_blind_rounds(self._h, int(rounds))

    def set_batch_streams(self, n):
        lib().lr_set_batch_streams(self._h, int(n))

    def find_line_segment_groups_batch_device(self, dptr, image_stride, batch, w, h, min_length, refine=False, capacity=4096, cfg=None, out=None, fmt=PIX_F32, stride=None):
        """fmt: the resident frames' format; image_stride (and stride, default w) in pixels of it"""
        if out is None:
            out = np.zeros((batch, capacity), LINE_DTYPE)
        n = np.zeros(batch, np.int32)
        tf = (ImageTransform * batch)()
        cfg = cfg or RectificationConfig()
        self.shape = (h, w)
        _check(lib().lr_find_line_segment_groups_batch_device(self._h, C.c_void_p(dptr), image_stride, batch, w, h, stride or w, min_length, frames_word(fmt, refine), -1, _ptr(out), capacity, _ptr(n), C.byref(cfg), C.byref(tf)))
        return out, n, tf

    def find_line_segment_groups_batch_host(self, frames, min_length, refine=False, num_threads=-1, capacity=4096, cfg=None, out=None, devices=None):
        """frames: float32 array [B, H, W] (rows contiguous; any row/frame strides) or a list of 2-D float32 arrays
        of one shape, in HOST memory (pageable, or page-locked as host_alloc returns it); or 8-bit frames: a uint8 array
        [B, H, W] or [B, H, W, 3], or a list of such frames.  devices: a list of device indices to deal the frames over in
        contiguous blocks (lr_find_line_segment_groups_batch_host_multi)."""
        fmt, array_stride = PIX_F32, None
        if isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.ndim in (3, 4):
            _, fmt, bpp, stride = _host_frame(frames[0], "find_line_segment_groups_batch_host")
            batch, h, w = frames.shape[:3]
            ptrs = (C.c_void_p * batch)(*[frames.ctypes.data + b * frames.strides[0] for b in range(batch)])
            if frames.strides[0] > 0 and frames.strides[0] % bpp == 0:  # (one array: the entry that takes a frame stride)
                array_stride = frames.strides[0] // bpp
        elif isinstance(frames, np.ndarray) and frames.ndim == 3:
            assert frames.dtype == np.float32 and frames.strides[2] == 4
            batch, h, w = frames.shape
            stride = frames.strides[1] // 4
            ptrs = (C.c_void_p * batch)(*[frames.ctypes.data + b * frames.strides[0] for b in range(batch)])
        elif len(frames) and np.asarray(frames[0]).dtype == np.uint8:
            frames = [_host_frame(f, "find_line_segment_groups_batch_host") for f in frames]
            fmt, stride = frames[0][1], frames[0][3]
            frames = [f[0] for f in frames]
            batch = len(frames)
            h, w = frames[0].shape[:2]
            assert all(f.dtype == np.uint8 and f.shape == frames[0].shape and f.strides == frames[0].strides for f in frames)
            ptrs = (C.c_void_p * batch)(*[f.ctypes.data for f in frames])
        else:
            frames = [np.asarray(f, np.float32) for f in frames]
            batch = len(frames)
            h, w = frames[0].shape
            stride = frames[0].strides[0] // 4
            assert all(f.shape == (h, w) and f.strides == frames[0].strides and f.strides[1] == 4 for f in frames)
            ptrs = (C.c_void_p * batch)(*[f.ctypes.data for f in frames])
        word = frames_word(fmt, refine)
        if out is None:
            out = np.zeros((batch, capacity), LINE_DTYPE)
        n = np.zeros(batch, np.int32)
        tf = (ImageTransform * batch)()
        cfg = cfg or RectificationConfig()
        self.shape = (h, w)
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(lib().lr_find_line_segment_groups_batch_host_multi(self._h, devs, len(devices), ptrs, batch, w, h, stride, min_length, word, num_threads, _ptr(out), capacity, _ptr(n), C.byref(cfg), C.byref(tf)))
            return out, n, tf
        if array_stride is not None:
            _check(lib().lr_find_line_segment_groups_batch_host(self._h, C.c_void_p(frames.ctypes.data), array_stride, batch, w, h, stride, min_length, word, num_threads, _ptr(out), capacity, _ptr(n), C.byref(cfg), C.byref(tf)))
            return out, n, tf
        _check(lib().lr_find_line_segment_groups_batch_host_ptrs(self._h, ptrs, batch, w, h, stride, min_length, word, num_threads, _ptr(out), capacity, _ptr(n), C.byref(cfg), C.byref(tf)))
        return out, n, tf

    def host_alloc(self, shape, dtype=np.float32):
        """Page-locked host array (free with host_free(array)): frames in it are uploaded without a staging copy."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _check(lib().lr_host_alloc(self._h, nbytes, C.byref(p)))
        buf = (C.c_ubyte * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, array):
        p = self._pinned.pop(array.ctypes.data)
        _check(lib().lr_host_free(self._h, C.c_void_p(p)))

    # ---- RANSAC ----
    def ransac_best(self, lines_norm, indices, tol, n_iter, seed, rnd=0):
        lines_norm = np.ascontiguousarray(lines_norm, LINE_DTYPE)
        indices = np.ascontiguousarray(indices, np.int32)
        bh = np.zeros(3, np.float32)
        bs = C.c_float(0)
        bi = C.c_int(0)
        _check(lib().lr_ransac_best(self._h, _ptr(lines_norm), len(lines_norm), _ptr(indices), len(indices), tol, n_iter, C.c_uint64(seed), C.c_uint32(rnd), _ptr(bh), C.byref(bs), C.byref(bi)))
        return dict(best_h=bh, score=bs.value, iter=bi.value)

    def cht_vanishing_point(self, lines, d=128):
        lines = np.ascontiguousarray(lines, LINE_DTYPE)
        vp = Point()
        acc = np.zeros((d, d), np.uint64)
        _check(lib().lr_cht_vanishing_point(self._h, _ptr(lines), len(lines), d, C.byref(vp), _ptr(acc)))
        return np.array([vp.x, vp.y, vp.z], np.float32), acc

    def refine_lines(self, lines):
        lines = np.ascontiguousarray(lines, LINE_DTYPE)
        out = np.zeros(len(lines), LINE_DTYPE)
        n = C.c_int(0)
        _check(lib().lr_refine_lines(self._h, _ptr(lines), len(lines), _ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def set_flood_partial_commits(self, on=True):
        lib().lr_set_flood_partial_commits(self._h, int(bool(on)))

    def set_flood_just_in_time(self, on=True):
        lib().lr_set_flood_just_in_time(self._h, int(bool(on)))

    def trim(self):
        """gives the memory that is sized by the largest frame seen back to the system (the next call allocates what it needs)"""
        _check(lib().lr_context_trim(self._h))

    def set_flood_giant_step(self, on=True):
        """the lowest active seed's flood by the whole device when it outgrows the LDS tiers (default); False = the slab walk"""
        lib().lr_set_flood_giant_step(self._h, int(bool(on)))

    def set_flood_logs(self, on=1):
        """0 = off, 1 = on (default for single calls), 2 = on with every log through the fall-back path (test hook)."""
        lib().lr_set_flood_logs(self._h, int(on))

    def set_flood_schedule(self, order=0, seed=0, width=0):
        """Test hook: the order of a flood round's active list (0 as is, 1 reversed, 2 flood_schedule_perm of (seed, round,
        length)) and the workgroups of every launch that walks it (0: its own grid, 1: a serial round).  Single calls and stage
        calls; stage_counters()["scheduled_rounds"] counts the rounds enqueued under it."""
        lib().lr_set_flood_schedule(self._h, int(order), int(seed) & 0xFFFFFFFF, int(width))

    def set_stage_timing(self, on=True):
        """stage timers of the frame calls (off by default: each event record idles the GPU for a few microseconds)"""
        lib().lr_set_stage_timing(self._h, int(bool(on)))

    def set_estimator(self, kind, param=-1):
        """0 RANSAC (default), 1 PROSAC (param = T_N), 2 DirectEstimator, 3 diamond-space accumulator (param = its size d)."""
        lib().lr_set_estimator(self._h, int(kind), int(param))

    def estimate_line_pencils_cht(self, lines, max_models=4, inlier_deg=2.0, garbage_deg=4.0, d=128):
        """-> (lines with group_id, refit models (k, 3), winning cells (k,), cells voted for)"""
        lines = np.ascontiguousarray(lines, LINE_DTYPE).copy()
        models = np.zeros((max(max_models, 1), 3), np.float32)
        cells = np.zeros(max(max_models, 1), np.uint32)
        k = C.c_int(0)
        votes = C.c_uint64(0)
        _check(lib().lr_estimate_line_pencils_cht(self._h, _ptr(lines), len(lines), max_models, inlier_deg, garbage_deg, d, _ptr(models), C.byref(k), _ptr(cells), C.byref(votes)))
        return lines, models[: k.value].copy(), cells[: k.value].copy(), int(votes.value)

    def ht_weights(self, lines_norm, indices):
        lines_norm = np.ascontiguousarray(lines_norm, LINE_DTYPE)
        indices = np.ascontiguousarray(indices, np.int32)
        out = np.zeros(len(indices), np.float32)
        _check(lib().lr_ht_weights(self._h, _ptr(lines_norm), len(lines_norm), _ptr(indices), len(indices), _ptr(out)))
        return out

    def prosac_solve(self, lines_norm, indices, tol, T_N=-1, seed=0, rnd=0):
        lines_norm = np.ascontiguousarray(lines_norm, LINE_DTYPE)
        indices = np.ascontiguousarray(indices, np.int32)
        h = np.zeros(3, np.float32)
        tr = np.zeros(4, np.int32)
        _check(lib().lr_prosac_solve(self._h, _ptr(lines_norm), len(lines_norm), _ptr(indices), len(indices), tol, T_N, C.c_uint64(seed), C.c_uint32(rnd), _ptr(h), _ptr(tr)))
        return dict(h=h, iterations=int(tr[0]), n_star=int(tr[1]), best_iter=int(tr[2]), I_N_best=int(tr[3]))

    def estimate_line_pencils_prosac(self, lines, max_models=4, inlier_deg=2.0, garbage_deg=4.0, T_N=-1, seed=0):
        lines = np.ascontiguousarray(lines, LINE_DTYPE).copy()
        _check(lib().lr_estimate_line_pencils_prosac(self._h, _ptr(lines), len(lines), max_models, inlier_deg, garbage_deg, T_N, C.c_uint64(seed)))
        return lines

    def direct_solve(self, lines_norm, indices):
        lines_norm = np.ascontiguousarray(lines_norm, LINE_DTYPE)
        indices = np.ascontiguousarray(indices, np.int32)
        h = np.zeros(3, np.float32)
        _check(lib().lr_direct_solve(self._h, _ptr(lines_norm), len(lines_norm), _ptr(indices), len(indices), _ptr(h)))
        return h

    def estimate_line_pencils_direct(self, lines, max_models=4, inlier_deg=2.0, garbage_deg=4.0):
        lines = np.ascontiguousarray(lines, LINE_DTYPE).copy()
        _check(lib().lr_estimate_line_pencils_direct(self._h, _ptr(lines), len(lines), max_models, inlier_deg, garbage_deg))
        return lines

    def estimate_line_pencils(self, lines, max_models=4, inlier_deg=2.0, garbage_deg=4.0, n_iter=10000, seed=0):
        lines = np.ascontiguousarray(lines, LINE_DTYPE).copy()
        _check(lib().lr_estimate_line_pencils(self._h, _ptr(lines), len(lines), max_models, inlier_deg, garbage_deg, n_iter, C.c_uint64(seed)))
        return lines


# ---- the reference's six functions, by name --------------------------------------------------

def release_thread_context():
    """frees the calling thread's drop-in context (the next drop-in call makes a new one)"""
    lib().lr_release_thread_context()


def find_line_segment_groups(buffer, min_length, refine=False, num_threads=-1):
    """reference find_line_segment_groups (src/librectify.h:111-116) on a 2-D float32 array.
    Returns a LINE_DTYPE array (empty where the reference returns NULL)."""
    buffer = np.asarray(buffer, np.float32)
    h, w = buffer.shape
    assert buffer.strides[1] == 4
    n = C.c_int(0)
    p = lib().find_line_segment_groups(_ptr(buffer), w, h, buffer.strides[0] // 4, min_length, bool(refine), num_threads, C.byref(n))
    if not p:
        err = lib().lr_last_error().decode()
        if err:  # NULL because of a missing GPU / HIP failure, not because nothing was found
            raise LibrectifyError(err)
        return np.zeros(0, LINE_DTYPE)
    out = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(n.value * LINE_DTYPE.itemsize,)).view(LINE_DTYPE).copy()
    pp = C.c_void_p(p)
    lib().release_line_segments(C.byref(pp))
    assert pp.value is None
    return out


def compute_rectification_transform(lines, width, height, cfg=None):
    lines = np.ascontiguousarray(lines, LINE_DTYPE)
    cfg = cfg or RectificationConfig()
    return lib().compute_rectification_transform(_ptr(lines), len(lines), width, height, C.byref(cfg))


def compute_rectification_transform_from_vp(width, height, vp_h, vp_v):
    a = Point(*[float(v) for v in vp_h])
    b = Point(*[float(v) for v in vp_v])
    return lib().compute_rectification_transform_from_vp(width, height, C.byref(a), C.byref(b))


def rectification_homography(t, clip=3.0):
    """lr_rectification_homography (the reference demo's homography_from_corners; host only) on an ImageTransform.
    Returns (H, M, (width, height)): H (3x3) maps the source frame into the rectified image of that size, M = H^-1 the
    rectified image back into the source (what the warp takes)."""
    H = np.zeros(9, np.float64)
    M = np.zeros(9, np.float64)
    w, h = C.c_int(0), C.c_int(0)
    _check(lib().lr_rectification_homography(C.byref(t), clip, _ptr(H), _ptr(M), C.byref(w), C.byref(h)))
    return H.reshape(3, 3), M.reshape(3, 3), (w.value, h.value)


def fit_vanishing_point(lines, group):
    lines = np.ascontiguousarray(lines, LINE_DTYPE)
    p = lib().fit_vanishing_point(_ptr(lines), len(lines), group)
    return np.array([p.x, p.y, p.z], np.float32)


def assign_to_group(lines, new_lines, angular_tolerance):
    lines = np.ascontiguousarray(lines, LINE_DTYPE)
    new_lines = np.ascontiguousarray(new_lines, LINE_DTYPE).copy()
    lib().assign_to_group(_ptr(lines), len(lines), _ptr(new_lines), len(new_lines), angular_tolerance)
    return new_lines
