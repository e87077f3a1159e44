"""aeon_amd -- MI355X (gfx950) image-augmentation stage for NervanaSystems/aeon.

Python binding of the C ABI in include/aeon_hip.h (libaeon_hip.so, built in-tree).
The pixel path runs only in the HIP kernels of that library: there is no CPU fallback, and
importing this package fails loudly when the library is missing.  PyTorch is used only as
plumbing (device memory and streams) by callers; the binding itself takes raw pointers.
"""
import ctypes
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# AEON_HIP_LIB: a kernel tuning variant built by tools/build_variants.sh (development only)
LIB_PATH = os.environ.get("AEON_HIP_LIB") or os.path.join(HERE, "libaeon_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "aeon_hip.h")

AEON_HIP_OK = 0
AEON_HIP_EINVAL = -1
AEON_HIP_ERUNTIME = -2
AEON_HIP_EUNSUPPORTED = -3
AEON_HIP_EDEVICE = -4

DTYPE_U8 = 0
DTYPE_F32 = 1
# output dtype name -> (AEON_DTYPE_* code, numpy type); aeon output_type uint32_t maps to int32 storage
DTYPES = {"uint8": (0, np.uint8), "float32": (1, np.float32), "int8": (2, np.int8), "int16": (3, np.int16),
          "uint16": (4, np.uint16), "int32": (5, np.int32), "float64": (6, np.float64),
          # image outputs only: the float32 output rounded once to the 16-bit type.  numpy has no bfloat16:
          # its arrays are uint16 carrying the bfloat16 bits (as_torch views them as torch.bfloat16)
          "float16": (7, np.float16), "bfloat16": (8, np.uint16)}
NP_DTYPE = {code: t for code, t in DTYPES.values()}
TYPE_NAME = {code: name for name, (code, _) in DTYPES.items()}


def as_torch(array, type_name):
    """A decoder / stage output array as a torch tensor sharing its memory: torch.float16 for "float16",
    torch.bfloat16 for "bfloat16" (whose numpy arrays hold the bits as uint16), else the array's own type."""
    import torch
    if type_name == "bfloat16":
        if array.dtype != np.uint16:
            raise TypeError("bfloat16 outputs are uint16 arrays of the bfloat16 bits")
        return torch.from_numpy(array.view(np.int16)).view(torch.bfloat16)
    if type_name == "float16" and array.dtype != np.float16:
        raise TypeError("float16 outputs are float16 arrays")
    return torch.from_numpy(array)
INTERP_LINEAR = 0
INTERP_NEAREST = 1
INTERP_CUBIC = 2
INTERP_AREA = 3
INTERP_LANCZOS4 = 4


class ImgDesc(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("channels", ctypes.c_int32), ("elem_bytes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class AugParams(ctypes.Structure):
    """POD mirror of augment::image::params (aeon src/augment_image.hpp:99-119)."""
    _fields_ = [
        ("crop_x", ctypes.c_int32), ("crop_y", ctypes.c_int32),
        ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
        ("resize_short_size", ctypes.c_int32),
        ("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32),
        ("angle", ctypes.c_int32), ("flip", ctypes.c_int32),
        ("padding", ctypes.c_int32), ("pad_off_x", ctypes.c_int32), ("pad_off_y", ctypes.c_int32),
        ("n_lighting", ctypes.c_int32), ("lighting", ctypes.c_float * 3),
        ("color_noise_std", ctypes.c_float),
        ("contrast", ctypes.c_float), ("brightness", ctypes.c_float),
        ("saturation", ctypes.c_float), ("hue", ctypes.c_int32),
        ("interp", ctypes.c_int32),
        ("expand_ratio", ctypes.c_float), ("expand_x", ctypes.c_int32), ("expand_y", ctypes.c_int32),
        ("expand_w", ctypes.c_int32), ("expand_h", ctypes.c_int32),
    ]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["lighting"] = list(self.lighting)
        return d


class OutDesc(ctypes.Structure):
    """image::loader configuration + batch item stride (aeon src/etl_image.cpp:204-244)."""
    _fields_ = [("dtype", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("channel_major", ctypes.c_int32), ("bgr_to_rgb", ctypes.c_int32),
                ("has_mean", ctypes.c_int32), ("fixed_aspect_ratio", ctypes.c_int32),
                ("mean", ctypes.c_double * 3), ("stddev", ctypes.c_double * 3),
                ("item_stride", ctypes.c_uint64), ("canvas_w", ctypes.c_int32), ("canvas_h", ctypes.c_int32)]


class RecordElem(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("stride", ctypes.c_int32)]


class EncodedElem(ctypes.Structure):
    """aeon_encoded_elem: an encoded JPEG file (width 0) or decoded HWC uint8 pixels."""
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_size_t), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("channels", ctypes.c_int32), ("stride", ctypes.c_int32)]


class AviFrame(ctypes.Structure):
    """aeon_avi_frame: one frame of an MJPEG AVI datum, `size` bytes at `offset` (size 0: an empty chunk)."""
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint32)]


class EncodedRecords:
    """Records marshalled once (Decoder.encoded): their aeon_encoded_elem array and the Python objects
    whose memory it points at."""

    def __init__(self, n, elems, keep):
        self.n, self.elems, self.keep = n, elems, keep

    def __len__(self):
        return self.n


BOX_BOUNDINGBOX, BOX_SSD, BOX_RCNN = 0, 1, 2
EMIT_NONE, EMIT_CENTER, EMIT_MIN_OVERLAP = 0, 1, 2


class BoxRecord(ctypes.Structure):
    """aeon_box_record: a record's boxes in the box table of an aeon_hip_box_targets_batch call."""
    _fields_ = [("first", ctypes.c_uint32), ("count", ctypes.c_int32)]


class BoxOut(ctypes.Structure):
    """aeon_box_out: target kind, sizes, emit constraint and the output buffers of a box call."""
    _fields_ = [("kind", ctypes.c_int32), ("max_boxes", ctypes.c_int32), ("out_w", ctypes.c_int32),
                ("out_h", ctypes.c_int32), ("emit_type", ctypes.c_int32), ("emit_min_overlap", ctypes.c_float),
                ("buf", ctypes.c_void_p * 5), ("item_stride", ctypes.c_uint64 * 5)]


class RcnnInfo(ctypes.Structure):
    """aeon_rcnn_info: the derived numbers of a localization_rcnn config and this build's limits."""
    _fields_ = [("total_anchors", ctypes.c_int64), ("rois_per_image", ctypes.c_int32), ("num_fg", ctypes.c_int32),
                ("max_gt_boxes", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("negative_overlap", ctypes.c_float), ("positive_overlap", ctypes.c_float),
                ("max_total_anchors", ctypes.c_int32), ("max_rois_per_image", ctypes.c_int32),
                ("max_boxes_per_record", ctypes.c_int32)]


class RcnnOut(ctypes.Structure):
    """aeon_rcnn_out: sizes, thresholds, emit constraint, anchors and the ten output buffers of an rcnn call."""
    _fields_ = [("total_anchors", ctypes.c_int32), ("max_gt_boxes", ctypes.c_int32), ("rois_per_image", ctypes.c_int32),
                ("num_fg", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("emit_type", ctypes.c_int32), ("emit_min_overlap", ctypes.c_float),
                ("negative_overlap", ctypes.c_float), ("positive_overlap", ctypes.c_float),
                ("fixed_scaling_factor", ctypes.c_float), ("anchors", ctypes.POINTER(ctypes.c_float)),
                ("anchors_key", ctypes.c_uint64), ("buf", ctypes.c_void_p * 10), ("item_stride", ctypes.c_uint64 * 10)]


class AeonHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aeon_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libaeon_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                              " (the HIP extension is required; there is no CPU fallback)")
        # One HIP runtime per process: PyTorch ships its own libamdhip64 (SONAME libamdhip64.so.7,
        # loaded by file name).  Loaded first, it also satisfies this library's dependency, so
        # torch streams/events and this library's launches share one runtime.  Loaded after this
        # library, it would bring a second runtime whose queues are not ordered with ours.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        vp = ctypes.c_void_p
        L.aeon_hip_ctx_create.argtypes = [ctypes.c_int, P(vp)]
        L.aeon_hip_ctx_destroy.argtypes = [vp]
        for fn in (L.aeon_hip_augment_batch, L.aeon_hip_mask_batch, L.aeon_hip_depthmap_batch):
            fn.argtypes = [vp, ctypes.c_int, P(ImgDesc), vp, P(AugParams), P(OutDesc), vp, vp]
        if hasattr(L, "aeon_hip_augment_pair_batch"):  # absent only in older tuning-variant builds
            L.aeon_hip_augment_pair_batch.argtypes = [vp, ctypes.c_int, P(ImgDesc), vp, P(ImgDesc), vp, P(AugParams),
                                                      P(OutDesc), vp, P(OutDesc), vp, vp]
        L.aeon_hip_synchronize.argtypes = [vp, vp]
        if hasattr(L, "aeon_hip_transpose_batch"):  # absent only in older tuning-variant builds
            L.aeon_hip_transpose_batch.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, vp]
        L.aeon_hip_set_timing.argtypes = [vp, ctypes.c_int]
        L.aeon_hip_kernel_times.argtypes = [vp, ctypes.c_int, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_long)]
        L.aeon_param_factory_create.argtypes = [ctypes.c_char_p, P(vp)]
        L.aeon_param_factory_destroy.argtypes = [vp]
        L.aeon_make_params.argtypes = [vp, P(ctypes.c_uint32), ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, P(AugParams)]
        L.aeon_make_ssd_params.argtypes = [vp, P(ctypes.c_uint32), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, P(ctypes.c_float), ctypes.c_int, P(AugParams)]
        L.aeon_batch_sample_patches.argtypes = [vp, ctypes.c_int, P(ctypes.c_uint32), P(ctypes.c_float),
                                                ctypes.c_int, P(ctypes.c_float), ctypes.c_int, P(ctypes.c_int)]
        L.aeon_param_factory_emit.argtypes = [vp, P(ctypes.c_int), P(ctypes.c_float)]
        L.aeon_box_extract.argtypes = ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 3 +
                                       [P(ctypes.c_float), P(ctypes.c_int32), P(ctypes.c_int32), ctypes.c_int,
                                        P(ctypes.c_int)])
        L.aeon_box_last_error.restype = ctypes.c_char_p
        L.aeon_hip_box_targets_batch.argtypes = [vp, ctypes.c_int, P(BoxRecord), P(ctypes.c_float), P(ctypes.c_int32),
                                                 P(ctypes.c_int32), P(AugParams), P(BoxOut), vp]
        L.aeon_rcnn_anchors.argtypes = [ctypes.c_char_p, P(ctypes.c_float), ctypes.c_int, P(ctypes.c_int)]
        L.aeon_rcnn_config_info.argtypes = [ctypes.c_char_p, P(RcnnInfo)]
        L.aeon_rcnn_sample_anchors.argtypes = [P(ctypes.c_int32), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               P(ctypes.c_uint32), P(ctypes.c_int32), P(ctypes.c_int)]
        L.aeon_rcnn_last_error.restype = ctypes.c_char_p
        L.aeon_hip_rcnn_targets_batch.argtypes = [vp, ctypes.c_int, P(BoxRecord), P(ctypes.c_float), P(ctypes.c_int32),
                                                  P(ctypes.c_int32), P(AugParams), P(ctypes.c_uint32), ctypes.c_int,
                                                  P(RcnnOut), vp]
        L.aeon_seed_slots.argtypes = [ctypes.c_uint32, ctypes.c_int, P(ctypes.c_uint32)]
        L.aeon_unbiased_round.argtypes = [ctypes.c_float, P(ctypes.c_int64)]
        L.aeon_calculate_scale.argtypes = [ctypes.c_int] * 4 + [P(ctypes.c_float)]
        L.aeon_cropbox_max_proportional.argtypes = [ctypes.c_float] * 4 + [P(ctypes.c_float)] * 2
        L.aeon_jpeg_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 3
        L.aeon_jpeg_entropy_decode.argtypes = ([ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 3 +
                                               [P(ctypes.c_int64)] * 2 + [P(ctypes.c_uint64)])
        L.aeon_jpeg_host_stage.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_int), P(ctypes.c_int64)]
        L.aeon_jpeg_huff_layout.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_int32),
                                            P(ctypes.c_int32), ctypes.c_int]
        L.aeon_hip_jpeg_huff_stage_cap.argtypes = [ctypes.c_int, P(ctypes.c_int)]
        L.aeon_hip_jpeg_huff_lanes.argtypes = [vp, P(ctypes.c_int)]
        L.aeon_png_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 4
        L.aeon_decode_png.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t,
                                      P(ctypes.c_int)]
        L.aeon_hip_decode_jpeg_batch.argtypes = [vp, ctypes.c_int, P(vp), P(ctypes.c_size_t), P(ImgDesc), vp, vp]
        L.aeon_hip_decode_png_batch.argtypes = [vp, ctypes.c_int, P(vp), P(ctypes.c_size_t), P(ctypes.c_int), P(ImgDesc),
                                                vp, vp]
        L.aeon_png_host_stage.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int64)]
        L.aeon_png_decoder_route.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_int)]
        L.aeon_png_gpu_emulate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t]
        L.aeon_pixmap_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 5
        L.aeon_decode_pixmap.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t,
                                         P(ctypes.c_int)]
        L.aeon_hip_decode_pixmap_batch.argtypes = [vp, ctypes.c_int, P(vp), P(ctypes.c_size_t), P(ctypes.c_int), P(ImgDesc),
                                                   vp, vp]
        L.aeon_pixmap_host_stage.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_int),
                                             P(ctypes.c_int64)]
        L.aeon_pixmap_gpu_emulate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t]
        L.aeon_tiff_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t] + [P(ctypes.c_int)] * 4
        L.aeon_decode_tiff.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t, P(ctypes.c_int)]
        L.aeon_hip_decode_tiff_batch.argtypes = [vp, ctypes.c_int, P(vp), P(ctypes.c_size_t), P(ctypes.c_int), P(ImgDesc),
                                                 vp, vp]
        L.aeon_tiff_host_stage.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_int),
                                           P(ctypes.c_int64)]
        L.aeon_tiff_decoder_route.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_int)]
        L.aeon_tiff_gpu_emulate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t]
        L.aeon_avi_frames.argtypes =[ctypes.c_char_p, ctypes.c_size_t, P(AviFrame), ctypes.c_int] + [P(ctypes.c_int)] * 3
        L.aeon_avi_last_error.restype = ctypes.c_char_p
        L.aeon_hip_video_batch.argtypes = [vp, ctypes.c_int, P(ctypes.c_int32), P(ImgDesc), vp, P(AugParams), ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint64, vp]
        L.aeon_hip_stager_create.argtypes = [vp, ctypes.c_int, P(OutDesc), ctypes.c_int, P(vp)]
        L.aeon_hip_stager_destroy.argtypes = [vp]
        L.aeon_hip_stager_stage.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, P(AugParams)]
        L.aeon_hip_stager_flush.argtypes = [vp, vp]
        L.aeon_hip_stager_launch.argtypes = [vp, vp]
        L.aeon_hip_stager_wait.argtypes = [vp, vp]
        L.aeon_hip_stager_last_launch.argtypes = [vp, P(StagerLaunchInfo)]
        L.aeon_encoded_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int] + [P(ctypes.c_int)] * 6
        L.aeon_hip_stager_stage_encoded.argtypes = [vp, vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, P(AugParams)]
        L.aeon_hip_stager_last_decode.argtypes = [vp, P(StagerDecodeInfo)]
        L.aeon_hip_stager_create_video.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                                   ctypes.c_int, P(vp)]
        L.aeon_clip_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int] + [P(ctypes.c_int)] * 3
        L.aeon_hip_stager_stage_clip.argtypes = [vp, vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, P(AugParams)]
        L.aeon_hip_stager_stage_frames.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, P(vp), ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, P(AugParams)]
        L.aeon_hip_release_stream.argtypes = [vp, vp]
        L.aeon_hip_stager_last_error.restype = ctypes.c_char_p
        L.aeon_hip_host_alloc.argtypes = [ctypes.c_size_t, P(vp)]
        L.aeon_hip_host_free.argtypes = [vp]
        L.aeon_decoder_create.argtypes = [ctypes.c_char_p, ctypes.c_int, P(vp)]
        L.aeon_decoder_destroy.argtypes = [vp]
        L.aeon_decoder_output_count.argtypes = [vp, P(ctypes.c_int)]
        L.aeon_decoder_output_info.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                               P(ctypes.c_int64), P(ctypes.c_int), P(ctypes.c_size_t),
                                               P(ctypes.c_int)]
        L.aeon_decoder_decode.argtypes = [vp, ctypes.c_int, P(RecordElem), P(vp), ctypes.c_int, vp]
        L.aeon_decoder_decode_encoded.argtypes = [vp, ctypes.c_int, P(EncodedElem), P(vp), ctypes.c_int, vp]
        L.aeon_decoder_draw_params.argtypes = [vp, ctypes.c_int, P(RecordElem), P(AugParams), ctypes.c_int]
        L.aeon_decoder_submit.argtypes = [vp, ctypes.c_int, P(EncodedElem), P(vp), ctypes.c_int]
        L.aeon_decoder_wait.argtypes = [vp]
        L.aeon_decoder_last_error.restype = ctypes.c_char_p
        L.aeon_thread_affinity_map.argtypes = [ctypes.c_char_p, P(ctypes.c_int), ctypes.c_int, P(ctypes.c_int)]
        L.aeon_decoder_pool_size.argtypes = [vp, P(ctypes.c_int)]
        L.aeon_decoder_pool_cpus.argtypes = [vp, ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int), ctypes.c_int,
                                             P(ctypes.c_int)]
        L.aeon_manifest_node_slice.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               P(ctypes.c_int64), P(ctypes.c_int64)]
        L.aeon_hip_last_error.restype = ctypes.c_char_p
        L.aeon_hip_version.restype = ctypes.c_char_p
        L.aeon_hip_debug_uncached_blocks.argtypes = [P(ctypes.c_uint64), ctypes.c_int, P(ctypes.c_int)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise AeonHipError(rc, lib().aeon_hip_last_error().decode())
    return rc


def uncached_blocks():
    """[(lo, hi)] device address ranges of every uncached job-table block of this process (diagnostics:
    aeon_hip_debug_uncached_blocks)."""
    n = ctypes.c_int()
    _check(lib().aeon_hip_debug_uncached_blocks(None, 0, ctypes.byref(n)))
    buf = (ctypes.c_uint64 * (2 * max(n.value, 1)))()
    _check(lib().aeon_hip_debug_uncached_blocks(buf, n.value, ctypes.byref(n)))
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]


def exported_symbols():
    """Function names declared in include/aeon_hip.h."""
    import re
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(aeon_\w+)\s*\(", text, re.M)))


# ---- parameters (host) -------------------------------------------------------------------------
class ParamFactory:
    """augment::image::param_factory (aeon src/augment_image.cpp:28-230)."""

    def __init__(self, aug_config):
        text = aug_config if isinstance(aug_config, str) else json.dumps(aug_config)
        h = ctypes.c_void_p()
        _check(lib().aeon_param_factory_create(text.encode(), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.aeon_param_factory_destroy(self._h)
            self._h = None

    def make_params(self, state, in_w, in_h, out_w, out_h):
        """state: np.uint32 array of one element (minstd_rand0 state word, updated in place)."""
        p = AugParams()
        st = ctypes.c_uint32(int(state[0]))
        _check(lib().aeon_make_params(self._h, ctypes.byref(st), in_w, in_h, out_w, out_h, ctypes.byref(p)))
        state[0] = st.value
        return p

    def sample_patches(self, sampler, state, nboxes, cap=4096):
        """batch_sampler::sample_patches of batch_samplers[sampler] (aeon src/augment_image.cpp:567-586)
        over normalized boxes; returns the sampled normalized boxes."""
        st = ctypes.c_uint32(int(state[0]))
        flat = (ctypes.c_float * max(1, 4 * len(nboxes)))(*[float(v) for b in nboxes for v in b])
        out = (ctypes.c_float * (4 * cap))()
        n = ctypes.c_int()
        _check(lib().aeon_batch_sample_patches(self._h, sampler, ctypes.byref(st), flat, len(nboxes), out, cap,
                                               ctypes.byref(n)))
        state[0] = st.value
        return [tuple(out[4 * i:4 * i + 4]) for i in range(min(n.value, cap))]

    def make_ssd_params(self, state, in_w, in_h, out_w, out_h, boxes=()):
        """param_factory::make_ssd_params (aeon src/augment_image.cpp:232-310); boxes are
        boundingbox::box pixel coordinates (xmin, ymin, xmax, ymax), xmax/ymax inclusive."""
        p = AugParams()
        st = ctypes.c_uint32(int(state[0]))
        flat = (ctypes.c_float * max(1, 4 * len(boxes)))(*[float(v) for b in boxes for v in b])
        _check(lib().aeon_make_ssd_params(self._h, ctypes.byref(st), in_w, in_h, out_w, out_h, flat, len(boxes),
                                          ctypes.byref(p)))
        state[0] = st.value
        return p

    def emit(self):
        """(EMIT_* code, emit_constraint_min_overlap) of the factory (aeon_param_factory_emit): what a
        box call takes next to the params this factory draws."""
        t, m = ctypes.c_int(), ctypes.c_float()
        _check(lib().aeon_param_factory_emit(self._h, ctypes.byref(t), ctypes.byref(m)))
        return t.value, m.value


def box_extract(class_names, text):
    """boundingbox::extractor::extract (aeon src/etl_boundingbox.cpp:64-132) of one record's JSON
    metadata: {"width", "height", "depth", "boxes" (n x 4 float32: xmin, ymin, xmax, ymax), "labels",
    "difficult" (int32)}.  AeonHipError with aeon's message for malformed metadata."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    names = json.dumps(list(class_names)).encode()
    w, h, d, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cap = 64
    while True:
        boxes, labels, diff = np.zeros((cap, 4), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        rc = lib().aeon_box_extract(names, data, len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(d),
                                    boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    diff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cap, ctypes.byref(n))
        if rc != 0:
            raise AeonHipError(rc, lib().aeon_box_last_error().decode())
        if n.value <= cap:
            break
        cap = n.value
    k = n.value
    return {"width": w.value, "height": h.value, "depth": d.value, "boxes": boxes[:k].copy(),
            "labels": labels[:k].copy(), "difficult": diff[:k].copy()}


SSD_OUTPUTS = ("image_shape", "gt_boxes", "gt_box_count", "gt_class_count", "difficult_flag")


def _pack_box_call(records, params):
    """The input side of a box / rcnn targets call: records[i] = a box_extract() dict or a (boxes n x 4, labels,
    difficult) tuple, params[i] = the record's AugParams.  Returns (BoxRecord array, boxes, labels, difficult flags,
    AugParams array), the three tables contiguous over all records."""
    n = len(records)
    recs = (BoxRecord * max(n, 1))()
    bx, lb, df = [], [], []
    first = 0
    for i, r in enumerate(records):
        b, l, d = (r["boxes"], r["labels"], r["difficult"]) if isinstance(r, dict) else r
        b = np.asarray(b, np.float32).reshape(-1, 4)
        recs[i] = BoxRecord(first, len(b))
        bx.append(b), lb.append(np.asarray(l, np.int32).reshape(-1)), df.append(np.asarray(d, np.int32).reshape(-1))
        if not len(b) == len(lb[-1]) == len(df[-1]):
            raise ValueError(f"record {i}: {len(b)} boxes, {len(lb[-1])} labels, {len(df[-1])} difficult flags")
        first += len(b)
    boxes = np.ascontiguousarray(np.concatenate(bx) if bx else np.zeros((0, 4), np.float32))
    labels = np.ascontiguousarray(np.concatenate(lb) if lb else np.zeros(0, np.int32))
    diff = np.ascontiguousarray(np.concatenate(df) if df else np.zeros(0, np.int32))
    p = params if isinstance(params, ctypes.Array) else (AugParams * max(n, 1))(*params)
    if len(p) < n:
        raise ValueError(f"{len(p)} params for {n} records")
    return recs, boxes, labels, diff, p


def _into_pinned(ctx, n, strides, out_ptrs, stream, launch):
    """launch(ptrs) with one output address per stride.  With out_ptrs those, and None comes back (the call
    stays as asynchronous as launch leaves it); without, pinned device-mapped buffers of n items each, filled
    with 0xCD beforehand, read back as uint8 arrays after a synchronize and freed."""
    if out_ptrs is not None:
        launch(out_ptrs)
        return None
    own = []
    try:
        for s in strides:
            q = ctypes.c_void_p()
            _check(lib().aeon_hip_host_alloc(max(n * s, 16), ctypes.byref(q)))
            own.append(q)
            ctypes.memset(q, 0xCD, max(n * s, 16))
        launch([q.value for q in own])
        ctx.synchronize(stream)
        return [np.frombuffer(ctypes.string_at(q, n * s), np.uint8).copy() for q, s in zip(own, strides)]
    finally:
        for q in own:
            lib().aeon_hip_host_free(q)


def box_targets(ctx, records, params, kind=BOX_SSD, max_boxes=64, out_w=0, out_h=0, emit=(EMIT_NONE, 0.0),
                item_bytes=None, out_ptrs=None, stream=0):
    """aeon_hip_box_targets_batch for len(records) records: records[i] = a box_extract() dict or a
    (boxes n x 4, labels, difficult) tuple, params[i] = the AugParams of the record's image, emit = the
    factory's ParamFactory.emit().  Without out_ptrs the kernel stores into pinned device-mapped buffers
    filled with 0xCD beforehand, and the result comes back as numpy arrays: BOX_BOUNDINGBOX one float32
    array (n, item_bytes / 4) (item_bytes: aeon's max_bbox_count * 16 * sizeof(output_type), default
    float), BOX_SSD a dict of the five outputs by aeon's names.  With out_ptrs (device addresses, one per
    output) the call is left asynchronous on `stream` and returns None."""
    n = len(records)
    recs, boxes, labels, diff, p = _pack_box_call(records, params)
    if kind == BOX_SSD:
        strides = [8, max_boxes * 16, 4, max_boxes * 4, max_boxes * 4]
    else:
        strides = [item_bytes if item_bytes is not None else max_boxes * 16 * 4]
    o = BoxOut(kind=kind, max_boxes=max_boxes, out_w=out_w, out_h=out_h, emit_type=emit[0], emit_min_overlap=emit[1])
    for k, s in enumerate(strides):
        o.item_stride[k] = s

    def launch(ptrs):
        for k in range(len(strides)):
            o.buf[k] = ptrs[k]
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        _check(lib().aeon_hip_box_targets_batch(ctx._h, n, recs, boxes.ctypes.data_as(fp), labels.ctypes.data_as(ip),
                                                diff.ctypes.data_as(ip), p, ctypes.byref(o),
                                                ctypes.c_void_p(stream or 0)))

    outs = _into_pinned(ctx, n, strides, out_ptrs, stream, launch)
    if outs is None:
        return None
    if kind != BOX_SSD:
        return outs[0].view(np.float32).reshape(n, -1)
    res = {"image_shape": outs[0].view(np.int32).reshape(n, 2), "gt_boxes": outs[1].view(np.float32).reshape(n, max_boxes, 4),
           "gt_box_count": outs[2].view(np.int32).reshape(n), "gt_class_count": outs[3].view(np.int32).reshape(n, max_boxes),
           "difficult_flag": outs[4].view(np.int32).reshape(n, max_boxes)}
    return res


# ---- localization_rcnn ---------------------------------------------------------------------------
RCNN_OUTPUTS = ("bbtargets", "bbtargets_mask", "labels_flat", "labels_mask", "image_shape", "gt_boxes",
                "gt_box_count", "gt_class_count", "image_scale", "difficult_flag")


def _check_rcnn(rc):
    if rc != 0:
        raise AeonHipError(rc, lib().aeon_rcnn_last_error().decode())


def _rcnn_text(config):
    return (config if isinstance(config, str) else json.dumps(config)).encode()


def rcnn_config_info(config):
    """localization::rcnn::config of an ETL object (dict or JSON text): total_anchors, rois_per_image,
    num_fg, max_gt_boxes, the thresholds, and this build's limits, as a dict (aeon_rcnn_config_info).
    AeonHipError for a missing or unknown key or a fraction outside [0, 1]."""
    info = RcnnInfo()
    _check_rcnn(lib().aeon_rcnn_config_info(_rcnn_text(config), ctypes.byref(info)))
    return {k: getattr(info, k) for k, _ in RcnnInfo._fields_}


def rcnn_anchors(config):
    """anchor::generate (aeon src/etl_localization_rcnn.cpp:430-469): (total_anchors, 4) float32, base
    anchors outermost, then shift rows, then shift columns."""
    n = ctypes.c_int()
    text = _rcnn_text(config)
    _check_rcnn(lib().aeon_rcnn_anchors(text, None, 0, ctypes.byref(n)))
    out = np.zeros((n.value, 4), np.float32)
    _check_rcnn(lib().aeon_rcnn_anchors(text, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n.value,
                                        ctypes.byref(n)))
    return out


def rcnn_sample_anchors(labels, rois_per_image, num_fg, shuffle=True, state=None):
    """transformer::sample_anchors (aeon src/etl_localization_rcnn.cpp:222-261) with the real std::shuffle
    over std::minstd_rand0.  state: np.uint32 array of one element (the engine's state word, updated in
    place); returns the sampled anchor indices, foreground first."""
    lab = np.ascontiguousarray(labels, np.int32)
    out = np.zeros(max(int(rois_per_image), 1), np.int32)
    st = ctypes.c_uint32(int(state[0]) if state is not None else 1)
    n = ctypes.c_int()
    ip = ctypes.POINTER(ctypes.c_int32)
    _check_rcnn(lib().aeon_rcnn_sample_anchors(lab.ctypes.data_as(ip), len(lab), int(rois_per_image), int(num_fg),
                                               int(bool(shuffle)), ctypes.byref(st), out.ctypes.data_as(ip),
                                               ctypes.byref(n)))
    if state is not None:
        state[0] = st.value
    return out[:n.value].copy()


class RcnnCall:
    """The marshalled arguments of aeon_hip_rcnn_targets_batch for one window, for calls made again and
    again (tools/rcnn_window_timing.py): launch() is the C call alone."""

    def __init__(self, ctx, config, records, params, emit=(EMIT_NONE, 0.0), fixed_scaling_factor=-1.0):
        info = rcnn_config_info(config)
        self.ctx, self.info, self.anchors = ctx, info, rcnn_anchors(config)
        self.n = n = len(records)
        A, m = int(info["total_anchors"]), info["max_gt_boxes"]
        self.recs, self.boxes, self.labels, self.diff, self.params = _pack_box_call(records, params)
        self.strides = [16 * A, 16 * A, 8 * A, 8 * A, 8, 16 * m, 4, 4 * m, 4, 4 * m]
        self.shapes = [(4 * A,), (4 * A,), (1, 2 * A), (2 * A, 1), (2, 1), (m, 4), (1, 1), (m, 1), (1, 1), (m, 1)]
        self.dtypes = [np.float32, np.float32, np.int32, np.int32, np.int32, np.float32, np.int32, np.int32, np.float32,
                       np.int32]
        self.out = RcnnOut(total_anchors=A, max_gt_boxes=m, rois_per_image=info["rois_per_image"],
                           num_fg=info["num_fg"], width=info["width"], height=info["height"], emit_type=emit[0],
                           emit_min_overlap=emit[1], negative_overlap=info["negative_overlap"],
                           positive_overlap=info["positive_overlap"], fixed_scaling_factor=fixed_scaling_factor)
        self.out.anchors = self.anchors.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        for k, s in enumerate(self.strides):
            self.out.item_stride[k] = s

    def launch(self, out_ptrs, states=None, shuffle=True, stream=0):
        """states: a contiguous np.uint32 array of n engine states, updated in place (the call then
        synchronizes the stream), or None (asynchronous; shuffle must be off)."""
        for k, q in enumerate(out_ptrs):
            self.out.buf[k] = q
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        _check(lib().aeon_hip_rcnn_targets_batch(
            self.ctx._h, self.n, self.recs, self.boxes.ctypes.data_as(fp), self.labels.ctypes.data_as(ip),
            self.diff.ctypes.data_as(ip), self.params,
            states.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if states is not None else None, int(bool(shuffle)),
            ctypes.byref(self.out), ctypes.c_void_p(stream or 0)))


def rcnn_targets(ctx, config, records, params, states=None, shuffle=True, emit=(EMIT_NONE, 0.0),
                 fixed_scaling_factor=-1.0, out_ptrs=None, stream=0):
    """aeon_hip_rcnn_targets_batch for len(records) records of the localization_rcnn ETL object `config`:
    records[i] = a box_extract() dict or a (boxes n x 4, labels, difficult) tuple, params[i] = the
    AugParams of the record's image, emit = the factory's ParamFactory.emit(), fixed_scaling_factor the
    factory's.  states: np.uint32 array of one engine state per record, updated in place to the states
    after the shuffles (required with shuffle).  The kernel stores into pinned device-mapped buffers filled
    with 0xCD beforehand; returns the ten outputs by aeon's names, each (n, ...) as aeon shapes them.  With
    out_ptrs (ten device addresses) the outputs stay there and the call returns None; it is asynchronous
    on `stream` unless it hands engine states back."""
    call = RcnnCall(ctx, config, records, params, emit, fixed_scaling_factor)
    n = call.n
    st = None
    if states is not None:
        if len(states) < n:
            raise ValueError(f"{len(states)} engine states for {n} records")
        st = np.ascontiguousarray(states[:n], np.uint32).copy()
    outs = _into_pinned(ctx, n, call.strides, out_ptrs, stream, lambda ptrs: call.launch(ptrs, st, shuffle, stream))
    if st is not None:
        states[:n] = st
    if outs is None:
        return None
    return {name: a.view(dt).reshape((n,) + sh) for name, a, dt, sh in zip(RCNN_OUTPUTS, outs, call.dtypes, call.shapes)}


def seed_slots(seed, n):
    """batch_decoder deterministic-mode engine states (aeon src/batch_decoder.cpp:47-54)."""
    out = np.zeros(n, np.uint32)
    _check(lib().aeon_seed_slots(seed, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    return out


def jpeg_info(data):
    """(width, height, components) of a JPEG file (aeon_jpeg_info)."""
    w, h, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib().aeon_jpeg_info(bytes(data), len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)))
    return w.value, h.value, n.value


def jpeg_entropy_decode(data):
    """Host-only Huffman decode of a JPEG file (aeon_jpeg_entropy_decode): (width, height,
    components, blocks, non-zero values, FNV-1a hash of the sparse coefficient stream)."""
    w, h, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nb, nv, hv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64()
    _check(lib().aeon_jpeg_entropy_decode(bytes(data), len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n),
                                          ctypes.byref(nb), ctypes.byref(nv), ctypes.byref(hv)))
    return w.value, h.value, n.value, nb.value, nv.value, hv.value


def jpeg_host_stage(data):
    """The JPEG batch decode's host work for one file (aeon_jpeg_host_stage): (GPU entropy decoding?,
    bytes staged for the H2D)."""
    g, nb = ctypes.c_int(), ctypes.c_int64()
    _check(lib().aeon_jpeg_host_stage(bytes(data), len(data), ctypes.byref(g), ctypes.byref(nb)))
    return bool(g.value), nb.value


def jpeg_huff_layout(data, lanes):
    """How the host lays a file out for the GPU Huffman decoder at `lanes` lanes (aeon_jpeg_huff_layout): a dict
    of gpu_entropy, nseg, nsub, sub_bits, data_bytes, seg_nsub (per restart segment, file order) and the decoder's
    limits sub_min, sub_max, default_lanes, stage_max.  nsub > lanes: the strided path; else the lanes path, staged
    when data_bytes fits jpeg_huff_stage_cap(lanes)."""
    out = (ctypes.c_int32 * 10)()
    _check(lib().aeon_jpeg_huff_layout(bytes(data), len(data), lanes, out, None, 0))
    segs = (ctypes.c_int32 * max(out[1], 1))()
    _check(lib().aeon_jpeg_huff_layout(bytes(data), len(data), lanes, out, segs, out[1]))
    keys = ("gpu_entropy", "nseg", "nsub", "sub_bits", "data_bytes", "seg_max", "sub_min", "sub_max", "default_lanes",
            "stage_max")
    d = dict(zip(keys, out))
    d["gpu_entropy"] = bool(out[0])
    d["seg_nsub"] = list(segs[:out[1]])
    return d


def jpeg_huff_stage_cap(lanes):
    """The most data bytes jpeg_huff copies into LDS per file at `lanes` lanes on the current device
    (aeon_hip_jpeg_huff_stage_cap); 0 without a device."""
    n = ctypes.c_int()
    _check(lib().aeon_hip_jpeg_huff_stage_cap(lanes, ctypes.byref(n)))
    return n.value


def avi_frames(data, cap=None):
    """video::extractor's demux of one MJPEG AVI datum (aeon_avi_frames): (frames, width, height) with
    frames = [(offset, size)] of the chunks' data in index order (size 0: an empty chunk, whose frame
    repeats the previous one) and width / height from the main header.  cap: look at the first cap
    frames only (what a provider with max_frame_count = cap does).  AeonHipError for a datum the
    demux refuses."""
    data = bytes(data)
    n, w, h = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if cap is None:
        rc = lib().aeon_avi_frames(data, len(data), None, 0, ctypes.byref(n), ctypes.byref(w), ctypes.byref(h))
        if rc != 0:
            raise AeonHipError(rc, lib().aeon_avi_last_error().decode())
        cap = n.value
    buf = (AviFrame * max(cap, 1))()
    rc = lib().aeon_avi_frames(data, len(data), buf, cap, ctypes.byref(n), ctypes.byref(w), ctypes.byref(h))
    if rc != 0:
        raise AeonHipError(rc, lib().aeon_avi_last_error().decode())
    return [(buf[i].offset, buf[i].size) for i in range(min(n.value, cap))], w.value, h.value


PNG_BGR8, PNG_GRAY8, PNG_ANYDEPTH = 0, 1, 2


def clip_info(data, max_frames):
    """(kept, width, height) of an MJPEG AVI datum (aeon_clip_info): min(frame count, max_frames) and the first kept
    frame's decoded size, which is what provider::video draws the clip's params with."""
    data = bytes(data)
    k, w, h = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check_stager(lib().aeon_clip_info(data, len(data), int(max_frames), ctypes.byref(k), ctypes.byref(w), ctypes.byref(h)))
    return k.value, w.value, h.value


def png_info(data):
    """(width, height, bit depth, PNG colour type) of a PNG file (aeon_png_info)."""
    w, h, d, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib().aeon_png_info(bytes(data), len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(d),
                               ctypes.byref(c)))
    return w.value, h.value, d.value, c.value


def decode_png(data, mode=PNG_BGR8):
    """cv::imdecode of a PNG file as aeon's extractors ask for it (aeon_decode_png): HxWx3 uint8 BGR
    (PNG_BGR8), HxW uint8 (PNG_GRAY8), or HxW uint8 / uint16 at the file's depth (PNG_ANYDEPTH)."""
    w, h, d, c = png_info(data)
    wide = mode == PNG_ANYDEPTH and d == 16 and c != 3
    cn = 3 if mode == PNG_BGR8 else 1
    out = np.zeros((h, w, cn) if cn == 3 else (h, w), np.uint16 if wide else np.uint8)
    eb = ctypes.c_int()
    _check(lib().aeon_decode_png(bytes(data), len(data), mode, out.ctypes.data, out.strides[0], ctypes.byref(eb)))
    return out


def png_host_stage(data, mode=PNG_BGR8):
    """The PNG batch decode's host work for one file (aeon_png_host_stage): (does the device take the file's
    inflate?, bytes staged for the H2D)."""
    g, nb = ctypes.c_int(), ctypes.c_int64()
    _check(lib().aeon_png_host_stage(bytes(data), len(data), mode, ctypes.byref(g), ctypes.byref(nb)))
    return bool(g.value), nb.value


def png_decoder_route(data):
    """Does a Decoder send this encoded PNG element through the device stage (aeon_png_decoder_route)?"""
    g = ctypes.c_int()
    _check(lib().aeon_png_decoder_route(bytes(data), len(data), ctypes.byref(g)))
    return bool(g.value)


def png_gpu_emulate(data, mode=PNG_BGR8):
    """decode_png through the PNG stage's kernel code run on the host (aeon_png_gpu_emulate).  AeonHipError
    for a file the stage leaves to the host decoder, or one the device would report as corrupt."""
    w, h, d, c = png_info(data)
    wide = mode == PNG_ANYDEPTH and d == 16 and c != 3
    cn = 3 if mode == PNG_BGR8 else 1
    out = np.zeros((h, w, cn) if cn == 3 else (h, w), np.uint16 if wide else np.uint8)
    _check(lib().aeon_png_gpu_emulate(bytes(data), len(data), mode, out.ctypes.data, out.strides[0]))
    return out


DECODE_BGR8, DECODE_GRAY8, DECODE_ANYDEPTH = PNG_BGR8, PNG_GRAY8, PNG_ANYDEPTH
PIXMAP_BMP = 0  # pixmap_info's format of a BMP file; a PNM file's is its magic digit (1..6)


def pixmap_info(data):
    """(width, height, decoded bits per sample, the file's channels, format) of a BMP or PNM file
    (aeon_pixmap_info); format is PIXMAP_BMP or the PNM magic's digit."""
    v = [ctypes.c_int() for _ in range(5)]
    _check(lib().aeon_pixmap_info(bytes(data), len(data), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _pixmap_out(data, mode):
    w, h, d, _, _ = pixmap_info(data)
    cn = 3 if mode == DECODE_BGR8 else 1
    return np.zeros((h, w, cn) if cn == 3 else (h, w), np.uint16 if (mode == DECODE_ANYDEPTH and d == 16) else np.uint8)


def decode_pixmap(data, mode=DECODE_BGR8):
    """cv::imdecode of a BMP or PNM file as aeon's extractors ask for it (aeon_decode_pixmap): HxWx3 uint8 BGR
    (DECODE_BGR8), HxW uint8 (DECODE_GRAY8), or HxW uint8 / uint16 (a PNM with maxval > 255) (DECODE_ANYDEPTH)."""
    out = _pixmap_out(data, mode)
    eb = ctypes.c_int()
    _check(lib().aeon_decode_pixmap(bytes(data), len(data), mode, out.ctypes.data, out.strides[0], ctypes.byref(eb)))
    return out


def pixmap_host_stage(data, mode=DECODE_BGR8):
    """The pixmap batch decode's host work for one file (aeon_pixmap_host_stage): (does the device convert the
    file?, bytes staged for the H2D)."""
    g, nb = ctypes.c_int(), ctypes.c_int64()
    _check(lib().aeon_pixmap_host_stage(bytes(data), len(data), mode, ctypes.byref(g), ctypes.byref(nb)))
    return bool(g.value), nb.value


def pixmap_gpu_emulate(data, mode=DECODE_BGR8):
    """decode_pixmap through the pixmap stage's kernel code run on the host (aeon_pixmap_gpu_emulate).
    AeonHipError for a file the stage leaves to the host decoder (ASCII PNM)."""
    out = _pixmap_out(data, mode)
    _check(lib().aeon_pixmap_gpu_emulate(bytes(data), len(data), mode, out.ctypes.data, out.strides[0]))
    return out


def tiff_info(data):
    """(width, height, the file's channels, the element bytes DECODE_ANYDEPTH gives) of a TIFF file (aeon_tiff_info)."""
    v = [ctypes.c_int() for _ in range(4)]
    _check(lib().aeon_tiff_info(bytes(data), len(data), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _tiff_out(data, mode):
    w, h, _, eb = tiff_info(data)
    cn = 3 if mode == DECODE_BGR8 else 1
    return np.zeros((h, w, cn) if cn == 3 else (h, w), np.uint16 if (mode == DECODE_ANYDEPTH and eb == 2) else np.uint8)


def decode_tiff(data, mode=DECODE_BGR8):
    """cv::imdecode of a TIFF file as aeon's extractors ask for it (aeon_decode_tiff): HxWx3 uint8 BGR (DECODE_BGR8),
    HxW uint8 (DECODE_GRAY8), or HxW uint8 / uint16 (a 16-bit gray file) (DECODE_ANYDEPTH)."""
    out = _tiff_out(data, mode)
    eb = ctypes.c_int()
    _check(lib().aeon_decode_tiff(bytes(data), len(data), mode, out.ctypes.data, out.strides[0], ctypes.byref(eb)))
    return out


def tiff_host_stage(data, mode=DECODE_BGR8):
    """The TIFF batch decode's host work for one file (aeon_tiff_host_stage): (does the device decode the file?,
    bytes staged for the H2D)."""
    g, nb = ctypes.c_int(), ctypes.c_int64()
    _check(lib().aeon_tiff_host_stage(bytes(data), len(data), mode, ctypes.byref(g), ctypes.byref(nb)))
    return bool(g.value), nb.value


def tiff_decoder_route(data):
    """Does the decoder send this TIFF file through the stage (aeon_tiff_decoder_route)?"""
    g = ctypes.c_int()
    _check(lib().aeon_tiff_decoder_route(bytes(data), len(data), ctypes.byref(g)))
    return bool(g.value)


def tiff_gpu_emulate(data, mode=DECODE_BGR8, out=None):
    """decode_tiff through the TIFF stage's kernel code run on the host (aeon_tiff_gpu_emulate), into `out` (a
    2-D uint8 view with any row stride) if given.  AeonHipError for a file the stage leaves to the host decoder
    or one the device would report as corrupt."""
    if out is None:
        out = _tiff_out(data, mode)
    _check(lib().aeon_tiff_gpu_emulate(bytes(data), len(data), mode, out.ctypes.data, out.strides[0]))
    return out


FORMAT_JPEG, FORMAT_PNG, FORMAT_PIXMAP, FORMAT_TIFF = 0, 1, 2, 3
FORMAT_NAMES = ("jpeg", "png", "pixmap", "tiff")


def encoded_info(data, mask=False):
    """What a Decoder finds out about an encoded element before it decodes it (aeon_encoded_info): a dict of
    format (FORMAT_*), width, height, file_channels, elem_bytes (2: a mask that decodes to uint16) and
    device_route (does the decoder's routing rule send the file through its device stage?).  mask: the file
    is a pixel mask (ANYDEPTH), for which a JPEG file is refused."""
    v = [ctypes.c_int() for _ in range(6)]
    _check(lib().aeon_encoded_info(bytes(data), len(data), 1 if mask else 0, *[ctypes.byref(x) for x in v]))
    keys = ("format", "width", "height", "file_channels", "elem_bytes", "device_route")
    d = {k: x.value for k, x in zip(keys, v)}
    d["device_route"] = bool(d["device_route"])
    return d


def unbiased_round(x):
    """nervana::unbiased_round (aeon src/util.cpp:212-239)."""
    r = ctypes.c_int64()
    _check(lib().aeon_unbiased_round(x, ctypes.byref(r)))
    return r.value


def calculate_scale(w, h, out_w, out_h):
    """image::calculate_scale (aeon src/image.cpp:214-224)."""
    s = ctypes.c_float()
    _check(lib().aeon_calculate_scale(w, h, out_w, out_h, ctypes.byref(s)))
    return s.value


def cropbox_max_proportional(in_w, in_h, out_w, out_h):
    """image::cropbox_max_proportional (aeon src/image.cpp:226-237) -> (width, height)."""
    rw, rh = ctypes.c_float(), ctypes.c_float()
    _check(lib().aeon_cropbox_max_proportional(in_w, in_h, out_w, out_h, ctypes.byref(rw), ctypes.byref(rh)))
    return rw.value, rh.value


def aug_params(**kw):
    p = AugParams(contrast=1.0, brightness=1.0, saturation=1.0, interp=INTERP_LINEAR)
    for k, v in kw.items():
        if k == "lighting":
            p.n_lighting = len(v)
            for i, x in enumerate(v):
                p.lighting[i] = x
        else:
            setattr(p, k, v)
    return p


def out_desc(channels=3, channel_major=True, bgr_to_rgb=False, dtype="float32", mean=None,
             stddev=None, item_stride=0, fixed_aspect_ratio=False, canvas=(0, 0)):
    o = OutDesc(dtype=DTYPES[dtype][0], channels=channels,
                channel_major=int(channel_major), bgr_to_rgb=int(bgr_to_rgb), has_mean=0,
                item_stride=item_stride, fixed_aspect_ratio=int(fixed_aspect_ratio),
                canvas_w=canvas[0], canvas_h=canvas[1])
    if mean is not None:
        o.has_mean = 1
        for i in range(channels):
            o.mean[i] = mean[i]
            o.stddev[i] = stddev[i]
    return o


# ---- device stage --------------------------------------------------------------------------------
class JpegFiles:
    """Encoded files marshalled once for aeon_hip_decode_jpeg_batch (the pointer and size arrays; the
    bytes objects are kept alive here)."""

    def __init__(self, files):
        self.bufs = [bytes(f) for f in files]
        n = len(self.bufs)
        self.ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in self.bufs])
        self.sizes = (ctypes.c_size_t * n)(*[len(b) for b in self.bufs])

    def __len__(self):
        return len(self.bufs)


class Context:
    """One per GPU (aeon_hip_ctx)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        _check(lib().aeon_hip_ctx_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _check(lib().aeon_hip_ctx_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch(self, fn, descs, src_ptr, params, out, out_ptr, stream):
        n = len(descs)
        # prebuilt ctypes arrays pass straight through (the C++ host fills these in place)
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        p = params if isinstance(params, ctypes.Array) else (AugParams * n)(*params)
        if len(p) < n:
            raise ValueError(f"{len(p)} params for {n} records")
        _check(fn(self._h, n, d, ctypes.c_void_p(src_ptr), p, ctypes.byref(out),
                  ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)))

    def augment_batch(self, descs, src_ptr, params, out, out_ptr, stream=0):
        """transform_single_image + loader::load for len(descs) records (async on stream)."""
        self._batch(lib().aeon_hip_augment_batch, descs, src_ptr, params, out, out_ptr, stream)

    def mask_batch(self, descs, src_ptr, params, out, out_ptr, stream=0):
        """pixel_mask transform + load for len(descs) records (async on stream)."""
        self._batch(lib().aeon_hip_mask_batch, descs, src_ptr, params, out, out_ptr, stream)

    def pair_batch(self, descs, src_ptr, mask_descs, mask_src_ptr, params, out, out_ptr, mask_out, mask_out_ptr,
                   stream=0):
        """provider::image + provider::pixelmask of the same records, one params set per record
        (aeon_hip_augment_pair_batch: for 8-bit unrotated masks into uint8 items one job table and two
        launches -- the image tiles, then the masks' gather; AEON_HIP_FUSE_MASKS=1: one launch)."""
        n = len(descs)
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        md = mask_descs if isinstance(mask_descs, ctypes.Array) else (ImgDesc * n)(*mask_descs)
        p = params if isinstance(params, ctypes.Array) else (AugParams * n)(*params)
        if len(md) < n or len(p) < n:
            raise ValueError(f"{len(md)} masks / {len(p)} params for {n} records")
        _check(lib().aeon_hip_augment_pair_batch(self._h, n, d, ctypes.c_void_p(src_ptr), md, ctypes.c_void_p(mask_src_ptr),
                                                 p, ctypes.byref(out), ctypes.c_void_p(out_ptr), ctypes.byref(mask_out),
                                                 ctypes.c_void_p(mask_out_ptr), ctypes.c_void_p(stream or 0)))

    def depthmap_batch(self, descs, src_ptr, params, out, out_ptr, stream=0):
        """depthmap transform + load (aeon src/etl_depthmap.cpp) for len(descs) records."""
        self._batch(lib().aeon_hip_depthmap_batch, descs, src_ptr, params, out, out_ptr, stream)

    def video_batch(self, frame_counts, descs, src_ptr, params, max_frames, out_w, out_h, out_ptr, item_stride,
                    stream=0):
        """video::transformer + video::loader for len(frame_counts) clips (aeon_hip_video_batch, async on
        stream): frame_counts = a list, or a prebuilt c_int32 array; descs = max_frames descriptors per clip,
        row-major (a list, or a prebuilt ImgDesc array),
        of which clip i's first frame_counts[i] are read; params[i] = clip i's AugParams.  Clip i is
        written at out_ptr + i * item_stride as uint8 (3, max_frames, out_h, out_w), B, G, R planes, its
        frames past frame_counts[i] zero."""
        n = len(frame_counts)
        fc = frame_counts if isinstance(frame_counts, ctypes.Array) else (ctypes.c_int32 * max(n, 1))(*[int(c) for c in frame_counts])
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * max(len(descs), 1))(*descs)
        p = params if isinstance(params, ctypes.Array) else (AugParams * max(n, 1))(*params)
        if len(d) < n * max_frames or len(p) < n:
            raise ValueError(f"{len(d)} frame descriptors / {len(p)} params for {n} clips of {max_frames} frames")
        _check(lib().aeon_hip_video_batch(self._h, n, fc, d, ctypes.c_void_p(src_ptr), p, int(max_frames), int(out_w),
                                          int(out_h), ctypes.c_void_p(out_ptr), int(item_stride),
                                          ctypes.c_void_p(stream or 0)))

    def decode_jpeg_batch(self, files, descs, dst_ptr, stream=0):
        """image::extractor::extract of JPEG files into device memory (aeon_hip_decode_jpeg_batch):
        files = list of bytes (or a JpegFiles, marshalled once), descs[i] = where record i goes (HWC,
        channels 3 = BGR / 1 = gray)."""
        jf = files if isinstance(files, JpegFiles) else JpegFiles(files)
        n, ptrs, sizes = len(jf), jf.ptrs, jf.sizes
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        _check(lib().aeon_hip_decode_jpeg_batch(self._h, n, ptrs, sizes, d, ctypes.c_void_p(dst_ptr),
                                                ctypes.c_void_p(stream or 0)))

    def jpeg_huff_lanes(self):
        """The workgroup size this context's GPU Huffman decoder runs (aeon_hip_jpeg_huff_lanes)."""
        n = ctypes.c_int()
        _check(lib().aeon_hip_jpeg_huff_lanes(self._h, ctypes.byref(n)))
        return n.value

    def decode_png_batch(self, files, modes, descs, dst_ptr, stream=0):
        """decode_png of PNG files into device memory (aeon_hip_decode_png_batch): files = list of bytes (or
        a JpegFiles, marshalled once), modes[i] = PNG_BGR8 / PNG_GRAY8 / PNG_ANYDEPTH, descs[i] = where
        record i goes (HWC; ANYDEPTH of a 16-bit file: native uint16)."""
        jf = files if isinstance(files, JpegFiles) else JpegFiles(files)
        n, ptrs, sizes = len(jf), jf.ptrs, jf.sizes
        m = modes if isinstance(modes, ctypes.Array) else (ctypes.c_int * n)(*[int(x) for x in modes])
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        if len(m) < n or len(d) < n:
            raise ValueError(f"{len(m)} modes / {len(d)} descriptors for {n} files")
        _check(lib().aeon_hip_decode_png_batch(self._h, n, ptrs, sizes, m, d, ctypes.c_void_p(dst_ptr),
                                               ctypes.c_void_p(stream or 0)))

    def decode_pixmap_batch(self, files, modes, descs, dst_ptr, stream=0):
        """decode_pixmap of BMP / PNM files into device memory (aeon_hip_decode_pixmap_batch): files = list of
        bytes (or a JpegFiles, marshalled once), modes[i] = DECODE_BGR8 / DECODE_GRAY8 / DECODE_ANYDEPTH,
        descs[i] = where record i goes (HWC; ANYDEPTH of a 16-bit PNM: native uint16)."""
        jf = files if isinstance(files, JpegFiles) else JpegFiles(files)
        n, ptrs, sizes = len(jf), jf.ptrs, jf.sizes
        m = modes if isinstance(modes, ctypes.Array) else (ctypes.c_int * n)(*[int(x) for x in modes])
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        if len(m) < n or len(d) < n:
            raise ValueError(f"{len(m)} modes / {len(d)} descriptors for {n} files")
        _check(lib().aeon_hip_decode_pixmap_batch(self._h, n, ptrs, sizes, m, d, ctypes.c_void_p(dst_ptr),
                                                  ctypes.c_void_p(stream or 0)))

    def decode_tiff_batch(self, files, modes, descs, dst_ptr, stream=0):
        """decode_tiff of TIFF files into device memory (aeon_hip_decode_tiff_batch): files = list of bytes (or a
        JpegFiles, marshalled once), modes[i] = DECODE_BGR8 / DECODE_GRAY8 / DECODE_ANYDEPTH, descs[i] = where
        record i goes (HWC; ANYDEPTH of a 16-bit gray file: native uint16)."""
        jf = files if isinstance(files, JpegFiles) else JpegFiles(files)
        n, ptrs, sizes = len(jf), jf.ptrs, jf.sizes
        m = modes if isinstance(modes, ctypes.Array) else (ctypes.c_int * n)(*[int(x) for x in modes])
        d = descs if isinstance(descs, ctypes.Array) else (ImgDesc * n)(*descs)
        if len(m) < n or len(d) < n:
            raise ValueError(f"{len(m)} modes / {len(d)} descriptors for {n} files")
        _check(lib().aeon_hip_decode_tiff_batch(self._h, n, ptrs, sizes, m, d, ctypes.c_void_p(dst_ptr),
                                                ctypes.c_void_p(stream or 0)))

    def set_timing(self, every=1):
        """Time the launches of one call in `every` (0 = off) with HIP events on their stream."""
        _check(lib().aeon_hip_set_timing(self._h, int(every)))

    def kernel_times(self):
        """{'augment'|'stats'|'pre'|'jpeg'|'png': (total_ms, total_algorithmic_bytes, launches)}"""
        ms, by, ct = (ctypes.c_double * 5)(), (ctypes.c_double * 5)(), (ctypes.c_long * 5)()
        _check(lib().aeon_hip_kernel_times(self._h, 5, ms, by, ct))
        return {k: (ms[i], by[i], ct[i]) for i, k in enumerate(("augment", "stats", "pre", "jpeg", "png"))}

    def synchronize(self, stream=0):
        _check(lib().aeon_hip_synchronize(self._h, ctypes.c_void_p(stream or 0)))

    def release_stream(self, stream):
        """The caller is about to destroy `stream` (aeon_hip_release_stream)."""
        _check(lib().aeon_hip_release_stream(self._h, ctypes.c_void_p(stream or 0)))

    def transpose_batch(self, src_ptr, dst_ptr, rows, cols, element_size, stream=0):
        """batch_major=false layout: dst[c*rows + r] = src[r*cols + c] (async on stream)."""
        _check(lib().aeon_hip_transpose_batch(self._h, ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr),
                                              rows, cols, element_size, ctypes.c_void_p(stream or 0)))


STAGER_IMAGE, STAGER_MASK, STAGER_VIDEO, STAGER_DEVICE_OUT = 0, 1, 2, 0x100


class StagerLaunchInfo(ctypes.Structure):  # aeon_stager_launch_info
    _fields_ = [("launches", ctypes.c_uint64), ("src_zero_copy", ctypes.c_int32), ("out_direct", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("records", ctypes.c_int32)]


class StagerDecodeInfo(ctypes.Structure):  # aeon_stager_decode_info
    _fields_ = [("launches", ctypes.c_uint64), ("device", ctypes.c_int32 * 4), ("host", ctypes.c_int32 * 4),
                ("pixels", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _check_stager(rc):
    if rc != 0:
        raise AeonHipError(rc, lib().aeon_hip_stager_last_error().decode())
    return rc


class Stager:
    """aeon_hip_stager: what the aeon-side provider::image / ::pixelmask hold.
    stage() from provide() on any pool thread (the ctypes call releases the GIL); launch() from
    post_process() once per batch (the first launch of a window launches the whole window and
    returns), wait() from the consumer before it reads a batch (wait_buffer(): by buffer alone, as
    batch_iterator_fbm::filler calls it); flush() = launch + wait."""

    def __init__(self, ctx, out, batch_size, kind=STAGER_IMAGE):
        h = ctypes.c_void_p()
        self._out = out
        _check_stager(lib().aeon_hip_stager_create(ctx._h, kind, ctypes.byref(out), batch_size, ctypes.byref(h)))
        self._h = h

    def stage(self, batch_out, idx, pixels, params):
        """pixels: HxWxC or HxW uint8 / uint16 array (host)."""
        a = np.ascontiguousarray(pixels)
        h, w = a.shape[:2]
        cn = 1 if a.ndim == 2 else a.shape[2]
        _check_stager(lib().aeon_hip_stager_stage(self._h, ctypes.c_void_p(batch_out), idx, a.ctypes.data, w, h,
                                                   a.strides[0], cn, a.itemsize, ctypes.byref(params)))

    def stage_encoded(self, batch_out, idx, data, params):
        """data: the record's file (JPEG, PNG, BMP / PNM, TIFF) as bytes; decoded by the stager, on the device where
        the decoder's routing rule says so, else on the calling thread (aeon_hip_stager_stage_encoded)."""
        data = bytes(data)
        _check_stager(lib().aeon_hip_stager_stage_encoded(self._h, ctypes.c_void_p(batch_out), idx, data, len(data),
                                                          ctypes.byref(params)))

    @classmethod
    def video(cls, ctx, max_frames, out_w, out_h, item_stride, batch_size, device_out=False):
        """What the aeon-side provider::video holds (aeon_hip_stager_create_video): an item of a batch buffer is one
        clip, uint8 (3, max_frames, out_h, out_w), item_stride bytes apart; stage_clip() / stage_frames() from
        provide(), the rest as for images."""
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        self._out = None
        _check_stager(lib().aeon_hip_stager_create_video(ctx._h, STAGER_DEVICE_OUT if device_out else 0, max_frames, out_w,
                                                         out_h, item_stride, batch_size, ctypes.byref(h)))
        self._h = h
        return self

    def stage_clip(self, batch_out, idx, data, params):
        """data: the record's MJPEG AVI datum as bytes; its first max_frames frames are decoded by the window's launch
        (aeon_hip_stager_stage_clip)."""
        data = bytes(data)
        _check_stager(lib().aeon_hip_stager_stage_clip(self._h, ctypes.c_void_p(batch_out), idx, data, len(data),
                                                       ctypes.byref(params)))

    def stage_frames(self, batch_out, idx, frames, params):
        """frames: the clip's decoded frames, HxWx3 uint8 arrays of one size; None after the first repeats the frame
        before it (aeon_hip_stager_stage_frames)."""
        arrays = [None if f is None else np.ascontiguousarray(f) for f in frames]
        first = arrays[0] if arrays and arrays[0] is not None else np.zeros((0, 0, 3), np.uint8)
        if any(a is not None and (a.shape != first.shape or a.dtype != np.uint8) for a in arrays) or first.ndim != 3:
            raise ValueError("the frames of a clip are HxWx3 uint8 arrays of one size")
        ptrs = (ctypes.c_void_p * max(len(arrays), 1))(*[None if a is None else a.ctypes.data for a in arrays])
        h, w = first.shape[:2]
        _check_stager(lib().aeon_hip_stager_stage_frames(self._h, ctypes.c_void_p(batch_out), idx, len(arrays), ptrs, w, h,
                                                         w * 3, ctypes.byref(params)))

    def flush(self, batch_out):
        _check_stager(lib().aeon_hip_stager_flush(self._h, ctypes.c_void_p(batch_out)))

    def launch(self, batch_out):
        _check_stager(lib().aeon_hip_stager_launch(self._h, ctypes.c_void_p(batch_out)))

    def wait(self, batch_out):
        _check_stager(lib().aeon_hip_stager_wait(self._h, ctypes.c_void_p(batch_out)))

    @staticmethod
    def wait_buffer(batch_out):
        """aeon_hip_stager_wait(NULL, batch_out): whichever stager launched the buffer, if any."""
        _check_stager(lib().aeon_hip_stager_wait(None, ctypes.c_void_p(batch_out)))

    def last_launch(self):
        """The paths of the most recently launched window (aeon_hip_stager_last_launch): a dict of launches,
        src_zero_copy, out_direct, chunks, records."""
        info = StagerLaunchInfo()
        _check_stager(lib().aeon_hip_stager_last_launch(self._h, ctypes.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in StagerLaunchInfo._fields_}

    def last_decode(self):
        """Where the records of the most recently launched window were decoded (aeon_hip_stager_last_decode): a
        dict of launches, device and host ({format name: records}) and pixels (staged decoded)."""
        info = StagerDecodeInfo()
        _check_stager(lib().aeon_hip_stager_last_decode(self._h, ctypes.byref(info)))
        return {"launches": int(info.launches), "device": dict(zip(FORMAT_NAMES, info.device)),
                "host": dict(zip(FORMAT_NAMES, info.host)), "pixels": int(info.pixels)}

    def close(self):
        if getattr(self, "_h", None):
            lib().aeon_hip_stager_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_images(images, align=16):
    """Concatenate HWC uint8 images into one byte arena; returns (arena, [ImgDesc])."""
    descs, chunks, off = [], [], 0
    for im in images:
        im = np.ascontiguousarray(im, dtype=np.uint8)
        h, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else im.shape[2]
        descs.append(ImgDesc(offset=off, width=w, height=h, stride=w * cn, channels=cn))
        b = im.reshape(-1)
        pad = (-b.size) % align
        chunks.append(b)
        if pad:
            chunks.append(np.zeros(pad, np.uint8))
        off += b.size + pad
    arena = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return arena, descs


def synthetic_image(index, w, h, cn=3, seed=0x5EED):
    """Counter-based synthetic HWC uint8 image: byte = splitmix64(seed^(img<<32)^idx)&0xFF."""
    idx = np.arange(w * h * cn, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) ^ (np.uint64(index) << np.uint64(32)) ^ idx) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFF)).astype(np.uint8).reshape(h, w, cn) if cn > 1 else \
        (z & np.uint64(0xFF)).astype(np.uint8).reshape(h, w)


# ---- decode stage (provider_factory + batch_decoder, host C++) -----------------------------------
def _check_host(rc):
    if rc != 0:
        raise AeonHipError(rc, lib().aeon_decoder_last_error().decode())
    return rc


class Decoder:
    """aeon batch_decoder over provider_factory::create(config): decode windows of records (per ETL
    element an HWC uint8 array, an encoded JPEG / PNG / BMP / PNM file, or -- boundingbox, localization_ssd and
    localization_rcnn elements -- the JSON metadata as bytes or str, a video element's MJPEG AVI file as
    bytes, a label element's text or 4 binary bytes) into the provider output buffers.  A provider may own
    several output buffers (localization_ssd: five, localization_rcnn: ten), so records have n_inputs elements and windows
    len(outputs) buffers, in get_output_shapes() order."""

    def __init__(self, config, device=0):
        text = config if isinstance(config, str) else json.dumps(config)
        try:
            self.n_inputs = len(json.loads(text)["etl"])
        except (ValueError, KeyError, TypeError):
            self.n_inputs = 0  # the library reports what is wrong with the config
        h = ctypes.c_void_p()
        _check_host(lib().aeon_decoder_create(text.encode(), device, ctypes.byref(h)))
        self._h = h
        n = ctypes.c_int()
        _check_host(lib().aeon_decoder_output_count(self._h, ctypes.byref(n)))
        self.outputs = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(256)
            shape = (ctypes.c_int64 * 8)()
            nd, ib, dt = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int()
            _check_host(lib().aeon_decoder_output_info(self._h, i, name, 256, shape, ctypes.byref(nd),
                                                       ctypes.byref(ib), ctypes.byref(dt)))
            self.outputs.append({"name": name.value.decode(), "shape": tuple(shape[:nd.value]),
                                 "item_bytes": ib.value,
                                 "dtype": NP_DTYPE.get(dt.value),
                                 "type_name": TYPE_NAME.get(dt.value)})

    def close(self):
        if getattr(self, "_h", None):
            lib().aeon_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encoded(self, records):
        """The records marshalled once into their aeon_encoded_elem array (EncodedRecords), for windows
        submitted again and again: aeon's host hands the decoder plain pointers, so a benchmark that
        rebuilds ctypes structures per record per window (~2-5 us each) would time Python instead."""
        elems, keep = self._encoded(records)
        return EncodedRecords(len(records), elems, keep)

    def _encoded(self, records):
        """aeon_encoded_elem array for records whose elements are JPEG bytes or HWC uint8 arrays."""
        if isinstance(records, EncodedRecords):
            return records.elems, records.keep
        n, ne = len(records), self.n_inputs
        keep = []
        elems = (EncodedElem * (n * ne))()
        for i, rec in enumerate(records):
            for k in range(ne):
                x = rec[k]
                if isinstance(x, str):
                    x = x.encode()
                if isinstance(x, (bytes, bytearray, memoryview)):
                    b = bytes(x)
                    keep.append(b)
                    elems[i * ne + k] = EncodedElem(ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p), len(b), 0, 0, 0, 0)
                else:
                    a = np.ascontiguousarray(x, dtype=np.uint8)
                    keep.append(a)
                    h, w = a.shape[:2]
                    cn = 1 if a.ndim == 2 else a.shape[2]
                    elems[i * ne + k] = EncodedElem(a.ctypes.data, a.nbytes, w, h, cn, w * cn)
        return elems, keep

    def decode(self, records, stream=0):
        """records: list of tuples, one element per ETL provider: HWC uint8 arrays or encoded JPEG
        bytes.  Returns one numpy array per output buffer, shape (n,) + item shape."""
        n = len(records)
        ne = self.n_inputs
        outs = [np.zeros((n,) + o["shape"], o["dtype"]) for o in self.outputs]
        ptrs = (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        if any(isinstance(x, (str, bytes, bytearray, memoryview)) for rec in records for x in rec):
            elems, keep = self._encoded(records)
            _check_host(lib().aeon_decoder_decode_encoded(self._h, n, elems, ptrs, 0, ctypes.c_void_p(stream or 0)))
            return outs
        keep = []
        elems = (RecordElem * (n * ne))()
        for i, rec in enumerate(records):
            for k in range(ne):
                a = np.ascontiguousarray(rec[k], dtype=np.uint8)
                keep.append(a)
                h, w = a.shape[:2]
                cn = 1 if a.ndim == 2 else a.shape[2]
                elems[i * ne + k] = RecordElem(a.ctypes.data, w, h, cn, w * cn)
        _check_host(lib().aeon_decoder_decode(self._h, n, elems, ptrs, 0, ctypes.c_void_p(stream or 0)))
        return outs

    def decode_named(self, records, stream=0):
        """decode() with the outputs by buffer name (aeon's fixed_buffer_map keys)."""
        return {o["name"]: a for o, a in zip(self.outputs, self.decode(records, stream))}

    def draw_params(self, sizes, serial=False):
        """The draw phase of one window alone (aeon_decoder_draw_params, host only): sizes = one
        (width, height) per record (of its first element; the others get the same size); returns
        the records' AugParams.  The slot engines advance as in a real window."""
        n, ne = len(sizes), self.n_inputs
        elems = (RecordElem * (n * ne))()
        dummy = ctypes.c_uint8(0)
        for i, (w, h) in enumerate(sizes):
            for k in range(ne):
                elems[i * ne + k] = RecordElem(ctypes.addressof(dummy), w, h, 3, w * 3)
        out = (AugParams * max(n, 1))()
        _check_host(lib().aeon_decoder_draw_params(self._h, n, elems, out, int(serial)))
        return list(out[:n])

    def submit(self, records, output_ptrs, on_device=False):
        """Double-buffered window (aeon_decoder_submit): output_ptrs[k] = address of n items of
        output k (pinned host memory, or device memory with on_device); complete after wait().
        records: a list of tuples, or an EncodedRecords from encoded() (kept alive by the caller
        until the window's wait())."""
        n = len(records)
        elems, keep = self._encoded(records)
        ptrs = (ctypes.c_void_p * len(self.outputs))(*output_ptrs)
        _check_host(lib().aeon_decoder_submit(self._h, n, elems, ptrs, int(on_device)))

    def wait(self):
        _check_host(lib().aeon_decoder_wait(self._h))

    def pool_cpus(self):
        """Per decode-pool worker: (CPU of the affinity map it was pinned to or -1, the CPUs its own
        sched_getaffinity reported after pinning)."""
        n = ctypes.c_int()
        _check_host(lib().aeon_decoder_pool_size(self._h, ctypes.byref(n)))
        res = []
        for w in range(n.value):
            mc, cnt = ctypes.c_int(), ctypes.c_int()
            buf = (ctypes.c_int * 4096)()
            _check_host(lib().aeon_decoder_pool_cpus(self._h, w, ctypes.byref(mc), buf, 4096, ctypes.byref(cnt)))
            res.append((mc.value, list(buf[:min(cnt.value, 4096)])))
        return res


def thread_affinity_map(cpu_list=""):
    """nervana::get_thread_affinity_map (aeon src/util.cpp:337-373): the CPUs the decode pool's
    workers are pinned to (AEON_CPU_LIST, else cpu_list, else the default policy)."""
    cnt = ctypes.c_int()
    buf = (ctypes.c_int * 4096)()
    _check_host(lib().aeon_thread_affinity_map(cpu_list.encode(), buf, 4096, ctypes.byref(cnt)))
    return list(buf[:min(cnt.value, 4096)])


def manifest_node_slice(record_count, batch_size, node_id, node_count):
    """Record indices of one node (aeon manifest_file node slicing)."""
    cnt = ctypes.c_int64()
    _check_host(lib().aeon_manifest_node_slice(record_count, batch_size, node_id, node_count, None,
                                               ctypes.byref(cnt)))
    out = np.zeros(cnt.value, np.int64)
    _check_host(lib().aeon_manifest_node_slice(record_count, batch_size, node_id, node_count,
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               ctypes.byref(cnt)))
    return out
