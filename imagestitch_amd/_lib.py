"""ctypes binding of libvfsms.so (include/vfsms.h) -- the only compute backend of this package.

There is deliberately NO CPU fallback: if the shared library is missing or no MI355X is visible, every
operator raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VFSMS_LIB: another build of the library (A/B timing of kernel variants: tools/microbench.py, bench.py); the product is the in-tree one
LIB_PATH = os.path.abspath(os.environ["VFSMS_LIB"]) if os.environ.get("VFSMS_LIB") else os.path.join(_HERE, "lib", "libvfsms.so")

VFSMS_OK = 0
VFSMS_ERR_BAD_ARG, VFSMS_ERR_CAPACITY, VFSMS_ERR_UNSUPPORTED = -1, -2, -6
ATTEMPT_INTS = 8


class VfsmsError(RuntimeError):
    """An error the library reported.  `code` is its return code (VFSMS_ERR_*; None when the error did not come from a library call)."""

    def __init__(self, message="", code=None):
        super().__init__(message)
        self.code = code


class SurfParams(C.Structure):
    _fields_ = [("hessian_threshold", C.c_float), ("n_octaves", C.c_int32), ("n_octave_layers", C.c_int32),
                ("extended", C.c_int32), ("upright", C.c_int32)]


class OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32), ("edge_threshold", C.c_int32),
                ("first_level", C.c_int32), ("wta_k", C.c_int32), ("score_type", C.c_int32), ("patch_size", C.c_int32),
                ("fast_threshold", C.c_int32)]


class SiftParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_octave_layers", C.c_int32), ("contrast_threshold", C.c_double),
                ("edge_threshold", C.c_double), ("sigma", C.c_double)]


class AttemptKey(C.Structure):
    _fields_ = [("pair", C.c_int32), ("direction", C.c_int32), ("i", C.c_int32)]


class GridParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("offset_evaluate", C.c_int32), ("direct_incre", C.c_int32), ("window", C.c_int32),
                ("orb_max_dist", C.c_int32), ("enhance_mode", C.c_int32), ("tile_grid", C.c_int32), ("reserved", C.c_int32),
                ("roi_ratio", C.c_double), ("search_ratio", C.c_double), ("phase_threshold", C.c_double), ("clip_limit", C.c_double),
                ("surf", SurfParams), ("orb", OrbParams),
                ("path_hint", C.POINTER(C.c_int32)), ("path_hint_len", C.c_int32), ("reserved2", C.c_int32)]


ATTEMPT_EVAL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(AttemptKey), C.c_int, C.POINTER(C.c_int32))


class RoiPair(C.Structure):
    _fields_ = [("tile_a", C.c_int64), ("tile_b", C.c_int64),
                ("ay0", C.c_int32), ("ax0", C.c_int32), ("by0", C.c_int32), ("bx0", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32)]


class NccJob(C.Structure):
    _fields_ = [("tile_a", C.c_int64), ("tile_b", C.c_int64), ("dx", C.c_int32), ("dy", C.c_int32)]


KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"),
                     ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])

_SIGNATURES = {
    # name: (restype, argtypes)
    "vfsms_version": (C.c_int, []),
    "vfsms_device_count": (C.c_int, []),
    "vfsms_last_error": (C.c_int, [C.c_char_p, C.c_int]),
    "vfsms_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "vfsms_ctx_destroy": (C.c_int, [C.c_void_p]),
    "vfsms_ctx_sync": (C.c_int, [C.c_void_p]),
    "vfsms_ctx_sync_uploads": (C.c_int, [C.c_void_p]),
    "vfsms_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "vfsms_ctx_set_keypoint_capacity": (C.c_int, [C.c_void_p, C.c_int]),
    "vfsms_ctx_set_offset_estimator": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "vfsms_ctx_set_offset_verifier": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int]),
    "vfsms_ctx_set_phase_resolver": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int]),
    "vfsms_attempt_phase_resolve_batch": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_phase_resolve_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_verify_ncc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_ncc_search_batch": (C.c_int, [C.c_void_p, C.POINTER(NccJob), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_ncc_wide_batch": (C.c_int, [C.c_void_p, C.POINTER(NccJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_overlap_sums_batch": (C.c_int, [C.c_void_p, C.POINTER(NccJob), C.c_int, C.c_void_p]),
    "vfsms_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "vfsms_profile_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "vfsms_tile_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_tile_upload_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_tile_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_tile_fill": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "vfsms_tile_reserve_ch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_tile_fill_pair": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int]),
    "vfsms_tile_fill_jpeg": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]),
    "vfsms_tile_fill_jpeg_dct": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]),
    "vfsms_jpeg_coefficients": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_idct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "vfsms_tile_fill_jpeg_huff": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]),
    "vfsms_jpeg_scan": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_entropy_decode": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "vfsms_jpeg_decode": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vfsms_jpeg_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_canvas_encode_jpeg_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_join": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_canvas_blend_tile_resident": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vfsms_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vfsms_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vfsms_tile_wrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_tile_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_integral_u8_i32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_surf_detect_describe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SurfParams),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_surf_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SurfParams),
                                    C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_orb_detect_describe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(OrbParams),
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_sift_detect_describe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SiftParams),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_sift_pyramid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SiftParams),
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_attempt_orb_batch": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.POINTER(OrbParams), C.c_int, C.c_int, C.c_void_p]),
    "vfsms_attempt_sift_batch": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.POINTER(SiftParams), C.c_double, C.c_int, C.c_void_p]),
    "vfsms_bf_l2_knn2_ratio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                         C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_bf_l2_knn2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_bf_l2_knn2_u8d128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_bf_hamming_nn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_mode_offset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p]),
    "vfsms_consensus_offset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p]),
    "vfsms_phase_correlate_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]),
    "vfsms_fuse_fade_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    "vfsms_fuse_ramps_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "vfsms_attempt_surf_batch": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.POINTER(SurfParams), C.c_double,
                                           C.c_int, C.c_void_p]),
    "vfsms_attempt_surf_batch_enhanced": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.POINTER(SurfParams), C.c_double,
                                                    C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "vfsms_features_surf": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SurfParams), C.c_int, C.c_double,
                                      C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "vfsms_features_match_offset": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int, C.c_void_p]),
    "vfsms_features_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vfsms_features_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_enhance_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "vfsms_pairs_offsets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(GridParams), C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "vfsms_pairs_offsets_blind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_pairs_offsets_blind_eval": (C.c_int, [ATTEMPT_EVAL, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_pairs_offsets_eval": (C.c_int, [ATTEMPT_EVAL, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(GridParams), C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "vfsms_attempt_phase_batch": (C.c_int, [C.c_void_p, C.POINTER(RoiPair), C.c_int, C.c_void_p]),
    "vfsms_phase_plan": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "vfsms_canvas_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_canvas_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_canvas_paste": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vfsms_canvas_blend_tile": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int]),
    "vfsms_canvas_paste_tile": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "vfsms_canvas_fuse_tile_resident": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_void_p]),
    "vfsms_canvas_fuse_tile": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_canvas_assemble_resident": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_canvas_fuse_tile_resident_m": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_canvas_fuse_tile_m": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_fuse_trig_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_fuse_multiband_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    "vfsms_canvas_set_multiband_levels": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "vfsms_fuse_seam_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_canvas_set_seam_blend": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "vfsms_features_surf_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_features_match_offset_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "vfsms_canvas_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "vfsms_canvas_download_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_canvas_download_rows_pyramid": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vfsms_tiff_jpeg_tables": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vfsms_jpeg_encode_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                 C.POINTER(C.c_size_t), C.c_void_p, C.c_int]),
    "vfsms_canvas_encode_pyramid_tiles": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_size_t), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_deflate_encode_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_size_t), C.c_void_p, C.c_int]),
    "vfsms_canvas_encode_pyramid_tiles_deflate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                            C.POINTER(C.c_size_t), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vfsms_png_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "vfsms_canvas_encode_png_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "vfsms_tile_upload_ch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_shading_estimate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_shading_from_gain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_shading_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_shading_apply": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "vfsms_shading_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_focus_stack": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_focus_scores": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_deep_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_deep_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_deep_window": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_deep_reduce": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_deep_mosaic_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_deep_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "vfsms_deep_shading_estimate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_deep_shading_from_gain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vfsms_deep_shading_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "vfsms_deep_shading_apply": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "vfsms_deep_shading_free": (C.c_int, [C.c_void_p, C.c_int64]),
    "vfsms_overlap_stats_batch": (C.c_int, [C.c_void_p, C.POINTER(NccJob), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vfsms_exposure_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vfsms_block_ncc_batch": (C.c_int, [C.c_void_p, C.POINTER(NccJob), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vfsms_lens_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int]),
    "vfsms_lens_remap_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int, C.c_void_p]),
}

_lib = None


def load_library():
    """dlopen libvfsms.so and bind every declared entry point.  Raises if the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VfsmsError("libvfsms.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(make -C imagestitch_amd/csrc).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)           # AttributeError here == header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_names():
    return sorted(_SIGNATURES)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _path_arrays(shapes, handles=None):
    """what the pairs_offsets entry points take of a path -> (tile count, int32[n, 2] shapes, int64[n] tile handles or None)"""
    sh = np.ascontiguousarray(np.array([[s[0], s[1]] for s in shapes], np.int32))
    hs = None if handles is None else np.array([h if h is not None else 0 for h in handles], np.int64)
    return len(shapes), sh, hs


def _u8_2d(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("expected a 2-D uint8 image, got %s %s" % (img.dtype, img.shape))
    if img.shape[1] > 1 and img.strides[1] != 1:
        img = np.ascontiguousarray(img)
    if img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    return img


class Engine:
    """One HIP context (one GPU, one stream).  All methods are synchronous."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.vfsms_ctx_create(int(device), C.byref(h))
        self.ctx = h
        self._check(rc)
        self.device = device

    # -- plumbing ---------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != VFSMS_OK:
            buf = C.create_string_buffer(512)
            self.lib.vfsms_last_error(buf, 512)
            raise VfsmsError("libvfsms error %d: %s" % (rc, buf.value.decode(errors="replace")), code=int(rc))

    def close(self):
        if getattr(self, "ctx", None):
            for p in self.__dict__.pop("_pinned", []):
                self.lib.vfsms_host_free(self.ctx, C.c_void_p(p))
            self.lib.vfsms_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.vfsms_ctx_sync(self.ctx))
        self.__dict__.pop("_inflight", None)

    def sync_uploads(self):
        """wait for tile_upload_async copies only: their host buffers may be reused"""
        self._check(self.lib.vfsms_ctx_sync_uploads(self.ctx))
        self.__dict__.pop("_inflight", None)

    def stream_handle(self):
        return self.lib.vfsms_ctx_stream(self.ctx)

    def set_keypoint_capacity(self, cap):
        self._check(self.lib.vfsms_ctx_set_keypoint_capacity(self.ctx, int(cap)))

    OFFSET_ESTIMATORS = {"mode": 0, "ransac": 1, "consensus": 1}

    def set_offset_estimator(self, kind="mode", tol=3):
        """How the fused paths (attempt batches, pairs_offsets, features_match_offset) turn matches into an offset: "mode" (default) or
        "ransac" / "consensus" (consensus_offset with tolerance `tol` px, 0..64); 0 / 1 as in include/vfsms.h."""
        est = self.OFFSET_ESTIMATORS[kind] if isinstance(kind, str) else int(kind)
        self._check(self.lib.vfsms_ctx_set_offset_estimator(self.ctx, est, int(tol)))

    OFFSET_VERIFIERS = {"none": 0, "ncc": 1}
    VERIFY_FIXED_ONE = 1 << 20

    def set_offset_verifier(self, kind="none", threshold=0.0, min_pixels=0):
        """The acceptance check behind the vote of the fused paths (attempt batches, pairs_offsets): "none" (default) or "ncc", the
        normalised cross-correlation of the raw pixels the two strips share under the voted offset (tests/verify_ref.py); a row keeps
        status 1 iff score >= threshold, int 7 of the row is the fixed-point score; 0 / 1 as in include/vfsms.h."""
        ver = self.OFFSET_VERIFIERS[kind] if isinstance(kind, str) else int(kind)
        self._check(self.lib.vfsms_ctx_set_offset_verifier(self.ctx, ver, float(threshold), int(min_pixels)))

    PHASE_RESOLVERS = {"none": 0, "ncc": 1}
    PHASE_MAX_PEAKS = 8

    def set_phase_resolver(self, kind="none", peaks=2, threshold=0.5, min_pixels=4096):
        """How method "phase" of pairs_offsets / pairs_offsets_blind reads a correlation surface: "none" (default: the reference's arg-max,
        sign and response gate) or "ncc" (tests/phase_resolve_ref.py: the `peaks` largest peaks, every circular reading scored by overlap
        correlation, status = score >= threshold); 0 / 1 as in include/vfsms.h."""
        res = self.PHASE_RESOLVERS[kind] if isinstance(kind, str) else int(kind)
        self._check(self.lib.vfsms_ctx_set_phase_resolver(self.ctx, res, int(peaks), float(threshold), int(min_pixels)))

    def attempt_phase_resolve_batch(self, jobs, peaks=2, threshold=0.5, min_pixels=4096):
        """vfsms_attempt_phase_resolve_batch over resident tiles -> (rows int32[n, 8] = status, dx, dy, 0, 1, 1, winning candidate, fixed-point
        score; cands int32[n, 4 peaks, 4] = dx, dy, fixed-point score, shared pixels; peak positions int32[n, peaks, 2] = uy, ux)"""
        n, K = len(jobs), int(peaks)
        rows = np.zeros((n, ATTEMPT_INTS), np.int32)
        cands = np.zeros((n, 4 * max(K, 0), 4), np.int32)
        pk = np.zeros((n, max(K, 0), 2), np.int32)
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs) if n else None
        self._check(self.lib.vfsms_attempt_phase_resolve_batch(self.ctx, arr, n, K, float(threshold), int(min_pixels), _ptr(rows), _ptr(cands), _ptr(pk)))
        return rows, cands, pk

    def phase_resolve(self, a, b, peaks=2, threshold=0.5, min_pixels=4096):
        """vfsms_phase_resolve_u8 on two host strips of one shape -> (row int32[8], cands int32[4 peaks, 4], peak positions int32[peaks, 2])"""
        a = _u8_2d(a); b = _u8_2d(b)
        if a.shape != b.shape:
            raise ValueError("phase_resolve: shapes differ")
        K = int(peaks)
        row = np.zeros(ATTEMPT_INTS, np.int32); cands = np.zeros((4 * max(K, 0), 4), np.int32); pk = np.zeros((max(K, 0), 2), np.int32)
        self._check(self.lib.vfsms_phase_resolve_u8(self.ctx, _ptr(a), _ptr(b), a.shape[0], a.shape[1], a.strides[0], b.strides[0], K, float(threshold),
                                                    int(min_pixels), _ptr(row), _ptr(cands), _ptr(pk)))
        return row, cands, pk

    def verify_ncc(self, a, b, dx, dy, min_pixels=0):
        """vfsms_verify_ncc on two host strips of one shape and a raw vote (dx, dy) -> ((N, Sa, Sb, Saa, Sbb, Sab), score, fixed-point score)"""
        a = _u8_2d(a); b = _u8_2d(b)
        if a.shape != b.shape:
            raise ValueError("verify_ncc: shapes differ")
        out = np.zeros(8, np.int64)
        self._check(self.lib.vfsms_verify_ncc(self.ctx, _ptr(a), a.strides[0], _ptr(b), b.strides[0], a.shape[0], a.shape[1],
                                              int(dx), int(dy), int(min_pixels), _ptr(out)))
        return tuple(int(v) for v in out[:6]), float(out[6:7].view(np.float64)[0]), int(out[7])

    def ncc_search_batch(self, jobs, radius, min_pixels, want_surface=False):
        """vfsms_ncc_search_batch: jobs = sequence of (tile_a, tile_b, dx, dy) over resident gray tiles of one shape per job; every offset
        (dx + i, dy + j), i, j in [-radius, radius] (radius 1..16), scored as verify_ncc scores one (tests/ncc_search_ref.py).
        -> int32[n, 4] = (i, j, fixed-point score, shared pixels) of the best candidate per job [, int32[n, 2 radius + 1, 2 radius + 1], the
        fixed-point score of every candidate, with want_surface]"""
        n = len(jobs)
        side = 2 * int(radius) + 1
        best = np.zeros((n, 4), np.int32)
        surface = np.zeros((n, side, side), np.int32) if want_surface else None
        arr = (NccJob * max(n, 1))()
        for k, j in enumerate(jobs):
            arr[k] = NccJob(*[int(v) for v in j])
        self._check(self.lib.vfsms_ncc_search_batch(self.ctx, arr, n, int(radius), int(min_pixels), _ptr(best), _ptr(surface)))
        return (best, surface) if want_surface else best

    def ncc_search(self, a, b, dx, dy, radius, min_pixels):
        """ncc_search_batch for two host arrays (uint8, one shape), uploaded for the call -> ((i, j), score / VERIFY_FIXED_ONE as the
        fixed-point integer, shared pixels, int32 surface)"""
        a = _u8_2d(a); b = _u8_2d(b)
        ha = self.tile_upload(a)
        try:
            hb = self.tile_upload(b)
            try:
                best, surface = self.ncc_search_batch([(ha, hb, dx, dy)], radius, min_pixels, want_surface=True)
            finally:
                self.tile_free(hb)
        finally:
            self.tile_free(ha)
        return (int(best[0, 0]), int(best[0, 1])), int(best[0, 2]), int(best[0, 3]), surface[0]

    WIDE_MAX_RADIUS, WIDE_MAX_PEAKS = 128, 4

    @staticmethod
    def _ncc_jobs(jobs):
        arr = (NccJob * max(len(jobs), 1))()
        for k, j in enumerate(jobs):
            arr[k] = NccJob(*[int(v) for v in j])
        return arr

    def ncc_wide_batch(self, jobs, radius, factor=4, peaks=2, min_pixels=4096, want_seeds=False):
        """vfsms_ncc_wide_batch: jobs as for ncc_search_batch; the window of radius 1..128 is searched in two levels (tests/ncc_wide_ref.py):
        on the pair reduced by factor x factor block means (factor 2, 4 or 8, ceil(radius / factor) <= 16), then at full resolution with
        radius min(factor, radius) around the `peaks` (1..4) best coarse candidates.
        -> int32[n, 8] = (ti, tj, fixed-point score, shared pixels, ci, cj, coarse fixed-point score of the winning seed, seeds used): the
        offset found is (dx + ti, dy + tj) [, int32[n, 4, 6] = (ci, cj, coarse score, ti, tj, fine score) per seed, with want_seeds]"""
        n = len(jobs)
        out = np.zeros((n, 8), np.int32)
        seeds = np.zeros((n, self.WIDE_MAX_PEAKS, 6), np.int32) if want_seeds else None
        self._check(self.lib.vfsms_ncc_wide_batch(self.ctx, self._ncc_jobs(jobs), n, int(radius), int(factor), int(peaks), int(min_pixels),
                                                  _ptr(out), _ptr(seeds), None))
        return (out, seeds) if want_seeds else out

    def ncc_wide_reduce(self, a, b, dx, dy, factor):
        """the two reduced planes (A's, B's) that ncc_wide_batch searches first, for two host arrays (uint8, one shape) uploaded for the
        call: the test hook of vfsms_ncc_wide_batch"""
        a = _u8_2d(a); b = _u8_2d(b)
        f = int(factor)
        if a.shape != b.shape or f not in (2, 4, 8):
            raise ValueError("ncc_wide_reduce: two arrays of one shape and a factor of 2, 4 or 8")
        ha = self.tile_upload(a)
        try:
            hb = self.tile_upload(b)
            try:
                return self.ncc_wide_reduce_tiles(ha, hb, a.shape, dx, dy, f)
            finally:
                self.tile_free(hb)
        finally:
            self.tile_free(ha)

    def ncc_wide_reduce_tiles(self, tile_a, tile_b, shape, dx, dy, factor):
        """ncc_wide_reduce for two resident gray tiles of `shape`"""
        f = int(factor)
        hc, wc = (int(shape[0]) - int(dx) % f) // f, (int(shape[1]) - int(dy) % f) // f
        red = np.zeros((2, max(hc, 0), max(wc, 0)), np.uint8)
        out = np.zeros((1, 8), np.int32)
        self._check(self.lib.vfsms_ncc_wide_batch(self.ctx, self._ncc_jobs([(tile_a, tile_b, dx, dy)]), 1, f, f, 1, 0, _ptr(out), None, _ptr(red)))
        return red[0], red[1]

    def overlap_sums_batch(self, jobs):
        """vfsms_overlap_sums_batch: jobs as for ncc_search_batch -> int64[n, 6] = (N, Sa, Sb, Saa, Sbb, Sab) over the pixels the two tiles
        share at the job's own offset (tests/verify_ref.py: sums)"""
        n = len(jobs)
        out = np.zeros((n, 6), np.int64)
        self._check(self.lib.vfsms_overlap_sums_batch(self.ctx, self._ncc_jobs(jobs), n, _ptr(out)))
        return out

    def profile_enable(self, on=True):
        self._check(self.lib.vfsms_profile_enable(self.ctx, int(bool(on))))

    def profile_read(self, reset=True):
        """-> {stage: (total_ms, launch_groups)} measured with HIP events on the engine's stream."""
        names = C.create_string_buffer(4096)
        ms = np.zeros(64, np.float64); calls = np.zeros(64, np.int64)
        n = C.c_int()
        self._check(self.lib.vfsms_profile_read(self.ctx, names, 4096, _ptr(ms), _ptr(calls), 64, C.byref(n), int(bool(reset))))
        keys = names.value.decode().split(",") if n.value else []
        return {k: (float(ms[i]), int(calls[i])) for i, k in enumerate(keys)}

    # -- tiles ---------------------------------------------------------------------------------------------
    def tile_upload(self, img):
        img = _u8_2d(img)
        h = C.c_int64()
        self._check(self.lib.vfsms_tile_upload(self.ctx, _ptr(img), img.shape[0], img.shape[1], img.strides[0], C.byref(h)))
        return self._note_tile(h.value, img.shape)

    def tile_reserve(self, h, w):
        """handle of a gray tile whose pixels a decoder thread delivers later (tile_fill); batch calls wait for exactly the tiles they name"""
        hd = C.c_int64()
        self._check(self.lib.vfsms_tile_reserve(self.ctx, int(h), int(w), C.byref(hd)))
        return self._note_tile(hd.value, (int(h), int(w)))

    def tile_reserve_color(self, h, w, ch=3):
        """tile_reserve for an interleaved tile of `ch` channels (the mosaic's colour tiles)"""
        hd = C.c_int64()
        self._check(self.lib.vfsms_tile_reserve_ch(self.ctx, int(h), int(w), int(ch), C.byref(hd)))
        return self._note_tile(hd.value, (int(h), int(w), int(ch)))

    def tile_fill(self, handle, img):
        """deliver (img: u8 (h, w) or (h, w, ch) array, C-contiguous rows) or give up on (img is None) a reserved tile; safe from any thread"""
        if img is None:
            self._check(self.lib.vfsms_tile_fill(self.ctx, C.c_int64(handle), None, 0))
            return
        assert img.dtype == np.uint8 and img.ndim in (2, 3) and img.strides[-1] == 1 and (img.ndim == 2 or img.strides[1] == img.shape[2])
        self._check(self.lib.vfsms_tile_fill(self.ctx, C.c_int64(handle), _ptr(img), img.strides[0]))

    SRC_GRAY8, SRC_YCC24, SRC_YCCX32 = 0, 1, 2

    def tile_fill_pair(self, gray_handle, color_handle, address, stride_bytes, fmt):
        """One decoded image -> the reserved gray tile and / or the reserved BGR tile (vfsms_tile_fill_pair; either handle may be 0 / None);
        `address`: raw host address of the decoder's output in format `fmt` (SRC_*), None gives both tiles up.  Safe from any thread."""
        self._check(self.lib.vfsms_tile_fill_pair(self.ctx, C.c_int64(gray_handle or 0), C.c_int64(color_handle or 0),
                                                  C.c_void_p(address) if address is not None else None, int(stride_bytes), int(fmt)))

    def _fill_from_file(self, entry, gray_handle, color_handle, data):
        """one of the three JPEG hand-overs: True when the tiles are filled, False when the entry hands the file back (tiles still reserved)"""
        rc = getattr(self.lib, entry)(self.ctx, C.c_int64(gray_handle or 0), C.c_int64(color_handle or 0), data, len(data))
        if rc in (VFSMS_ERR_UNSUPPORTED, VFSMS_ERR_BAD_ARG):
            return False
        self._check(rc)
        return True

    def tile_fill_jpeg(self, gray_handle, color_handle, data):
        """A JPEG file's bytes -> the reserved gray tile and / or the reserved BGR tile, decoded by the library itself (vfsms_tile_fill_jpeg:
        libjpeg-turbo into pinned staging, colour conversion on the device).  True when the tiles are filled; False when this decoder does
        not take the file (no libjpeg.so.8, an unusual colour space, a damaged file, a size other than the tiles'): the tiles are STILL
        RESERVED and the caller decodes some other way.  Safe from any thread."""
        return self._fill_from_file("vfsms_tile_fill_jpeg", gray_handle, color_handle, data)

    def tile_fill_jpeg_dct(self, gray_handle, color_handle, data):
        """tile_fill_jpeg with the device half of the decoder (vfsms_tile_fill_jpeg_dct, Method.jpegDecoder = "device"): the host stops behind
        the entropy decode, dequantisation and inverse DCT run on the device (csrc/jpeg_dec_kernels.hip).  Same bytes in the tiles, same
        answer: True when they are filled, False when this path does not take the file -- the tiles are STILL RESERVED, tile_fill_jpeg is
        next.  Safe from any thread."""
        return self._fill_from_file("vfsms_tile_fill_jpeg_dct", gray_handle, color_handle, data)

    def tile_fill_jpeg_huff(self, gray_handle, color_handle, data):
        """tile_fill_jpeg with the whole decoder on the device (vfsms_tile_fill_jpeg_huff, Method.jpegDecoder = "device-entropy"): the host scans
        the file for its markers, the compressed bytes cross the link, Huffman decode, DC prediction, dequantisation and inverse DCT run on the
        device (csrc/jpeg_huff_kernels.hip, csrc/jpeg_dec_kernels.hip).  Same bytes in the tiles, same answer: True when they are filled, False
        when this path does not take the file -- the tiles are STILL RESERVED, tile_fill_jpeg_dct or tile_fill_jpeg is next.  Any thread."""
        return self._fill_from_file("vfsms_tile_fill_jpeg_huff", gray_handle, color_handle, data)

    def jpeg_scan(self, data):
        """the module's jpeg_scan (vfsms_jpeg_scan: host only, no GPU): the scan record of a file as a dict, or its refusal code"""
        return jpeg_scan(data)

    def jpeg_entropy_decode(self, data, max_rounds=-1):
        """vfsms_jpeg_entropy_decode, the bare operator: file bytes -> (rc, h, w, comps, rounds_used), comps as jpeg_coefficients returns them
        -- [(coef int16 (block_rows, block_cols, 64), quant uint16 (64,))] -- decoded by the device.  rc: VFSMS_OK, or VFSMS_ERR_UNSUPPORTED /
        VFSMS_ERR_BAD_ARG with comps None (a file not taken or not in step after max_rounds repair rounds / a damaged file).  max_rounds -1:
        as many as there are subsequences."""
        h, w, nc, need, used = C.c_int(), C.c_int(), C.c_int(), C.c_size_t(), C.c_int()
        grid = (C.c_int * 6)()
        args = (C.byref(h), C.byref(w), C.byref(nc), grid, C.byref(need), C.byref(used))
        rc = self.lib.vfsms_jpeg_entropy_decode(self.ctx, data, len(data), int(max_rounds), None, 0, *args)
        if rc in (VFSMS_ERR_UNSUPPORTED, VFSMS_ERR_BAD_ARG):
            return rc, 0, 0, None, 0
        if rc != VFSMS_ERR_CAPACITY:
            self._check(rc)
        out = np.empty(need.value, np.uint8)
        rc = self.lib.vfsms_jpeg_entropy_decode(self.ctx, data, len(data), int(max_rounds), out.ctypes.data_as(C.c_void_p), out.nbytes, *args)
        if rc in (VFSMS_ERR_UNSUPPORTED, VFSMS_ERR_BAD_ARG):
            return rc, h.value, w.value, None, 0
        self._check(rc)
        return rc, h.value, w.value, _coefficient_layout(out, nc.value, grid), used.value

    def jpeg_idct(self, coef, quant, pitch=None):
        """vfsms_jpeg_idct, the bare operator: `coef` int16 (block_rows, block_cols, 64), quantised coefficients in natural order, and `quant`
        uint16 (64,) -> the u8 plane (block_rows * 8, block_cols * 8) of tests/jpeg_dec_ref.py's idct_plane (rows `pitch` bytes apart when
        given: the plane is a view of a wider array)."""
        coef = np.ascontiguousarray(coef, np.int16)
        quant = np.ascontiguousarray(quant, np.uint16)
        if coef.ndim != 3 or coef.shape[2] != 64 or quant.shape != (64,):
            raise ValueError("jpeg_idct: coef (block_rows, block_cols, 64) int16 and quant (64,) uint16")
        br, bc = coef.shape[:2]
        pitch = bc * 8 if pitch is None else int(pitch)
        out = np.zeros((br * 8, max(pitch, 1)), np.uint8)
        self._check(self.lib.vfsms_jpeg_idct(self.ctx, _ptr(coef), _ptr(quant), br, bc, _ptr(out), pitch))
        return out[:, :bc * 8]

    def tile_fill_ptr(self, handle, address, stride):
        """tile_fill from a raw host address (rows `stride` bytes apart); the caller keeps the memory alive until this returns"""
        self._check(self.lib.vfsms_tile_fill(self.ctx, C.c_int64(handle), C.c_void_p(address), int(stride)))

    def tile_upload_async(self, img):
        """Upload without waiting: the copy overlaps the compute stream; `img` must stay alive and unchanged until sync() or
        the first synchronous call that used the tile (arrays from pinned_empty() make the copy a true asynchronous DMA)."""
        img = _u8_2d(img)
        h = C.c_int64()
        self._check(self.lib.vfsms_tile_upload_async(self.ctx, _ptr(img), img.shape[0], img.shape[1], img.strides[0], C.byref(h)))
        self.__dict__.setdefault("_inflight", []).append(img)
        return self._note_tile(h.value, img.shape)

    def tile_upload_color(self, img, asynchronous=False):
        """Interleaved colour tile (h, w, ch) u8 for the mosaic canvas (vfsms_tile_upload_ch); asynchronous like tile_upload_async."""
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim != 3:
            raise ValueError("tile_upload_color takes an (h, w, ch) array")
        h = C.c_int64()
        self._check(self.lib.vfsms_tile_upload_ch(self.ctx, _ptr(img), img.shape[0], img.shape[1], img.shape[2], img.strides[0],
                                                  1 if asynchronous else 0, C.byref(h)))
        if asynchronous:
            self.__dict__.setdefault("_inflight", []).append(img)
        return self._note_tile(h.value, img.shape)

    def pinned_empty(self, shape, dtype=np.uint8):
        """numpy array over pinned host memory (vfsms_host_alloc); freed when the engine closes."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self.lib.vfsms_host_alloc(self.ctx, C.c_size_t(max(n, 1)), C.byref(p)))
        self.__dict__.setdefault("_pinned", []).append(p.value)
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def tile_wrap(self, device_ptr, h, w, stride):
        hd = C.c_int64()
        self._check(self.lib.vfsms_tile_wrap(self.ctx, C.c_void_p(int(device_ptr)), int(h), int(w), int(stride), C.byref(hd)))
        return self._note_tile(hd.value, (int(h), int(w)))

    def tile_free(self, handle):
        self._check(self.lib.vfsms_tile_free(self.ctx, C.c_int64(handle)))
        self.__dict__.get("_shapes", {}).pop(("tile", handle), None)

    def _note_tile(self, handle, shape):
        """the shape behind a tile handle: shading_download sizes its arrays by it (the C ABI reports no shapes)"""
        self.__dict__.setdefault("_shapes", {})[("tile", handle)] = tuple(int(v) for v in shape)
        return handle

    # -- operators -------------------------------------------------------------------------------------------
    def integral(self, img):
        img = _u8_2d(img)
        h, w = img.shape
        out = np.empty((h + 1, w + 1), np.int32)
        self._check(self.lib.vfsms_integral_u8_i32(self.ctx, _ptr(img), h, w, img.strides[0], _ptr(out)))
        return out

    @staticmethod
    def surf_params(hessian=100.0, n_octaves=4, n_layers=3, extended=False, upright=False):
        return SurfParams(float(hessian), int(n_octaves), int(n_layers), int(bool(extended)), int(bool(upright)))

    def surf_detect_describe(self, img, params=None, cap=None, full=False):
        img = _u8_2d(img)
        h, w = img.shape
        params = params or self.surf_params()
        cap = cap or (h * w // 24 + 4096)
        d = 128 if params.extended else 64
        kxy = np.empty((cap, 2), np.float32)
        desc = np.empty((cap, d), np.float32)
        kfull = np.empty(cap, KP_DTYPE) if full else None
        n = C.c_int()
        self._check(self.lib.vfsms_surf_detect_describe(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params),
                                                        _ptr(kxy), _ptr(desc), _ptr(kfull), cap, C.byref(n)))
        n = n.value
        if full:
            return kxy[:n].copy(), desc[:n].copy(), kfull[:n].copy()
        return kxy[:n].copy(), desc[:n].copy()

    def surf_detect(self, img, params=None, cap=None):
        img = _u8_2d(img)
        h, w = img.shape
        params = params or self.surf_params()
        cap = cap or (h * w // 24 + 4096)
        kfull = np.empty(cap, KP_DTYPE)
        n = C.c_int()
        self._check(self.lib.vfsms_surf_detect(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params),
                                               _ptr(kfull), cap, C.byref(n)))
        return kfull[:n.value].copy()

    @staticmethod
    def orb_params(nfeatures=5000, scale_factor=1.2, nlevels=8, edge_threshold=31, first_level=0, wta_k=2, score_type=0,
                   patch_size=31, fast_threshold=20):
        return OrbParams(int(nfeatures), float(scale_factor), int(nlevels), int(edge_threshold), int(first_level), int(wta_k),
                         int(score_type), int(patch_size), int(fast_threshold))

    def orb_detect_describe(self, img, params=None, cap=None, full=False):
        img = _u8_2d(img)
        h, w = img.shape
        params = params or self.orb_params()
        auto = not cap
        cap = cap or (2 * params.n_features + 2048)
        n = C.c_int(-1)
        while True:
            kxy = np.empty((cap, 2), np.float32)
            desc = np.empty((cap, 32), np.uint8)
            kfull = np.empty(cap, KP_DTYPE) if full else None
            rc = self.lib.vfsms_orb_detect_describe(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params),
                                                    _ptr(kxy), _ptr(desc), _ptr(kfull), cap, C.byref(n))
            # ties keep more than n_features: with no cap given, run once more with the count the library reports
            if auto and rc == VFSMS_ERR_CAPACITY and n.value > cap:
                auto, cap = False, n.value
                continue
            self._check(rc)
            break
        n = n.value
        if full:
            return kxy[:n].copy(), desc[:n].copy(), kfull[:n].copy()
        return kxy[:n].copy(), desc[:n].copy()

    @staticmethod
    def sift_params(n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, n_features=0):
        """cv2.xfeatures2d.SIFT_create() defaults; n_features > 0 (retainBest) is refused by the library"""
        return SiftParams(int(n_features), int(n_octave_layers), float(contrast_threshold), float(edge_threshold), float(sigma))

    def sift_detect_describe(self, img, params=None, cap=None, full=False):
        """-> (kps float32[N, 2], desc float32[N, 128]) [+ KP_DTYPE keypoints if full], keypoints in detection order"""
        img = _u8_2d(img)
        h, w = img.shape
        params = params or self.sift_params()
        cap = (h * w // 16 + 4096) if cap is None else int(cap)
        kxy = np.empty((max(cap, 1), 2), np.float32)
        desc = np.empty((max(cap, 1), 128), np.float32)
        kfull = np.empty(max(cap, 1), KP_DTYPE) if full else None
        n = C.c_int()
        self._check(self.lib.vfsms_sift_detect_describe(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params),
                                                        _ptr(kxy), _ptr(desc), _ptr(kfull), cap, C.byref(n)))
        n = n.value
        if full:
            return kxy[:n].copy(), desc[:n].copy(), kfull[:n].copy()
        return kxy[:n].copy(), desc[:n].copy()

    def sift_pyramid(self, img, params=None):
        """-> (gauss, dog): per octave a list of float32 levels (n_octave_layers + 3 Gaussian, n_octave_layers + 2 DoG)"""
        img = _u8_2d(img)
        h, w = img.shape
        params = params or self.sift_params()
        shapes = np.zeros((32, 2), np.int32)
        nref = C.c_int()
        self._check(self.lib.vfsms_sift_pyramid(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params), None, None, 0,
                                                _ptr(shapes), 32, C.byref(nref)))
        no = nref.value
        L = params.n_octave_layers
        gn = sum((L + 3) * int(r) * int(c) for r, c in shapes[:no])
        dn = sum((L + 2) * int(r) * int(c) for r, c in shapes[:no])
        g = np.empty(max(gn, 1), np.float32)
        d = np.empty(max(dn, 1), np.float32)
        self._check(self.lib.vfsms_sift_pyramid(self.ctx, _ptr(img), h, w, img.strides[0], C.byref(params), _ptr(g), _ptr(d), g.size,
                                                _ptr(shapes), 32, C.byref(nref)))
        gauss, dog, go, do = [], [], 0, 0
        for r, c in shapes[:no]:
            r, c = int(r), int(c)
            gauss.append([g[go + i * r * c:go + (i + 1) * r * c].reshape(r, c).copy() for i in range(L + 3)])
            dog.append([d[do + i * r * c:do + (i + 1) * r * c].reshape(r, c).copy() for i in range(L + 2)])
            go += (L + 3) * r * c
            do += (L + 2) * r * c
        return gauss, dog

    def attempt_orb_batch(self, jobs, params=None, max_dist=-1, offset_evaluate=3):
        n = len(jobs)
        out = np.zeros((n, ATTEMPT_INTS), np.int32)
        if n == 0:
            return out
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        params = params or self.orb_params()
        self._check(self.lib.vfsms_attempt_orb_batch(self.ctx, arr, n, C.byref(params), int(max_dist), int(offset_evaluate), _ptr(out)))
        return out

    def attempt_sift_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        """n fused SIFT + BF-L2 + ratio + vote attempts on resident tiles: int32[n][ATTEMPT_INTS] rows laid out as attempt_surf_batch's"""
        n = len(jobs)
        out = np.zeros((n, ATTEMPT_INTS), np.int32)
        if n == 0:
            return out
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        params = params or self.sift_params()
        self._check(self.lib.vfsms_attempt_sift_batch(self.ctx, arr, n, C.byref(params), float(ratio), int(offset_evaluate), _ptr(out)))
        return out

    def bf_l2_ratio_matches(self, q, t, ratio=0.75):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        nq, nt = len(q), len(t)
        if nq == 0 or nt == 0:
            return np.zeros((0, 2), np.int32)
        dim = q.shape[1]
        pairs = np.empty((nq, 2), np.int32)
        m = C.c_int()
        self._check(self.lib.vfsms_bf_l2_knn2_ratio(self.ctx, _ptr(q), nq, _ptr(t), nt, dim, float(ratio), _ptr(pairs), nq, C.byref(m)))
        return pairs[:m.value].copy()

    def bf_l2_knn2(self, q, t):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        nq, nt = len(q), len(t)
        dim = q.shape[1] if nq else (t.shape[1] if nt else 64)
        i1 = np.empty(nq, np.int32); d1 = np.empty(nq, np.float32); d2 = np.empty(nq, np.float32)
        self._check(self.lib.vfsms_bf_l2_knn2(self.ctx, _ptr(q), nq, _ptr(t), nt, dim, _ptr(i1), _ptr(d1), _ptr(d2)))
        return i1, d1, d2

    def bf_l2_knn2_u8d128(self, q, t, nsplit=0):
        """vfsms_bf_l2_knn2_u8d128: (i1, d1, d2) of bf_l2_knn2 from the integer matrix-core search of the fused SIFT batch, for (n, 128)
        rows whose elements are integers 0..255 (anything else raises VfsmsError).  nsplit 1..8: that many train splits; 0: the batch's
        own rule for one job.  A test and diagnostic operator."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 128); t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
        nq, nt = len(q), len(t)
        i1 = np.empty(nq, np.int32); d1 = np.empty(nq, np.float32); d2 = np.empty(nq, np.float32)
        self._check(self.lib.vfsms_bf_l2_knn2_u8d128(self.ctx, _ptr(q), nq, _ptr(t), nt, int(nsplit), _ptr(i1), _ptr(d1), _ptr(d2)))
        return i1, d1, d2

    def bf_hamming_matches(self, q, t, max_dist=-1):
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        nq, nt = len(q), len(t)
        if nq == 0 or nt == 0:
            return np.zeros((0, 2), np.int32)
        pairs = np.empty((nq, 2), np.int32)
        m = C.c_int()
        self._check(self.lib.vfsms_bf_hamming_nn(self.ctx, _ptr(q), nq, _ptr(t), nt, q.shape[1], int(max_dist), _ptr(pairs), nq, C.byref(m)))
        return pairs[:m.value].copy()

    def mode_offset(self, kpsA, kpsB, pairs, offset_evaluate=3):
        kpsA = np.ascontiguousarray(kpsA, np.float32).reshape(-1, 2)
        kpsB = np.ascontiguousarray(kpsB, np.float32).reshape(-1, 2)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_mode_offset(self.ctx, _ptr(kpsA), len(kpsA), _ptr(kpsB), len(kpsB), _ptr(pairs), len(pairs),
                                               int(offset_evaluate), _ptr(out)))
        return bool(out[0]), [int(out[1]), int(out[2])], int(out[3])

    def consensus_offset(self, kpsA, kpsB, pairs, tol=3, offset_evaluate=3):
        """Method.getOffsetByRansac's estimator (tests/consensus_ref.py) -> (status, [dx, dy], support)."""
        kpsA = np.ascontiguousarray(kpsA, np.float32).reshape(-1, 2)
        kpsB = np.ascontiguousarray(kpsB, np.float32).reshape(-1, 2)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_consensus_offset(self.ctx, _ptr(kpsA), len(kpsA), _ptr(kpsB), len(kpsB), _ptr(pairs), len(pairs),
                                                    int(tol), int(offset_evaluate), _ptr(out)))
        return bool(out[0]), [int(out[1]), int(out[2])], int(out[3])

    def phase_correlate(self, a, b):
        a = _u8_2d(a); b = _u8_2d(b)
        if a.shape != b.shape:
            raise ValueError("phase_correlate: shapes differ")
        out = np.zeros(3, np.float64)
        self._check(self.lib.vfsms_phase_correlate_u8(self.ctx, _ptr(a), _ptr(b), a.shape[0], a.shape[1], a.strides[0], b.strides[0], _ptr(out)))
        return (float(out[0]), float(out[1])), float(out[2])

    def phase_plan(self, h, w):
        """-> dict: how a strip of h x w is correlated (vfsms_phase_plan): the LDS transforms or rocFFT, orientation, padded sizes, workgroup shapes"""
        info = np.zeros(8, np.int32)
        self._check(self.lib.vfsms_phase_plan(int(h), int(w), _ptr(info)))
        keys = ("lds_transforms", "transposed", "M", "N", "columns_per_workgroup", "rows_per_workgroup", "row_threads", "column_threads")
        return {k: int(v) for k, v in zip(keys, info)}

    def fuse_fade_i64(self, A, B, dx, dy, return_info=False):
        A = np.ascontiguousarray(A, np.int64); B = np.ascontiguousarray(B, np.int64)
        if A.shape != B.shape:
            raise ValueError("fuse: shapes differ")
        r, c = A.shape[:2]
        ch = 1 if A.ndim == 2 else A.shape[2]
        out = np.empty(A.shape, np.uint8)
        info = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_fuse_fade_i64(self.ctx, _ptr(A), _ptr(B), r, c, ch, int(dx), int(dy), _ptr(out), _ptr(info)))
        return (out, info) if return_info else out

    def fuse_trig_i64(self, A, B, dx, dy, return_info=False):
        """ImageFusion.fuseByTrigonometric on int64 regions (-1 = empty) -> uint8"""
        A = np.ascontiguousarray(A, np.int64); B = np.ascontiguousarray(B, np.int64)
        if A.shape != B.shape:
            raise ValueError("fuse: shapes differ")
        r, c = A.shape[:2]
        ch = 1 if A.ndim == 2 else A.shape[2]
        out = np.empty(A.shape, np.uint8)
        info = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_fuse_trig_i64(self.ctx, _ptr(A), _ptr(B), r, c, ch, int(dx), int(dy), _ptr(out), _ptr(info)))
        return (out, info) if return_info else out

    def fuse_multiband_i64(self, A, B, dx, dy, levels=4, return_info=False):
        """multiBandBlending on int64 regions (-1 = empty) -> uint8: seam where the fade's weights tie, Laplacian pyramid of `levels`
        levels (vfsms_fuse_multiband_i64; the arithmetic is the library's own, tests/multiband_ref.py)."""
        A = np.ascontiguousarray(A, np.int64); B = np.ascontiguousarray(B, np.int64)
        if A.shape != B.shape:
            raise ValueError("fuse: shapes differ")
        r, c = A.shape[:2]
        ch = 1 if A.ndim == 2 else A.shape[2]
        out = np.empty(A.shape, np.uint8)
        info = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_fuse_multiband_i64(self.ctx, _ptr(A), _ptr(B), r, c, ch, int(dx), int(dy), int(levels), _ptr(out), _ptr(info)))
        return (out, info) if return_info else out

    SEAM_BLENDS = {"none": 0, "multiBandBlending": 1}

    def fuse_seam_i64(self, A, B, dx, dy, blend="none", levels=4, return_info=False, return_seam=False):
        """optimalSeamLine on int64 regions (-1 = empty) -> uint8: a minimum-cost seam inside the fade's geometry; blend "none" takes every
        pixel from one input, "multiBandBlending" feeds the label plane to the pyramid blend with `levels` levels (vfsms_fuse_seam_i64; the
        arithmetic is the library's own, tests/seam_ref.py).  return_seam: also the int32 [r + c] seam (the vertical seam's column per row,
        then the horizontal seam's row per column, -1 where a seam does not exist)."""
        if blend not in self.SEAM_BLENDS:
            raise ValueError("seamLineBlend must be 'none' or 'multiBandBlending'")
        A = np.ascontiguousarray(A, np.int64); B = np.ascontiguousarray(B, np.int64)
        if A.shape != B.shape:
            raise ValueError("fuse: shapes differ")
        r, c = A.shape[:2]
        ch = 1 if A.ndim == 2 else A.shape[2]
        out = np.empty(A.shape, np.uint8)
        info = np.zeros(4, np.int32)
        seam = np.empty(r + c, np.int32)
        self._check(self.lib.vfsms_fuse_seam_i64(self.ctx, _ptr(A), _ptr(B), r, c, ch, int(dx), int(dy), self.SEAM_BLENDS[blend], int(levels),
                                                 _ptr(out), _ptr(info), _ptr(seam) if return_seam else None))
        res = (out,) + ((info,) if return_info else ()) + ((seam,) if return_seam else ())
        return res if len(res) > 1 else out

    def fuse_ramps_i64(self, A, dx, dy, force_corner=False):
        """-> ((wA_r, wB_r, wA_c, wB_c), info): the separable float32 ramps of the fade blend / getWeightsMatrix."""
        A = np.ascontiguousarray(A, np.int64)
        r, c = A.shape[:2]
        ch = 1 if A.ndim == 2 else A.shape[2]
        ramps = np.empty(2 * (r + c), np.float32)
        info = np.zeros(4, np.int32)
        self._check(self.lib.vfsms_fuse_ramps_i64(self.ctx, _ptr(A), r, c, ch, int(dx), int(dy), int(bool(force_corner)),
                                                  _ptr(ramps), _ptr(info)))
        return (ramps[:r].copy(), ramps[r:2 * r].copy(), ramps[2 * r:2 * r + c].copy(), ramps[2 * r + c:].copy()), info

    # -- fused fast path ----------------------------------------------------------------------------------------
    @staticmethod
    def make_jobs(jobs):
        arr = (RoiPair * len(jobs))()
        for k, j in enumerate(jobs):
            arr[k] = RoiPair(*[int(v) for v in j])
        return arr

    def attempt_surf_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        """jobs: sequence of (tile_a, tile_b, ay0, ax0, by0, bx0, h, w) -> int32[n, 8]
        columns: status, dx, dy, votes, nA, nB, nMatches, 0   (raw vote, before the stitch-axis correction)."""
        n = len(jobs)
        out = np.zeros((n, ATTEMPT_INTS), np.int32)
        if n == 0:
            return out
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        params = params or self.surf_params()
        self._check(self.lib.vfsms_attempt_surf_batch(self.ctx, arr, n, C.byref(params), float(ratio), int(offset_evaluate), _ptr(out)))
        return out

    def attempt_surf_batch_enhanced(self, jobs, params=None, ratio=0.75, offset_evaluate=3, enhance=(0, 0.0, 0)):
        """attempt_surf_batch with every ROI strip equalised (enhance = (1, 0, 0)) or CLAHE'd (enhance = (2, clipLimit, tileSize))
        first, as Stitcher.py:327-334 does when Method.isEnhance is set."""
        n = len(jobs)
        out = np.zeros((n, ATTEMPT_INTS), np.int32)
        if n == 0:
            return out
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        params = params or self.surf_params()
        self._check(self.lib.vfsms_attempt_surf_batch_enhanced(self.ctx, arr, n, C.byref(params), float(ratio), int(offset_evaluate),
                                                               int(enhance[0]), float(enhance[1]), int(enhance[2]), _ptr(out)))
        return out

    # -- whole shooting paths ------------------------------------------------------------------------------------------------
    @staticmethod
    def grid_params(method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1, window=24, surf=None, orb=None,
                    phaseResponseThreshold=0.15, orbMaxDistance=-1, enhance=(0, 0.0, 0), hint=None):
        p = GridParams()
        if hint is not None and len(hint):
            arr = np.ascontiguousarray(hint, np.int32)
            p._hint_keepalive = arr                          # the struct only holds the address
            p.path_hint = arr.ctypes.data_as(C.POINTER(C.c_int32))
            p.path_hint_len = len(arr)
        p.method = {"surf": 0, "orb": 1, "phase": 2, "sift": 3}[method]     # 3: evaluator-supplied only (pairs_offsets_eval, _blind_eval)
        p.offset_evaluate, p.direct_incre, p.window, p.orb_max_dist = int(offsetEvaluate), int(directIncre), int(window), int(orbMaxDistance)
        p.enhance_mode, p.clip_limit, p.tile_grid = int(enhance[0]), float(enhance[1]), int(enhance[2])
        p.roi_ratio, p.search_ratio, p.phase_threshold = float(roiRatio), float(searchRatio), float(phaseResponseThreshold)
        p.surf = surf or Engine.surf_params()
        p.orb = orb or Engine.orb_params()
        return p

    def pairs_offsets(self, handles, shapes, params, first=0, last=None, direction=1, midpath=False, stop_on_fail=False):
        """vfsms_pairs_offsets: every pair of [first, last) of the path through the library's own candidate state machine.
        -> (int32[last-first, 6] = status, dx, dy, direction, i, votes; direction out; (attempts, batches, capacity retries))."""
        n, sh, hs = _path_arrays(shapes, handles)
        last = n - 1 if last is None else last
        out = np.zeros((max(last - first, 0), 6), np.int32)
        d_out = C.c_int32()
        stats = np.zeros(8, np.int64)
        self._check(self.lib.vfsms_pairs_offsets(self.ctx, _ptr(hs), _ptr(sh), n, int(first), int(last), int(direction), int(bool(midpath)),
                                                 int(bool(stop_on_fail)), C.byref(params), _ptr(out), C.byref(d_out), _ptr(stats)))
        return out, d_out.value, tuple(int(v) for v in stats)

    def pairs_offsets_blind(self, handles, shapes, params, first, last, per):
        """vfsms_pairs_offsets_blind: the chunk [first, last) for every possible incoming direction -> (int32[4, per, 6], int32[4] directions out, stats)."""
        n, sh, hs = _path_arrays(shapes, handles)
        out = np.zeros((4, max(per, 1), 6), np.int32)
        d_out = np.zeros(4, np.int32)
        stats = np.zeros(8, np.int64)
        self._check(self.lib.vfsms_pairs_offsets_blind(self.ctx, _ptr(hs), _ptr(sh), n, int(first), int(last), int(max(per, 1)), C.byref(params),
                                                       _ptr(out), _ptr(d_out), _ptr(stats)))
        return out[:, :per], d_out, tuple(int(v) for v in stats)

    # -- resident feature sets (Stitcher.tempImageFeature's payload kept in HBM) -----------------------------------------------
    def features_surf(self, tile_handle, rect, params=None, enhance=(0, 0.0, 0)):
        """SURF of rect = (y0, x0, h, w) of a resident tile -> (feature handle, n keypoints); nothing returns to the host."""
        params = params or self.surf_params()
        f, n = C.c_int64(), C.c_int()
        y0, x0, h, w = [int(v) for v in rect]
        self._check(self.lib.vfsms_features_surf(self.ctx, C.c_int64(tile_handle), y0, x0, h, w, C.byref(params), int(enhance[0]),
                                                 float(enhance[1]), int(enhance[2]), C.byref(f), C.byref(n)))
        return f.value, n.value

    def features_surf_batch(self, tile_handles, params=None, enhance=(0, 0.0, 0)):
        """whole-tile SURF of many resident tiles in fused launches -> (feature handles, keypoint counts)"""
        params = params or self.surf_params()
        n = len(tile_handles)
        th = np.ascontiguousarray(tile_handles, np.int64)
        feats = np.zeros(max(n, 1), np.int64); counts = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.vfsms_features_surf_batch(self.ctx, _ptr(th), n, C.byref(params), int(enhance[0]), float(enhance[1]), int(enhance[2]),
                                                       _ptr(feats), _ptr(counts)))
        return [int(f) for f in feats[:n]], [int(c) for c in counts[:n]]

    def features_match_offset_batch(self, feats_a, feats_b, ratio=0.75, offset_evaluate=3):
        """matchDescriptors + getOffsetByMode of n (A, B) jobs in one batch -> int32[n][8]"""
        n = len(feats_a)
        fa = np.ascontiguousarray(feats_a, np.int64); fb = np.ascontiguousarray(feats_b, np.int64)
        out = np.zeros((max(n, 1), ATTEMPT_INTS), np.int32)
        self._check(self.lib.vfsms_features_match_offset_batch(self.ctx, _ptr(fa), _ptr(fb), n, float(ratio), int(offset_evaluate), _ptr(out)))
        return out[:n]

    def features_match_offset(self, feat_a, feat_b, ratio=0.75, offset_evaluate=3):
        """matchDescriptors + getOffsetByMode on two resident sets -> int32[8] = status, dx, dy, votes, nA, nB, nMatches, 0."""
        out = np.zeros(ATTEMPT_INTS, np.int32)
        self._check(self.lib.vfsms_features_match_offset(self.ctx, C.c_int64(feat_a), C.c_int64(feat_b), float(ratio), int(offset_evaluate), _ptr(out)))
        return out

    def features_download(self, feat, n, dim=64):
        kxy = np.empty((max(n, 1), 2), np.float32); desc = np.empty((max(n, 1), dim), np.float32)
        nn, dd = C.c_int(), C.c_int()
        self._check(self.lib.vfsms_features_download(self.ctx, C.c_int64(feat), _ptr(kxy), _ptr(desc), max(n, 1), C.byref(nn), C.byref(dd)))
        return kxy[:nn.value].copy(), desc[:nn.value].copy()

    def features_free(self, feat):
        self._check(self.lib.vfsms_features_free(self.ctx, C.c_int64(feat)))

    def enhance(self, img, mode, clip_limit=20.0, tile_size=5):
        """mode 1: cv2.equalizeHist(img); mode 2: cv2.createCLAHE(clip_limit, (tile_size, tile_size)).apply(img)."""
        img = _u8_2d(img)
        out = np.empty(img.shape, np.uint8)
        self._check(self.lib.vfsms_enhance_u8(self.ctx, _ptr(img), img.shape[0], img.shape[1], img.strides[0], int(mode), float(clip_limit),
                                              int(tile_size), _ptr(out)))
        return out

    def attempt_phase_batch(self, jobs):
        n = len(jobs)
        out = np.zeros((n, 3), np.float64)
        if n == 0:
            return out
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        self._check(self.lib.vfsms_attempt_phase_batch(self.ctx, arr, n, _ptr(out)))
        return out

    # -- canvas ----------------------------------------------------------------------------------------------------
    # How a tile goes onto the canvas: fuseMethod -> the `mode` of a geometry row (vfsms_canvas_mode in include/vfsms.h; 5 is not a mode).
    # The per-tile calls keep their older arguments: `method` 0..3 of canvas_fuse_tile*, `mode` 0..2 of canvas_blend_tile*.
    CANVAS_MODES = {"notFuse": -1, "fadeInAndFadeOut": 0, "trigonometric": 1, "average": 2, "maximum": 3, "minimum": 4,
                    "multiBandBlending": 6, "optimalSeamLine": 7}
    CANVAS_FUSE_METHODS = {0: 0, 1: 1, 6: 2, 7: 3}       # row mode -> method
    CANVAS_BLEND_MODES = {2: 0, 3: 1, 4: 2}              # row mode -> blend mode

    def canvas_create(self, rows, cols, ch):
        h = C.c_int64()
        self._check(self.lib.vfsms_canvas_create(self.ctx, int(rows), int(cols), int(ch), C.byref(h)))
        return h.value

    def canvas_free(self, handle):
        self._check(self.lib.vfsms_canvas_free(self.ctx, C.c_int64(handle)))

    def canvas_paste(self, handle, tile, y0, x0):
        tile = np.ascontiguousarray(tile, np.uint8)
        self._check(self.lib.vfsms_canvas_paste(self.ctx, C.c_int64(handle), _ptr(tile), tile.shape[0], tile.shape[1], int(y0), int(x0)))

    def canvas_fuse_tile(self, handle, tile, y0, x0, roi, dx, dy, method=0):
        """method 0: fadeInAndFadeOut, 1: trigonometric, 2: multiBandBlending (levels: canvas_set_multiband_levels), 3: optimalSeamLine (blend:
        canvas_set_seam_blend)"""
        tile = np.ascontiguousarray(tile, np.uint8)
        info = np.zeros(4, np.int32)
        ry0, rx0, ry1, rx1 = [int(v) for v in roi]
        self._check(self.lib.vfsms_canvas_fuse_tile_m(self.ctx, C.c_int64(handle), _ptr(tile), tile.shape[0], tile.shape[1],
                                                      int(y0), int(x0), ry0, rx0, ry1, rx1, int(dx), int(dy), int(method), _ptr(info)))
        return info

    def canvas_blend_tile(self, handle, tile, y0, x0, roi, mode):
        """fuseMethod average / maximum / minimum (mode 0 / 1 / 2) of a host tile into the canvas."""
        tile = np.ascontiguousarray(tile, np.uint8)
        ry0, rx0, ry1, rx1 = [int(v) for v in roi]
        self._check(self.lib.vfsms_canvas_blend_tile(self.ctx, C.c_int64(handle), _ptr(tile), tile.shape[0], tile.shape[1],
                                                     int(y0), int(x0), ry0, rx0, ry1, rx1, int(mode)))

    def canvas_blend_tile_resident(self, handle, tile_handle, y0, x0, roi, mode):
        """canvas_blend_tile with a tile that is already resident; enqueue only"""
        ry0, rx0, ry1, rx1 = [int(v) for v in roi]
        self._check(self.lib.vfsms_canvas_blend_tile_resident(self.ctx, C.c_int64(handle), C.c_int64(tile_handle), int(y0), int(x0),
                                                              ry0, rx0, ry1, rx1, int(mode)))

    def canvas_paste_tile(self, handle, tile_handle, y0, x0):
        """paste of a single-channel tile that is already resident in HBM (tile_upload handle)."""
        self._check(self.lib.vfsms_canvas_paste_tile(self.ctx, C.c_int64(handle), C.c_int64(tile_handle), int(y0), int(x0)))

    def canvas_fuse_tile_resident(self, handle, tile_handle, y0, x0, roi, dx, dy, want_info=False, method=0):
        """want_info=False: the call only enqueues work; geometry errors surface in canvas_download.  method 0: fadeInAndFadeOut, 1: trigonometric,
        2: multiBandBlending, 3: optimalSeamLine"""
        info = np.zeros(4, np.int32) if want_info else None
        ry0, rx0, ry1, rx1 = [int(v) for v in roi]
        self._check(self.lib.vfsms_canvas_fuse_tile_resident_m(self.ctx, C.c_int64(handle), C.c_int64(tile_handle), int(y0), int(x0),
                                                               ry0, rx0, ry1, rx1, int(dx), int(dy), int(method), _ptr(info) if want_info else None))
        return info

    def canvas_assemble_resident(self, handle, tile_handles, geom):
        """The mosaic walk over resident tiles as one call.  geom: int32 [n][9] = y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode (mode: a value of
        CANVAS_MODES; Stitcher._placements builds the rows).  Enqueue only: geometry errors surface in canvas_download."""
        th = np.ascontiguousarray(tile_handles, np.int64)
        g = np.ascontiguousarray(geom, np.int32).reshape(-1, 9)
        if len(th) != len(g):
            raise ValueError("canvas_assemble_resident: one geometry row per tile")
        self._check(self.lib.vfsms_canvas_assemble_resident(self.ctx, C.c_int64(handle), len(th), _ptr(th), _ptr(g)))

    def canvas_set_multiband_levels(self, handle, levels):
        """pyramid levels (1..8) of the canvas's multiBandBlending fuses (default 4)"""
        self._check(self.lib.vfsms_canvas_set_multiband_levels(self.ctx, C.c_int64(handle), int(levels)))

    def canvas_set_seam_blend(self, handle, blend):
        """how the canvas's optimalSeamLine fuses merge the seam's two sides: "none" (default) or "multiBandBlending" (levels:
        canvas_set_multiband_levels)"""
        if blend not in self.SEAM_BLENDS:
            raise ValueError("seamLineBlend must be 'none' or 'multiBandBlending'")
        self._check(self.lib.vfsms_canvas_set_seam_blend(self.ctx, C.c_int64(handle), self.SEAM_BLENDS[blend]))

    # -- shading correction (tests/shading_ref.py is the specification) -----------------------------------------------------
    def shading_estimate(self, handles, percentile=50, radius=32):
        """A shading field from resident tiles of one shape (vfsms_shading_estimate): the `percentile` order statistic over the stack,
        smoothed by two box passes of `radius`, as a Q12 gain -> field handle (shading_apply, shading_download, shading_free)."""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        f = C.c_int64()
        self._check(self.lib.vfsms_shading_estimate(self.ctx, len(th), _ptr(th), int(percentile), int(radius), C.byref(f)))
        shapes = self.__dict__.setdefault("_shapes", {})
        shapes[("field", f.value)] = shapes.get(("tile", int(th[0])))
        return f.value

    def shading_from_gain(self, gain):
        """A field from a gain measured elsewhere (a blank-slide image): uint16 Q12 of shape (h, w) or (h, w, ch)."""
        gain = np.asarray(gain)
        if gain.dtype != np.uint16 or gain.ndim not in (2, 3):
            raise ValueError("shading_from_gain takes a uint16 (h, w) or (h, w, ch) array, got %s %s" % (gain.dtype, gain.shape))
        gain = np.ascontiguousarray(gain)
        f = C.c_int64()
        self._check(self.lib.vfsms_shading_from_gain(self.ctx, _ptr(gain), gain.shape[0], gain.shape[1], gain.shape[2] if gain.ndim == 3 else 1,
                                                     C.byref(f)))
        self.__dict__.setdefault("_shapes", {})[("field", f.value)] = gain.shape
        return f.value

    def shading_download(self, field, with_profile=False):
        """-> gain (uint16 Q12), or with_profile: (gain, smoothed Q8 field uint16, profile uint8), each of the tile shape; the last two are
        zeros for a field from shading_from_gain."""
        shape = self.__dict__.get("_shapes", {}).get(("field", field))
        if shape is None:
            raise ValueError("shading_download: not a field of this engine's shading_estimate / shading_from_gain")
        gain = np.empty(shape, np.uint16)
        q8 = np.empty(shape, np.uint16) if with_profile else None
        prof = np.empty(shape, np.uint8) if with_profile else None
        self._check(self.lib.vfsms_shading_download(self.ctx, C.c_int64(field), _ptr(gain), _ptr(q8), _ptr(prof)))
        return (gain, q8, prof) if with_profile else gain

    def shading_apply(self, field, handles):
        """the tiles corrected in place by the field's gain (vfsms_shading_apply); owned tiles of the field's shape, each named once"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        self._check(self.lib.vfsms_shading_apply(self.ctx, C.c_int64(field), len(th), _ptr(th)))

    def shading_free(self, field):
        self._check(self.lib.vfsms_shading_free(self.ctx, C.c_int64(field)))
        self.__dict__.get("_shapes", {}).pop(("field", field), None)

    # -- focus stacking (tests/focus_ref.py is the specification) --------------------------------------------------------------
    FOCUS_MODES = {"pixel": 0, "plane": 1}

    def focus_stack(self, handles, mode="pixel", radius=4, median=1, want_tile=False):
        """A focus series fused into one tile (vfsms_focus_stack): 2..64 resident planes of one shape, gray or B G R.  mode "pixel": per
        pixel the plane whose sum-modified Laplacian, summed over (2 radius + 1)^2, is largest (the lowest index on a tie), the index map
        cleaned by one 3 x 3 median when `median`; mode "plane": the whole plane of the largest score.  -> (out, D, S): out the fused
        array of the planes' shape, or with want_tile the handle of a NEW resident tile (tile_free); D uint8 (h, w) the plane index per
        pixel; S int64 [n] the per-plane scores.  The planes are only read."""
        if mode not in self.FOCUS_MODES:
            raise ValueError("focus_stack: mode must be 'pixel' or 'plane', got %r" % (mode,))
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        shape = self.__dict__.get("_shapes", {}).get(("tile", int(th[0]))) if len(th) else None
        if shape is None:                                     # no plane, or not a tile of this engine: the library's refusal says which
            self._check(self.lib.vfsms_focus_stack(self.ctx, len(th), _ptr(th), self.FOCUS_MODES[mode], int(radius), int(median), None, None, None, None))
            raise ValueError("focus_stack: the planes are tiles of this engine (tile_upload, tile_upload_color, tile_reserve, tile_wrap)")
        out = None if want_tile else np.empty(shape, np.uint8)
        D = np.empty(shape[:2], np.uint8)
        S = np.zeros(len(th), np.int64)
        tile = C.c_int64(0)
        self._check(self.lib.vfsms_focus_stack(self.ctx, len(th), _ptr(th), self.FOCUS_MODES[mode], int(radius), int(median),
                                               C.byref(tile) if want_tile else None, _ptr(out), _ptr(D), _ptr(S)))
        return (self._note_tile(tile.value, shape) if want_tile else out), D, S

    def focus_scores(self, handles):
        """vfsms_focus_scores: the sum of the sum-modified Laplacian over each of 1..4096 resident tiles (any shapes, gray or B G R)
        -> int64 [n] (tests/focus_ref.py: scores)"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        S = np.zeros(len(th), np.int64)
        self._check(self.lib.vfsms_focus_scores(self.ctx, len(th), _ptr(th), _ptr(S)))
        return S

    # -- 16-bit tiles (tests/deep_ref.py is the specification) ------------------------------------------------------------------
    DEEP_MODES = {"paste": 0, "notFuse": 0, "feather": 1}

    def deep_upload(self, img):
        """A 16-bit gray tile resident on the device (vfsms_deep_upload): a 2-D uint16 array, any row stride -> deep handle (deep_free).
        A handle kind of its own: only the deep_* methods take it."""
        img = np.asarray(img)
        if img.dtype != np.uint16 or img.ndim != 2:
            raise ValueError("deep_upload takes a 2-D uint16 array, got %s %s" % (img.dtype, img.shape))
        if (img.shape[1] > 1 and img.strides[1] != 2) or img.strides[0] < 2 * img.shape[1]:
            img = np.ascontiguousarray(img)
        h = C.c_int64()
        self._check(self.lib.vfsms_deep_upload(self.ctx, _ptr(img), img.shape[0], img.shape[1], img.strides[0], C.byref(h)))
        self.__dict__.setdefault("_shapes", {})[("deep", h.value)] = (int(img.shape[0]), int(img.shape[1]))
        return h.value

    def deep_free(self, handle):
        self._check(self.lib.vfsms_deep_free(self.ctx, C.c_int64(handle)))
        self.__dict__.get("_shapes", {}).pop(("deep", handle), None)

    def deep_window(self, handles, lo_ppm=1000, hi_ppm=999000):
        """vfsms_deep_window: the samples of rank (N - 1) * ppm // 10^6 among all samples of the deep tiles, exactly -> (lo, hi), lo < hi"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        win = np.zeros(2, np.int32)
        self._check(self.lib.vfsms_deep_window(self.ctx, len(th), _ptr(th), int(lo_ppm), int(hi_ppm), _ptr(win)))
        return int(win[0]), int(win[1])

    def deep_reduce(self, handles, lo, hi):
        """vfsms_deep_reduce: the 8-bit views of the deep tiles through the window (lo, hi) -> NEW ordinary gray tile handles (tile_free)"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        out = np.zeros(len(th), np.int64)
        self._check(self.lib.vfsms_deep_reduce(self.ctx, len(th), _ptr(th), int(lo), int(hi), _ptr(out)))
        shapes = self.__dict__.setdefault("_shapes", {})
        return [self._note_tile(int(t), shapes.get(("deep", int(d)), (0, 0))) for t, d in zip(out, th)]

    def deep_mosaic_rows(self, handles, yx, rows, cols, mode="feather", feather=0, row0=0, nrows=None, out=None):
        """vfsms_deep_mosaic_rows: rows [row0, row0 + nrows) of the rows x cols uint16 mosaic gathered from the deep tiles at yx (int [n][2],
        top-left corners) -> uint16 [nrows][cols].  mode "paste" / "notFuse" (the largest covering index) or "feather" (the mean weighted by
        the distance to each tile's border, cut at `feather` when positive); 0 / 1 as in include/vfsms.h.  Stateless: any band on demand."""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        at = np.ascontiguousarray(yx, np.int32).reshape(-1, 2)
        if len(at) != len(th):
            raise ValueError("deep_mosaic_rows: %d tiles, %d positions" % (len(th), len(at)))
        nrows = int(rows) - int(row0) if nrows is None else int(nrows)
        m = self.DEEP_MODES[mode] if isinstance(mode, str) else int(mode)
        if out is None:
            out = np.empty((max(nrows, 0), max(int(cols), 0)), np.uint16)
        self._check(self.lib.vfsms_deep_mosaic_rows(self.ctx, len(th), _ptr(th), _ptr(at), int(rows), int(cols), m, int(feather), int(row0), nrows, _ptr(out)))
        return out

    def deep_mosaic_bands(self, handles, yx, rows, cols, mode="feather", feather=0, band_rows=4096):
        """the whole mosaic as (row0, band) pairs of at most band_rows rows, one gather launch each"""
        for r0 in range(0, int(rows), int(band_rows)):
            yield r0, self.deep_mosaic_rows(handles, yx, rows, cols, mode, feather, r0, min(int(band_rows), int(rows) - r0))

    def deep_download(self, handle, out=None):
        """vfsms_deep_download: the samples of a deep tile -> uint16 (h, w); `out`: a uint16 array or view of that shape to fill (rows may
        be strided, samples adjacent)"""
        shape = self.__dict__.get("_shapes", {}).get(("deep", handle))
        if shape is None:
            raise ValueError("deep_download: not a deep tile of this engine's deep_upload")
        if out is None:
            out = np.empty(shape, np.uint16)
        if out.dtype != np.uint16 or out.shape != shape or (shape[1] > 1 and out.strides[1] != 2) or out.strides[0] < 2 * shape[1]:
            raise ValueError("deep_download: out must be a uint16 %s array with adjacent samples" % (shape,))
        self._check(self.lib.vfsms_deep_download(self.ctx, C.c_int64(handle), _ptr(out), out.strides[0]))
        return out

    # -- shading correction of 16-bit tiles (tests/deep_shading_ref.py is the specification) ---------------------------------------
    def deep_shading_estimate(self, handles, percentile=50, radius=32, pedestal=0):
        """A shading field from deep tiles of one shape (vfsms_deep_shading_estimate): the `percentile` order statistic over the stack, less
        the camera's dark level `pedestal`, smoothed by two box passes of `radius`, as a Q12 gain -> deep field handle
        (deep_shading_apply, deep_shading_download, deep_shading_free).  A handle kind of its own: the shading_* methods refuse it."""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        f = C.c_int64()
        self._check(self.lib.vfsms_deep_shading_estimate(self.ctx, len(th), _ptr(th), int(percentile), int(radius), int(pedestal), C.byref(f)))
        shapes = self.__dict__.setdefault("_shapes", {})
        shapes[("deep_field", f.value)] = shapes.get(("deep", int(th[0])))
        return f.value

    def deep_shading_from_gain(self, gain, pedestal=0):
        """A deep field from a gain measured elsewhere (a blank slide): uint16 Q12 of shape (h, w), and the pedestal of the tiles it corrects."""
        gain = np.asarray(gain)
        if gain.dtype != np.uint16 or gain.ndim != 2:
            raise ValueError("deep_shading_from_gain takes a uint16 (h, w) array, got %s %s" % (gain.dtype, gain.shape))
        gain = np.ascontiguousarray(gain)
        f = C.c_int64()
        self._check(self.lib.vfsms_deep_shading_from_gain(self.ctx, _ptr(gain), gain.shape[0], gain.shape[1], int(pedestal), C.byref(f)))
        self.__dict__.setdefault("_shapes", {})[("deep_field", f.value)] = gain.shape
        return f.value

    def deep_shading_download(self, field):
        """-> (gain uint16 Q12, smoothed field uint16, profile uint16, pedestal), the planes of the tile shape; smooth and profile are zeros
        for a field from deep_shading_from_gain."""
        shape = self.__dict__.get("_shapes", {}).get(("deep_field", field))
        if shape is None:
            raise ValueError("deep_shading_download: not a field of this engine's deep_shading_estimate / deep_shading_from_gain")
        gain, smooth, prof = (np.empty(shape, np.uint16) for _ in range(3))
        ped = C.c_int32()
        self._check(self.lib.vfsms_deep_shading_download(self.ctx, C.c_int64(field), _ptr(gain), _ptr(smooth), _ptr(prof), C.byref(ped)))
        return gain, smooth, prof, int(ped.value)

    def deep_shading_apply(self, field, handles):
        """the deep tiles corrected in place by the field's gain above its pedestal (vfsms_deep_shading_apply); tiles of the field's shape,
        each named once"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        self._check(self.lib.vfsms_deep_shading_apply(self.ctx, C.c_int64(field), len(th), _ptr(th)))

    def deep_shading_free(self, field):
        self._check(self.lib.vfsms_deep_shading_free(self.ctx, C.c_int64(field)))
        self.__dict__.get("_shapes", {}).pop(("deep_field", field), None)

    # -- exposure compensation (tests/exposure_ref.py is the specification) -------------------------------------------------
    def overlap_stats_batch(self, jobs, lo, hi):
        """vfsms_overlap_stats_batch: jobs = sequence of (tile_a, tile_b, dx, dy) over resident tiles (gray or colour, one channel count
        per job, any shapes); tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy).  -> int64[n, 3] = (N, Sa, Sb) over the samples
        of the overlap with lo <= a <= hi and lo <= b <= hi"""
        n = len(jobs)
        out = np.zeros((n, 3), np.int64)
        arr = (NccJob * max(n, 1))()
        for k, j in enumerate(jobs):
            arr[k] = NccJob(*[int(v) for v in j])
        self._check(self.lib.vfsms_overlap_stats_batch(self.ctx, arr, n, int(lo), int(hi), _ptr(out)))
        return out

    def exposure_apply(self, handles, gains):
        """the tiles corrected in place, tile i by the Q12 gain gains[i] (vfsms_exposure_apply): out = min(255, (p * Q + 2048) >> 12);
        owned tiles, each named once; a tile whose gain is 4096 is left alone"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        g = np.asarray(gains).reshape(-1)
        if len(g) != len(th) or (len(g) and (g.min() < 0 or g.max() > 65535)):
            raise ValueError("exposure_apply: one Q12 gain in 0..65535 per tile")
        g = np.ascontiguousarray(g, np.uint16)
        self._check(self.lib.vfsms_exposure_apply(self.ctx, len(th), _ptr(th), _ptr(g)))

    # -- lens correction (tests/lens_ref.py is the specification) -------------------------------------------------------------
    LENS_INTERPOLATIONS = {"bilinear": 0, "cubic": 1}

    def block_ncc_batch(self, jobs, first, block, radius, want_surface=False):
        """vfsms_block_ncc_batch: jobs = sequence of (tile_a, tile_b, dx, dy) over resident tiles, both of a job of one shape and channel
        count (gray or B G R); first = int64 [n + 1], the index of every job's first block and the total (lens.block_first): the library
        checks it against the lattice.  Every block x block square of the overlap shrunk by `radius` (block 8..128 in multiples of 8,
        radius 1..16) is scored at every (i, j) in [-radius, radius]^2 as verify_ncc scores an overlap.
        -> int32[blocks, 4] = (i, j, fixed-point score, block^2) of the best candidate per block [, int32[blocks, 2 radius + 1,
        2 radius + 1], the fixed-point score of every candidate, with want_surface]"""
        n = len(jobs)
        first = np.ascontiguousarray(first, np.int64).reshape(-1)
        if len(first) != n + 1:
            raise ValueError("block_ncc_batch: %d jobs need %d entries of first, got %d" % (n, n + 1, len(first)))
        total = max(int(first[-1]), 0)
        side = 2 * int(radius) + 1
        best = np.zeros((total, 4), np.int32)
        surface = np.zeros((total, side, side), np.int32) if want_surface else None
        self._check(self.lib.vfsms_block_ncc_batch(self.ctx, self._ncc_jobs(jobs), n, int(block), int(radius), _ptr(first), _ptr(best),
                                                   _ptr(surface)))
        return (best, surface) if want_surface else best

    def lens_apply(self, handles, a1_q30, a2_q30, centre2=(-1, -1), interpolation="cubic"):
        """the tiles resampled in place under the radial map of tests/lens_ref.py (vfsms_lens_apply): Q30 coefficients, the centre in
        half pixels (a coordinate below 0: every tile's own middle); owned tiles of any shapes, each named once"""
        th = np.ascontiguousarray(handles, np.int64).reshape(-1)
        self._check(self.lib.vfsms_lens_apply(self.ctx, len(th), _ptr(th), int(a1_q30), int(a2_q30), int(centre2[0]), int(centre2[1]),
                                              self._lens_interp(interpolation)))

    def lens_remap(self, img, a1_q30, a2_q30, centre2=(-1, -1), interpolation="cubic"):
        """vfsms_lens_remap_u8: the same map for a host array, (h, w) or (h, w, ch) uint8 with any row stride -> a new array"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3):
            raise ValueError("lens_remap takes an (h, w) or (h, w, ch) uint8 array, got %s %s" % (img.dtype, img.shape))
        ch = img.shape[2] if img.ndim == 3 else 1
        if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != ch) or img.strides[0] < img.shape[1] * ch:
            img = np.ascontiguousarray(img)
        out = np.empty(img.shape, np.uint8)
        self._check(self.lib.vfsms_lens_remap_u8(self.ctx, _ptr(img), img.shape[0], img.shape[1], ch, img.strides[0], int(a1_q30), int(a2_q30),
                                                 int(centre2[0]), int(centre2[1]), self._lens_interp(interpolation), _ptr(out)))
        return out

    def _lens_interp(self, interpolation):
        if isinstance(interpolation, str):
            if interpolation not in self.LENS_INTERPOLATIONS:
                raise ValueError("interpolation must be 'bilinear' or 'cubic', got %r" % (interpolation,))
            return self.LENS_INTERPOLATIONS[interpolation]
        return int(interpolation)                             # (a number goes to the library as it is: its refusal says what it takes)

    def canvas_download(self, handle, rows, cols, ch):
        out = np.empty((rows, cols, ch) if ch > 1 else (rows, cols), np.uint8)
        self._check(self.lib.vfsms_canvas_download(self.ctx, C.c_int64(handle), _ptr(out)))
        return out

    def canvas_download_rows(self, handle, row0, nrows, cols, ch, out=None):
        """Rows [row0, row0 + nrows) of the mosaic (vfsms_canvas_download_rows); `out` may be a preallocated band buffer."""
        shape = (nrows, cols, ch) if ch > 1 else (nrows, cols)
        if out is None:
            out = np.empty(shape, np.uint8)
        if out.shape != shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("canvas_download_rows: `out` must be a C-contiguous u8 array of shape %r" % (shape,))
        self._check(self.lib.vfsms_canvas_download_rows(self.ctx, C.c_int64(handle), int(row0), int(nrows), _ptr(out)))
        return out

    BAND_RING = 3

    # ---- the band walk of the four write-out routes: the walk itself, the ring of pinned buffers the bands land in, the one retry -----
    @staticmethod
    def _bands(rows, band_rows):
        """(k, row0, nrows) of every band of `band_rows` rows over `rows` rows"""
        for k, r0 in enumerate(range(0, rows, band_rows)):
            yield k, r0, min(band_rows, rows - r0)

    def _ring(self, name, need):
        """the ring `name` of BAND_RING pinned u8 buffers kept by the engine, every slot of at least `need` bytes: a slot that is smaller
        is replaced (outgrown buffers stay valid: they are freed with the engine)"""
        ring = self.__dict__.setdefault(name, [None] * self.BAND_RING)
        for j in range(self.BAND_RING):
            if ring[j] is None or ring[j].size < need:
                ring[j] = self.pinned_empty((need,))
        return ring

    def _encode_ring(self, need=0):
        """the ring of the two encode routes: 64 KiB a slot at first, then a band's answer `need` with room for denser bands"""
        return self._ring("_jpeg_ring", need + need // 4 + (1 << 16))

    def _capacity_or(self, rc):
        """rc, with every error but VFSMS_ERR_CAPACITY raised: that one means nothing was written -- call again with room"""
        if rc != VFSMS_ERR_CAPACITY:
            self._check(rc)
        return rc

    def _fitted(self, who, what, call, buf, grown):
        """call(buf) -> (return code, bytes needed, ...) as _capacity_or leaves it.  On VFSMS_ERR_CAPACITY once more, with the buffer
        grown(bytes needed, ...) gives -> (the buffer that held the result, bytes needed, ...)"""
        ans = call(buf)
        if ans[0] == VFSMS_ERR_CAPACITY:
            buf = grown(*ans[1:])
            ans = call(buf)
            if ans[0] != VFSMS_OK:
                raise VfsmsError("%s: the %s did not fit the size the library asked for" % (who, what))
        return (buf,) + tuple(ans[1:])

    @staticmethod
    def _u8_image(img, who):
        """a u8 (h, w) or (h, w, ch) array whose rows are contiguous (they may be strided) -> (img, h, w, ch)"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != img.shape[2]) or img.strides[0] < 0:
            raise ValueError("%s: a u8 (h, w) or (h, w, ch) array whose rows are contiguous" % who)
        return img, img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2]

    def canvas_download_bands(self, handle, rows, cols, ch, band_rows=4096, transient=False):
        """Generator of (row0, band) over the whole mosaic, `band_rows` rows at a time (streamed write-out of large mosaics).  With
        `transient` the bands are views of a ring of BAND_RING pinned buffers kept by the engine (the copy is a DMA at link speed, no
        page faults of a fresh array per band): a band is valid until BAND_RING - 1 further bands have been requested -- for consumers
        that are done with a band by then (JpegBandWriter declares it: `transient_bands`)."""
        ring = self._ring("_band_ring", min(band_rows, rows) * cols * ch) if transient else None
        for k, r0, n in self._bands(rows, band_rows):
            out = ring[k % self.BAND_RING][:n * cols * ch].reshape((n, cols, ch) if ch > 1 else (n, cols)) if transient else None
            yield r0, self.canvas_download_rows(handle, r0, n, cols, ch, out=out)

    @staticmethod
    def pyramid_band_shapes(row0, nrows, cols, ch, levels):
        """shapes of levels 1 .. levels of the band [row0, row0 + nrows) as vfsms_canvas_download_rows_pyramid lays them out"""
        shapes, c = [], cols
        for k in range(1, levels + 1):
            c = (c + 1) >> 1
            n = ((row0 + nrows + (1 << k) - 1) >> k) - (row0 >> k)
            shapes.append((n, c, ch) if ch > 1 else (n, c))
        return shapes

    def _pyramid_rows(self, handle, row0, nrows, cols, ch, levels, band, buf):
        """one vfsms_canvas_download_rows_pyramid call: rows into `band` (None: levels only), the levels into the u8 vector `buf` -> views"""
        self._check(self.lib.vfsms_canvas_download_rows_pyramid(self.ctx, C.c_int64(handle), int(row0), int(nrows), int(levels),
                                                                _ptr(band), _ptr(buf), C.c_size_t(buf.size)))
        out, off = [], 0
        for shape in self.pyramid_band_shapes(row0, nrows, cols, ch, levels):
            n = int(np.prod(shape))
            out.append(buf[off:off + n].reshape(shape)); off += n
        return out

    def canvas_pyramid(self, handle, rows, cols, ch, levels):
        """levels 1 .. levels of the whole mosaic (tests/pyramid_ref.py: pyramid_levels of canvas_download), formed on the device in one
        call over all rows; level 0 is not downloaded."""
        if not 1 <= int(levels) <= 10:
            raise ValueError("canvas_pyramid: levels must be 1..10")
        need = sum(int(np.prod(s_)) for s_ in self.pyramid_band_shapes(0, rows, cols, ch, int(levels)))
        return self._pyramid_rows(handle, 0, rows, cols, ch, int(levels), None, np.empty(need, np.uint8))

    def canvas_download_pyramid_bands(self, handle, rows, cols, ch, levels, band_rows=4096, transient=False):
        """Generator of (row0, band, [level-1 rows, ..., level-`levels` rows]) over the whole mosaic: canvas_download_bands plus the reduced
        levels of every band, formed on the device while the band is in HBM anyway (vfsms_canvas_download_rows_pyramid).  band_rows must be
        a multiple of 2^levels, so that every band forms complete level rows.  With `transient` band and levels are views of ONE slot of the
        ring of BAND_RING pinned buffers and valid as long as a band of canvas_download_bands is."""
        levels, band_rows = int(levels), int(band_rows)
        if not 1 <= levels <= 10:
            raise ValueError("canvas_download_pyramid_bands: levels must be 1..10")
        if band_rows <= 0 or band_rows % (1 << levels):
            raise ValueError("canvas_download_pyramid_bands: band_rows = %d is not a multiple of 2^levels = %d" % (band_rows, 1 << levels))
        shape = lambda n: (n, cols, ch) if ch > 1 else (n, cols)
        nb0 = min(band_rows, rows) * cols * ch
        need = nb0 + sum(int(np.prod(s_)) for s_ in self.pyramid_band_shapes(0, min(band_rows, rows), cols, ch, levels))
        ring = self._ring("_band_ring", need) if transient else None
        for k, r0, n in self._bands(rows, band_rows):
            slot = ring[k % self.BAND_RING] if transient else np.empty(need, np.uint8)
            band = slot[:n * cols * ch].reshape(shape(n))
            yield r0, band, self._pyramid_rows(handle, r0, n, cols, ch, levels, band, slot[nb0:])

    def jpeg_encode_device(self, img, bgr=True, quality=95, restart_mcus=0):
        """vfsms_jpeg_encode_device: u8 (h, w) or (h, w, 3) rows (B G R when `bgr`; rows may be strided) -> a complete baseline JPEG as a u8
        array, encoded on the device: the bytes of tests/jpeg_enc_ref.py's encode(), which at restart_mcus = 0 (the image is one restart
        interval: at most 65535 MCUs) are libjpeg's.  restart_mcus = R: a restart interval of R MCUs."""
        img, h, w, ch = self._u8_image(img, "jpeg_encode_device")
        n = C.c_size_t()
        call = lambda out: (self._capacity_or(self.lib.vfsms_jpeg_encode_device(
            self.ctx, img.ctypes.data_as(C.c_void_p), h, w, ch, img.strides[0], int(bool(bgr)), int(quality), int(restart_mcus), _ptr(out), out.size, C.byref(n))), n.value)
        out, size = self._fitted("jpeg_encode_device", "stream", call, np.empty(max(1 << 16, h * w * ch // 4), np.uint8), lambda need: np.empty(need, np.uint8))
        return out[:size]

    def canvas_encode_jpeg_rows(self, handle, row0, nrows, quality, restart_mcus, out):
        """one vfsms_canvas_encode_jpeg_rows call into the u8 vector `out` -> (return code, bytes needed); VFSMS_ERR_CAPACITY is returned, not
        raised (nothing was written: call again with room), any other error raises"""
        n = C.c_size_t()
        rc = self.lib.vfsms_canvas_encode_jpeg_rows(self.ctx, C.c_int64(handle), int(row0), int(nrows), int(quality), int(restart_mcus),
                                                    _ptr(out), C.c_size_t(out.size), C.byref(n))
        return self._capacity_or(rc), n.value

    def _encode_bands(self, who, rows, band_rows, call, regrow=lambda *more: None):
        """The band loop of the four encode routes: generator of (row0, nrows, bytes-view, ...) with call(row0, nrows, out) -> (return code,
        bytes needed, ...), the route's *_rows method.  Band k goes into slot k % BAND_RING of the encode ring; one that does not fit comes
        again in the ring regrown to its answer, behind regrow(the answers beyond the bytes)"""
        for k, r0, n in self._bands(rows, band_rows):
            slot = k % self.BAND_RING
            ans = self._fitted(who, "band", lambda out: call(r0, n, out), self._encode_ring()[slot],
                               lambda need, *more: (regrow(*more), self._encode_ring(need)[slot])[1])
            yield (r0, n, ans[0][:ans[1]]) + ans[2:]

    def canvas_encode_jpeg_bands(self, handle, rows, cols, ch, quality, restart_mcus, band_rows):
        """Generator of (row0, nrows, bytes-view) over the whole mosaic: every band of `band_rows` rows as the entropy-coded bytes of a
        baseline JPEG (vfsms_canvas_encode_jpeg_rows), encoded on the device -- behind jpeg_header(...) and in front of FF D9 they are the
        file (imagestitch_amd.io.DeviceJpegFile).  band_rows must keep the band contract: a multiple of the MCU height (16 colour, 8 gray)
        whose MCUs are a multiple of restart_mcus.  The views belong to a ring of BAND_RING pinned buffers, sized from the first band's
        answer with room to spare and regrown when a later band needs more; a view is valid until BAND_RING - 1 further bands were asked for."""
        rows, cols, ch, band_rows = int(rows), int(cols), int(ch), int(band_rows)
        if band_rows <= 0:
            raise ValueError("canvas_encode_jpeg_bands: band_rows must be positive")
        yield from self._encode_bands("canvas_encode_jpeg_bands", rows, band_rows, lambda r0, n, out: self.canvas_encode_jpeg_rows(handle, r0, n, quality, restart_mcus, out))

    def _encode_tiles_device(self, who, entry, img, tile, bgr, first_guess, *coder_args):
        """the image-order tile operators: entry(ctx, image, bgr, tile, *coder_args, out, ...) -> (payload u8, offsets uint64 [n_tiles + 1]);
        the payload's first buffer is 64 KiB or the image's bytes over `first_guess`, whichever is more"""
        img, h, w, ch = self._u8_image(img, who)
        T = max(int(tile), 1)
        offsets = np.zeros(-(-h // T) * -(-w // T) + 1, np.uint64)
        n = C.c_size_t()
        call = lambda out: (self._capacity_or(entry(
            self.ctx, img.ctypes.data_as(C.c_void_p), h, w, ch, img.strides[0], int(bool(bgr)), int(tile), *(int(a) for a in coder_args),
            _ptr(out), out.size, C.byref(n), _ptr(offsets), offsets.size)), n.value)
        out, size = self._fitted(who, "tiles", call, np.empty(max(1 << 16, h * w * ch // first_guess), np.uint8), lambda need: np.empty(need, np.uint8))
        return out[:size], offsets

    def jpeg_encode_tiles_device(self, img, tile, bgr=True, quality=95, restart_mcus=0):
        """vfsms_jpeg_encode_tiles_device, the bare operator: u8 (h, w) or (h, w, 3) rows (B G R when `bgr`; rows may be strided) -> (payload u8,
        offsets uint64 [n_tiles + 1]): the abbreviated JPEG streams of the image's tile x tile tiles, row-major and back to back -- level 0 of
        tests/tiff_jpeg_ref.py's file_tiles.  Tile t is payload[offsets[t]:offsets[t + 1]]."""
        return self._encode_tiles_device("jpeg_encode_tiles_device", self.lib.vfsms_jpeg_encode_tiles_device, img, tile, bgr, 4, quality, restart_mcus)

    @staticmethod
    def pyramid_tiles_index(rows, cols, levels, tile, row0, nrows):
        """the (level, tile number in the level) pairs whose streams the band [row0, row0 + nrows) of a rows x cols mosaic completes, in the
        order vfsms_canvas_encode_pyramid_tiles returns them (level after level, a level's tiles row-major): level k's tile rows from the
        one row0 >> k lies in up to the last one that ceil((row0 + nrows) / 2^k) rows fill -- every remaining one when the band ends at the
        last row (tests/pyramid_ref.py: band_of_level)"""
        out, last = [], row0 + nrows >= rows
        r, c = int(rows), int(cols)
        for k in range(int(levels) + 1):
            ntx = -(-c // tile)
            first = (row0 >> k) // tile
            end = -(-r // tile) if last else ((row0 + nrows + (1 << k) - 1) >> k) // tile
            out += [(k, t) for t in range(first * ntx, end * ntx)]
            r, c = (r + 1) >> 1, (c + 1) >> 1
        return out

    def canvas_encode_pyramid_tiles_rows(self, handle, row0, nrows, levels, tile, quality, restart_mcus, out, index):
        """one vfsms_canvas_encode_pyramid_tiles call into the u8 vector `out` and the int64 (n, 4) array `index` -> (return code, bytes
        needed, records needed); VFSMS_ERR_CAPACITY is returned, not raised (nothing was written or consumed: call again with room)"""
        n, ni = C.c_size_t(), C.c_int()
        rc = self.lib.vfsms_canvas_encode_pyramid_tiles(self.ctx, C.c_int64(handle), int(row0), int(nrows), int(levels), int(tile), int(quality),
                                                        int(restart_mcus), _ptr(out), C.c_size_t(out.size), C.byref(n), _ptr(index), len(index), C.byref(ni))
        return self._capacity_or(rc), n.value, ni.value

    def canvas_encode_pyramid_tiles(self, handle, rows, cols, ch, levels, tile, quality, restart_mcus, band_rows):
        """Generator of (row0, nrows, bytes-view, index) over the whole mosaic: of every band of `band_rows` rows the finished JPEG tile
        streams of level 0 and of reduced levels 1 .. levels that the band completes (vfsms_canvas_encode_pyramid_tiles: levels formed,
        carried and encoded on the device), and int64 records (level, tile number, offset in the view, bytes) in the view's order -- what
        PyramidTiffBandWriter(compression="jpeg").tiles takes.  band_rows must be a multiple of the tile and of 2^levels.  The views belong
        to a ring of BAND_RING pinned buffers, regrown when a band needs more; a view is valid until BAND_RING - 1 further bands were asked for."""
        rows, cols, ch, levels, tile, band_rows = int(rows), int(cols), int(ch), int(levels), int(tile), int(band_rows)
        if tile <= 0 or band_rows <= 0 or band_rows % tile or band_rows % (1 << levels):
            raise ValueError("canvas_encode_pyramid_tiles: band_rows = %d is not a positive multiple of the tile = %d and of 2^levels = %d" % (band_rows, tile, 1 << levels))
        yield from self._pyramid_tile_bands("canvas_encode_pyramid_tiles", self.canvas_encode_pyramid_tiles_rows, handle, rows, cols, levels, tile, band_rows,
                                            quality, restart_mcus)

    def _pyramid_tile_bands(self, who, rows_method, handle, rows, cols, levels, tile, band_rows, *coder_args):
        """the bands of a tile route over rows_method(handle, row0, nrows, levels, tile, *coder_args, out, index), one of the two *_rows
        methods.  Every band gets an index array of its own, sized by pyramid_tiles_index, or at the library's count should the band not fit"""
        index = [None]

        def call(r0, n, out):
            if index[0] is None:
                index[0] = np.empty((len(self.pyramid_tiles_index(rows, cols, levels, tile, r0, n)), 4), np.int64)
            return rows_method(handle, r0, n, levels, tile, *coder_args, out, index[0])
        for r0, n, view, ni in self._encode_bands(who, rows, band_rows, call, lambda ni: index.__setitem__(0, np.empty((ni, 4), np.int64))):
            yield r0, n, view, index[0][:ni]
            index[0] = None

    def deflate_encode_tiles_device(self, img, tile, bgr=True):
        """vfsms_deflate_encode_tiles_device, the bare operator: u8 (h, w) or (h, w, 3) rows (B G R when `bgr`; rows may be strided) -> (payload
        u8, offsets uint64 [n_tiles + 1]): the zlib streams (TIFF predictor 2, colour stored R G B, zero padding) of the image's tile x tile
        tiles, row-major and back to back -- tests/deflate_ref.py's tile_streams.  Tile t is payload[offsets[t]:offsets[t + 1]]."""
        return self._encode_tiles_device("deflate_encode_tiles_device", self.lib.vfsms_deflate_encode_tiles_device, img, tile, bgr, 1)

    def canvas_encode_pyramid_tiles_deflate_rows(self, handle, row0, nrows, levels, tile, out, index):
        """one vfsms_canvas_encode_pyramid_tiles_deflate call into the u8 vector `out` and the int64 (n, 4) array `index` -> (return code, bytes
        needed, records needed); VFSMS_ERR_CAPACITY is returned, not raised (nothing was written or consumed: call again with room)"""
        n, ni = C.c_size_t(), C.c_int()
        rc = self.lib.vfsms_canvas_encode_pyramid_tiles_deflate(self.ctx, C.c_int64(handle), int(row0), int(nrows), int(levels), int(tile),
                                                                _ptr(out), C.c_size_t(out.size), C.byref(n), _ptr(index), len(index), C.byref(ni))
        return self._capacity_or(rc), n.value, ni.value

    def canvas_encode_pyramid_tiles_deflate(self, handle, rows, cols, ch, levels, tile, band_rows):
        """Generator of (row0, nrows, bytes-view, index) over the whole mosaic, as canvas_encode_pyramid_tiles yields them, with the lossless
        coder (vfsms_canvas_encode_pyramid_tiles_deflate): the finished zlib tile streams of level 0 and of reduced levels 1 .. levels that
        every band completes -- what PyramidTiffBandWriter(compression="deflate-device").tiles takes.  band_rows must be a multiple of the
        tile and of 2^levels.  The views belong to the same ring of BAND_RING pinned buffers."""
        rows, cols, ch, levels, tile, band_rows = int(rows), int(cols), int(ch), int(levels), int(tile), int(band_rows)
        if tile <= 0 or band_rows <= 0 or band_rows % tile or band_rows % (1 << levels):
            raise ValueError("canvas_encode_pyramid_tiles_deflate: band_rows = %d is not a positive multiple of the tile = %d and of 2^levels = %d" % (band_rows, tile, 1 << levels))
        yield from self._pyramid_tile_bands("canvas_encode_pyramid_tiles_deflate", self.canvas_encode_pyramid_tiles_deflate_rows, handle, rows, cols, levels, tile, band_rows)

    def png_encode_device(self, img, segment_rows=16, bgr=True):
        """vfsms_png_encode_device, the bare operator: u8 (h, w) or (h, w, 3) rows (B G R when `bgr`; rows may be strided) -> (payload u8, the
        Adler-32 of the filtered bytes): the IDAT chunks of the image's segments of `segment_rows` rows, adaptively filtered and coded on the
        device, CRC-32 included -- tests/png_ref.py's device_payload and band_adler.  imagestitch_amd.io.DevicePngFile makes a file of them."""
        img, h, w, ch = self._u8_image(img, "png_encode_device")
        n, adler = C.c_size_t(), C.c_uint32()
        call = lambda out: (self._capacity_or(self.lib.vfsms_png_encode_device(
            self.ctx, img.ctypes.data_as(C.c_void_p), h, w, ch, img.strides[0], int(bool(bgr)), int(segment_rows),
            _ptr(out), out.size, C.byref(n), C.byref(adler))), n.value)
        out, size = self._fitted("png_encode_device", "chunks", call, np.empty(max(1 << 16, h * w * ch), np.uint8), lambda need: np.empty(need, np.uint8))
        return out[:size], adler.value

    def canvas_encode_png_rows(self, handle, row0, nrows, segment_rows, out):
        """one vfsms_canvas_encode_png_rows call into the u8 vector `out` -> (return code, bytes needed, the band's Adler-32);
        VFSMS_ERR_CAPACITY is returned, not raised (nothing was written: call again with room), any other error raises"""
        n, adler = C.c_size_t(), C.c_uint32()
        rc = self.lib.vfsms_canvas_encode_png_rows(self.ctx, C.c_int64(handle), int(row0), int(nrows), int(segment_rows),
                                                   _ptr(out), C.c_size_t(out.size), C.byref(n), C.byref(adler))
        return self._capacity_or(rc), n.value, adler.value

    def canvas_encode_png_bands(self, handle, rows, cols, ch, segment_rows, band_rows):
        """Generator of (row0, nrows, bytes-view, adler) over the whole mosaic: every band of `band_rows` rows as the IDAT chunks of its
        segments (vfsms_canvas_encode_png_rows), filtered, coded and checksummed on the device, with the Adler-32 of the band's filtered bytes
        -- what imagestitch_amd.io.DevicePngFile.append takes.  band_rows must be a multiple of segment_rows.  The views belong to the ring of
        BAND_RING pinned buffers of the encode routes; a view is valid until BAND_RING - 1 further bands were asked for."""
        rows, cols, ch, segment_rows, band_rows = int(rows), int(cols), int(ch), int(segment_rows), int(band_rows)
        if segment_rows <= 0 or band_rows <= 0 or band_rows % segment_rows:
            raise ValueError("canvas_encode_png_bands: band_rows = %d is not a positive multiple of segment_rows = %d" % (band_rows, segment_rows))
        yield from self._encode_bands("canvas_encode_png_bands", rows, band_rows, lambda r0, n, out: self.canvas_encode_png_rows(handle, r0, n, segment_rows, out))


_default_engine = None


def tiff_jpeg_tables(ch, quality=95):
    """vfsms_tiff_jpeg_tables: the JPEGTables datastream of a TIFF with device-encoded JPEG tiles (SOI, DQT .., DHT .., EOI:
    tests/tiff_jpeg_ref.py's tables), as bytes.  No GPU involved."""
    lib = load_library()
    out = np.empty(1024, np.uint8)
    n = C.c_size_t()
    rc = lib.vfsms_tiff_jpeg_tables(int(ch), int(quality), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if rc != VFSMS_OK:
        raise VfsmsError("libvfsms error %d: %s" % (rc, _last_error(lib)), code=int(rc))
    return out[:n.value].tobytes()


def jpeg_header(rows, cols, ch, quality=95, restart_mcus=0):
    """vfsms_jpeg_header: SOI .. the SOS header of a baseline JPEG in libjpeg's layout (with a DRI segment when restart_mcus > 0), as bytes:
    what goes in front of Engine.canvas_encode_jpeg_bands' payloads.  No GPU involved.  The refusals of tests/jpeg_enc_ref.py raise VfsmsError."""
    lib = load_library()
    out = np.empty(1024, np.uint8)
    n = C.c_size_t()
    rc = lib.vfsms_jpeg_header(int(rows), int(cols), int(ch), int(quality), int(restart_mcus), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if rc != VFSMS_OK:
        raise VfsmsError("libvfsms error %d: %s" % (rc, _last_error(lib)), code=int(rc))
    return out[:n.value].tobytes()


def jpeg_decode(data, want_planes=False):
    """vfsms_jpeg_decode: the library's own JPEG decode (system libjpeg-turbo), no GPU involved -> u8 (h, w) -- the grayscale decode -- or,
    with want_planes and a three-component file, u8 (h, w, 3) Y Cb Cr.  None when the library does not take the file (see tile_fill_jpeg)."""
    lib = load_library()
    h, w, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.vfsms_jpeg_decode(data, len(data), int(bool(want_planes)), None, 0, C.byref(h), C.byref(w), C.byref(c))
    if rc != VFSMS_ERR_CAPACITY:
        return None
    out = np.empty((h.value, w.value, c.value), np.uint8)
    rc = lib.vfsms_jpeg_decode(data, len(data), int(bool(want_planes)), out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(h), C.byref(w), C.byref(c))
    if rc != VFSMS_OK:
        return None
    return out[:, :, 0] if c.value == 1 else out


def jpeg_decode_raw420(data):
    """vfsms_jpeg_decode(want_planes = 2): the DOWNSAMPLED planes of a 4:2:0 Y Cb Cr file as the entropy decode + IDCT leave them (what
    vfsms_tile_fill_jpeg stages for the device's upsampler) -> (Y u8 (ph, pw), Cb u8 (ph / 2, pw / 2), Cr, h, w) on the iMCU grid (pw, ph =
    w, h rounded up to 16), or None when the file is not 4:2:0 / not taken."""
    lib = load_library()
    h, w, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.vfsms_jpeg_decode(data, len(data), 2, None, 0, C.byref(h), C.byref(w), C.byref(c))
    if rc != VFSMS_ERR_CAPACITY:
        return None
    pw, ph = (w.value + 15) & ~15, (h.value + 15) & ~15
    out = np.empty(pw * ph * 3 // 2, np.uint8)
    rc = lib.vfsms_jpeg_decode(data, len(data), 2, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(h), C.byref(w), C.byref(c))
    if rc != VFSMS_OK:
        return None
    n = pw * ph
    return out[:n].reshape(ph, pw), out[n:n + n // 4].reshape(ph // 2, pw // 2), out[n + n // 4:].reshape(ph // 2, pw // 2), h.value, w.value


def _coefficient_layout(out, n, grid):
    """the bytes of vfsms_jpeg_coefficients' layout -> [(coef int16 (block_rows, block_cols, 64), quant uint16 (64,))] per component"""
    comps, off = [], 128 * n
    for k in range(n):
        br, bc = grid[2 * k], grid[2 * k + 1]
        nb = br * bc * 128
        comps.append((out[off:off + nb].view(np.int16).reshape(br, bc, 64), out[128 * k:128 * (k + 1)].view(np.uint16)))
        off += nb
    return comps


SCAN_HEADER_FIELDS = ("h", "w", "ncomp", "grid0", "grid1", "grid2", "grid3", "grid4", "grid5", "restart_interval", "nseg", "nsub", "mcus",
                      "blocks_per_mcu", "sub_bits", "stream_bytes", "off_quant", "off_tables", "off_stream", "off_seg", "off_subseg", "total_bytes")
HUFF_TABLE_BYTES = 2 * 512 + 4 * 17 + 4 * 17 + 256 + 16


def jpeg_scan(data):
    """vfsms_jpeg_scan: the host half of Method.jpegDecoder = "device-entropy", no GPU and no libjpeg involved -- the file read once for its
    markers -> dict(the header fields of SCAN_HEADER_FIELDS, grid6, quant = [uint16 (64,) natural order per component],
    dht = [(counts uint8 (16,), values uint8 (n,)) per component DC then AC], segments = [(bytes, first MCU, first subsequence)] unstuffed,
    subseg = uint32 (nsub,), record = the raw bytes).  A file not taken: the int return code (VFSMS_ERR_UNSUPPORTED / VFSMS_ERR_BAD_ARG)."""
    lib = load_library()
    need = C.c_size_t()
    rc = lib.vfsms_jpeg_scan(data, len(data), None, 0, C.byref(need))
    if rc != VFSMS_ERR_CAPACITY:
        return rc
    rec = np.zeros(need.value, np.uint8)
    rc = lib.vfsms_jpeg_scan(data, len(data), rec.ctypes.data_as(C.c_void_p), rec.nbytes, C.byref(need))
    if rc != VFSMS_OK:
        return rc
    rec = rec[:need.value]
    head = rec[:4 * len(SCAN_HEADER_FIELDS)].view(np.uint32)
    out = {k: int(v) for k, v in zip(SCAN_HEADER_FIELDS, head)}
    nc = out["ncomp"]
    out["grid6"] = [out["grid%d" % k] for k in range(6)]
    out["quant"] = [rec[out["off_quant"] + 128 * k:out["off_quant"] + 128 * (k + 1)].view(np.uint16).copy() for k in range(nc)]
    out["dht"] = []
    for k in range(2 * nc):
        t = rec[out["off_tables"] + k * HUFF_TABLE_BYTES:out["off_tables"] + (k + 1) * HUFF_TABLE_BYTES]
        counts = t[-16:].copy()
        out["dht"].append((counts, t[-272:-16][:int(counts.sum())].copy()))
    segs = rec[out["off_seg"]:out["off_seg"] + 16 * out["nseg"]].view(np.uint32).reshape(-1, 4)
    base = out["off_stream"]
    out["segments"] = [(rec[base + int(o):base + int(o) + int(n)].tobytes(), int(m), int(s0)) for o, n, m, s0 in segs]
    out["subseg"] = rec[out["off_subseg"]:out["off_subseg"] + 4 * out["nsub"]].view(np.uint32).copy()
    out["record"] = rec
    return out


def jpeg_coefficients(data):
    """vfsms_jpeg_coefficients: the host half of Method.jpegDecoder = "device", no GPU involved -- the quantised DCT coefficients of a JPEG
    file as the entropy decode leaves them (what vfsms_tile_fill_jpeg_dct stages for the device's inverse transform) -> (h, w, comps), comps a
    list of (coef int16 (block_rows, block_cols, 64) in natural order, quant uint16 (64,) in natural order) per component, the block grids on
    whole iMCUs.  None when the file is not taken (not 8-bit gray / 4:2:0 Y Cb Cr, damaged, no libjpeg.so.8)."""
    lib = load_library()
    h, w, nc, need = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    grid = (C.c_int * 6)()
    rc = lib.vfsms_jpeg_coefficients(data, len(data), None, 0, C.byref(h), C.byref(w), C.byref(nc), grid, C.byref(need))
    if rc != VFSMS_ERR_CAPACITY:
        return None
    out = np.empty(need.value, np.uint8)
    rc = lib.vfsms_jpeg_coefficients(data, len(data), out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(h), C.byref(w), C.byref(nc), grid, C.byref(need))
    if rc != VFSMS_OK:
        return None
    return h.value, w.value, _coefficient_layout(out, nc.value, grid)


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.vfsms_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def jpeg_encode(img, bgr=True, quality=95):
    """vfsms_jpeg_encode: u8 (h, w) or (h, w, 3) rows (B G R when `bgr`, the canvas order) -> a complete baseline JPEG stream as a u8 array,
    libjpeg defaults + `quality` (cv2.imwrite's: 95) -- byte for byte what Pillow / cv2 write for the same pixels.  None when the host has
    no libjpeg.so.8 (the caller writes through Pillow).  No GPU involved; releases the interpreter lock."""
    lib = load_library()
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and img.strides[-1] == 1 and (img.ndim == 2 or (img.shape[2] == 3 and img.strides[1] == 3))
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    cap = max(1 << 16, h * w * ch // 4)
    n = C.c_size_t()
    for _ in range(2):
        out = np.empty(cap, np.uint8)
        rc = lib.vfsms_jpeg_encode(img.ctypes.data_as(C.c_void_p), h, w, ch, img.strides[0], int(bool(bgr)), int(quality),
                                   out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        if rc == VFSMS_OK:
            return out[:n.value]
        if rc == VFSMS_ERR_UNSUPPORTED:
            return None
        if rc != VFSMS_ERR_CAPACITY:
            raise VfsmsError("libvfsms error %d: %s" % (rc, _last_error(lib)), code=int(rc))
        cap = n.value
    raise VfsmsError("jpeg_encode: the stream did not fit the size the library asked for")


def jpeg_join(parts, stripe_rows, total_rows):
    """vfsms_jpeg_join: the streams of consecutive stripes (jpeg_encode of rows [k * stripe_rows, (k + 1) * stripe_rows) of one image) -> ONE
    JPEG whose restart intervals are the stripes; u8 array."""
    lib = load_library()
    n = len(parts)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in parts])
    sizes = (C.c_size_t * n)(*[p.size for p in parts])
    need = C.c_size_t()
    rc = lib.vfsms_jpeg_join(ptrs, sizes, n, int(stripe_rows), int(total_rows), None, 0, C.byref(need))
    if rc == VFSMS_OK:
        out = np.empty(need.value, np.uint8)
        rc = lib.vfsms_jpeg_join(ptrs, sizes, n, int(stripe_rows), int(total_rows), out.ctypes.data_as(C.c_void_p), out.size, C.byref(need))
    if rc != VFSMS_OK:
        raise VfsmsError("libvfsms error %d: %s" % (rc, _last_error(lib)), code=int(rc))
    return out


def default_engine():
    """Process-wide engine on the GPU selected by LOCAL_RANK (one process per GPU) or device 0."""
    global _default_engine
    if _default_engine is None:
        dev = int(os.environ.get("VFSMS_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        lib = load_library()
        n = lib.vfsms_device_count()
        if n <= 0:
            raise VfsmsError("no HIP device visible: imagestitch_amd needs an MI355X (there is no CPU fallback)")
        _default_engine = Engine(dev % n)
    return _default_engine


def _call_with_evaluator(attempts, call):
    """call(vfsms_attempt_eval) -> return code, with the Python evaluator `attempts` behind the C callback: attempts(items) with
    items = [(pair, direction, i), ...] -> int32[n, <= 8] rows {status, raw dx, raw dy, votes, nA, nB, ...} (include/vfsms.h).  What
    `attempts` raises comes out of here as that same exception, once the library has unwound; a library error raises VfsmsError."""
    lib = load_library()
    err = []

    def cb(_user, items, count, rows):
        try:
            res = np.asarray(attempts([(items[k].pair, items[k].direction, items[k].i) for k in range(count)]), np.int32).reshape(count, -1)
            np.ctypeslib.as_array(rows, (count, ATTEMPT_INTS))[:, :res.shape[1]] = res[:, :ATTEMPT_INTS]       # columns the evaluator leaves out stay 0
            return VFSMS_OK
        except Exception as e:            # never let an exception cross the C frame
            err.append(e)
            return VFSMS_ERR_BAD_ARG
    rc = call(ATTEMPT_EVAL(cb))
    if err:
        raise err[0]
    if rc != VFSMS_OK:
        raise VfsmsError("libvfsms error %d: %s" % (rc, _last_error(lib)), code=int(rc))


def pairs_offsets_blind_eval(attempts, shapes, params, first, last, per):
    """vfsms_pairs_offsets_blind_eval over a Python evaluator (needs no GPU) -> (int32[4, per, 6], int32[4], stats)."""
    lib = load_library()
    n, sh, _hs = _path_arrays(shapes)
    out = np.zeros((4, max(per, 1), 6), np.int32)
    d_out = np.zeros(4, np.int32)
    stats = np.zeros(8, np.int64)
    _call_with_evaluator(attempts, lambda ev: lib.vfsms_pairs_offsets_blind_eval(ev, None, _ptr(sh), n, int(first), int(last), int(max(per, 1)),
                                                                                 C.byref(params), _ptr(out), _ptr(d_out), _ptr(stats)))
    return out[:, :per], d_out, tuple(int(v) for v in stats)


def pairs_offsets_eval(attempts, shapes, params, first=0, last=None, direction=1, midpath=False, stop_on_fail=False):
    """vfsms_pairs_offsets_eval: the library's candidate state machine over a Python evaluator of fused batches (needs no GPU).
    attempts(items) with items = [(pair, direction, i), ...] -> rows [[status, raw dx, raw dy, votes, nA, nB, ...], ...]."""
    lib = load_library()
    n, sh, _hs = _path_arrays(shapes)
    last = n - 1 if last is None else last
    out = np.zeros((max(last - first, 0), 6), np.int32)
    d_out = C.c_int32()
    stats = np.zeros(8, np.int64)
    _call_with_evaluator(attempts, lambda ev: lib.vfsms_pairs_offsets_eval(ev, None, _ptr(sh), n, int(first), int(last), int(direction),
                                                                           int(bool(midpath)), int(bool(stop_on_fail)), C.byref(params),
                                                                           _ptr(out), C.byref(d_out), _ptr(stats)))
    return out, d_out.value, tuple(int(v) for v in stats)
