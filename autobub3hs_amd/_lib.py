"""ctypes loader of the in-tree gfx950 library (autobub3hs_amd/libabub_hip.so).

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded this module
raises, loudly.  (No CPU fallback exists in this package.)
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libabub_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "abub_hip.h")


class Job(C.Structure):
    _fields_ = [("cur", C.c_uint32), ("ref", C.c_uint32), ("model", C.c_uint32), ("out", C.c_uint32)]


class TrigSeg(C.Structure):
    _fields_ = [("hist", C.c_void_p), ("pending", C.c_void_p), ("first", C.c_int32), ("count", C.c_int32)]


class TrigStack(C.Structure):
    _fields_ = [("seg0", C.c_uint32), ("nseg", C.c_uint32), ("F", C.c_int32), ("start", C.c_int32), ("tss", C.c_int32),
                ("first_bad", C.c_int32)]


TRIG_MAX_PIXELS = 2147483583  # ABUB_TRIG_MAX_PIXELS (2^31 - 65): abub_trigger_search_dev refuses a larger W * H


class ContourDesc(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("area", C.c_double),
                ("radius", C.c_double), ("m00", C.c_double), ("m10", C.c_double), ("m01", C.c_double), ("cx", C.c_float),
                ("cy", C.c_float), ("gx", C.c_float), ("gy", C.c_float), ("npts", C.c_uint32), ("reserved", C.c_uint32)]


class LocMask(C.Structure):
    _fields_ = [("fid", C.c_void_p), ("bel", C.c_void_p), ("fw", C.c_int32), ("fh", C.c_int32), ("bw", C.c_int32),
                ("bh", C.c_int32)]


LOC_MAXTRACK = 10


class LocStack(C.Structure):
    _fields_ = [("cam", C.c_int32), ("genesis", C.c_int32), ("ntrack", C.c_int32), ("bad", C.c_int32),
                ("track", C.c_int32 * LOC_MAXTRACK), ("reserved", C.c_int32 * 2)]


class PeekItem(C.Structure):
    _fields_ = [("diff", C.c_uint64), ("frame", C.c_uint64), ("thr_out", C.c_uint64), ("pres_out", C.c_uint64),
                ("thr", C.c_int32), ("rect_begin", C.c_int32), ("rect_count", C.c_int32), ("reserved", C.c_int32)]


class ActJob(C.Structure):  # abub_act_job
    _fields_ = [("cur", C.c_uint64), ("ref", C.c_uint64)]


def build(force=False):
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc"))
            if f.endswith((".hip", ".h", ".hpp")) or f == "Makefile"] + [HEADER]
    stale = force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), "-s"])
    return SO


_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
SIGNATURES = {
    "abub_last_error": (C.c_char_p, []),
    "abub_device_count": (_i, []),
    "abub_device_info": (_i, [_i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_uint64)]),
    "abub_sigma6_dev": (_i, [_vp, _vp, _sz, _vp]),
    "abub_fill_stack_jobs_dev": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp]),
    "abub_diff_hist_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    "abub_diff_roi_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_train_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "abub_pair_hist_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "abub_posttrig_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "abub_fg_compact_dev": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "abub_fast_path": (_i, [_i]),
    "abub_scratch_release": (_i, [_vp]),
    "abub_bound_counts_dev": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "abub_diff_hist_chained_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    "abub_diff_hist_chained_store_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "abub_k2_set_option": (_i, [C.c_char_p, _i]),
    "abub_k2_deferred_ok": (_i, [_i, _i]),
    "abub_k3_set_option": (_i, [C.c_char_p, _i]),
    "abub_k2_pieces_cap": (_sz, [_i, _i, _i]),
    "abub_png_raw_stride": (_sz, [_i, _i]),
    "abub_png_decode_dev": (_i, [_vp, _sz, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "abub_png_raw_stride_kind": (_sz, [_i, _i, C.c_uint32]),
    "abub_png_decode_typed_dev": (_i, [_vp, _sz, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "abub_png_raw_stride_adam7": (_sz, [_i, _i, C.c_uint32]),
    "abub_png_decode_adam7_dev": (_i, [_vp, _sz, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "abub_abf_decode_dev": (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "abub_bmp_decode_dev": (_i, [_vp, _sz, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "abub_unzip_dev": (_i, [_vp, _sz, _vp, _i, _vp, _sz, _vp, _vp]),
    "abub_crc32_dev": (_i, [_vp, _sz, _vp, _i, _vp, _vp, _vp]),
    "abub_abf_file_bound": (_sz, [_i, _i]),
    "abub_abf_encode_scratch_bytes": (_sz, [_i, _i, _i]),
    "abub_abf_encode_dev": (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "abub_png_file_bound": (_sz, [_i, _i]),
    "abub_png_encode_scratch_bytes": (_sz, [_i, _i, _i]),
    "abub_png_encode_dev": (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "abub_zip_pack_dev": (_i, [_vp, _sz, _vp, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "abub_frames_compare_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _sz, _vp, _vp]),
    "abub_frame_stats_dev": (_i, [_vp, _sz, _vp, _vp, _sz, _vp, _i, _sz, _vp, _vp]),
    "abub_pixel_activity_dev": (_i, [_vp, _sz, _vp, _vp, _vp, _i, _sz, _vp, _sz, _vp, _vp]),
    "abub_frame_shift_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_frame_cells_grid": (_i, [_i, _i, _i] + [C.POINTER(_i)] * 4),
    "abub_frame_shift_cells_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_frame_light_cells_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_frame_focus_cells_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_frame_noise_cells_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "abub_frame_lines_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "abub_peek_planes_dev": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "abub_diff_hist_chained_deferred_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, C.c_uint32, _vp, _vp, _vp]),
    "abub_diff_hist_pieces_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "abub_diff_hist_compact_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    "abub_posttrig_compact_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    "abub_pairs_group_dev": (_i, [_vp, _vp, C.c_uint32, _i, _vp, _vp, _vp, _vp, _vp]),
    "abub_pairs_group_hist_dev": (_i, [_vp, _vp, C.c_uint32, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "abub_fg_compact_pairs_dev": (_i, [_vp, _i, _i, _i, _vp, _vp, C.c_uint32, _vp, _vp]),
    "abub_match_ccorr_dev": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "abub_subsat_hist_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "abub_match_ccorr_batch_dev": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "abub_match_best_batch_dev": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "abub_match_best_scratch_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "abub_binarize_thr_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "abub_label_blobs_dev": (_i, [_vp, _vp, _vp, C.c_uint32, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp,
                                  C.c_uint32, _vp, _vp, _sz, _vp]),
    "abub_label_blobs_scratch_bytes": (_sz, [_i, _i, _i, C.c_uint32, _i]),
    "abub_trace_contours_dev": (_i, [_vp, _vp, C.c_uint32, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32,
                                     _vp, _vp, _sz, _vp]),
    "abub_trace_contours_scratch_bytes": (_sz, [_i, C.c_uint32]),
    "abub_trace_contours_limits": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "abub_trigger_search_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _i, _vp]),
    "abub_trigger_search_desc_bytes": (_sz, [_i, _i]),
    "abub_trigger_clear_pending_dev": (_i, [_vp, _vp, _sz, _vp]),
    "abub_trigger_search_limits": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "abub_describe_contours_dev": (_i, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _i, _vp, C.c_uint32, _vp]),
    "abub_localize_stacks_dev": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, C.c_uint32, _vp, _sz, _vp, _vp, C.c_uint32, _vp,
                                      C.c_uint32, _vp, _vp]),
    "abub_localize_scratch_bytes": (_sz, [_i, _i]),
    "abub_localize_limits": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "abub_ctx_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i]),
    "abub_ctx_destroy": (None, [_vp]),
    "abub_ctx_train": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp]),
    "abub_ctx_pair_hist": (_i, [_vp, _vp, _vp, _vp]),
    "abub_ctx_set_model": (_i, [_vp, _vp, _vp]),
    "abub_ctx_upload_stack": (_i, [_vp, C.POINTER(_vp), _i]),
    "abub_ctx_diff_hist_batch": (_i, [_vp, _i, _i, _i, _vp]),
    "abub_ctx_diff_frame": (_i, [_vp, _i, _i, _vp, _vp]),
    "abub_ctx_diff_frame_roi": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "abub_ctx_posttrig": (_i, [_vp, _i, _vp, _vp]),
    "abub_ctx_foreground": (_i, [_vp, _i, _vp, _i, C.POINTER(_i)]),
    "abub_ctx_match_template": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
    "abub_ctx_subtract_image": (_i, [_vp, _vp, _vp]),
    "abub_ctx_set_image": (_i, [_vp, _vp]),
    "abub_ctx_fetch_image": (_i, [_vp, _vp]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(
                f"{SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the hot path)")
        try:  # torch ships its own HIP runtime: load it first, so that the library binds to it instead of a second copy
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the header drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class AbubError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        raise AbubError(f"{what} failed rc={rc}: {lib().abub_last_error().decode(errors='replace')}")
