"""ctypes front-end of libabub_host.so: the C++ mirror of the reference's AnalyzerUnit / L3Localizer /
Trainer API (include/abub3hs/) driven the way AutoBubStart3.cpp drives it.  Fails loudly when the
native library is missing; nothing here computes on the CPU what the GPU path should compute."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libabub_host.so")

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_vp, _i, _s = C.c_void_p, C.c_int, C.c_char_p
# name -> (restype, argtypes) of every abh_* entry this module calls (host/capi.cpp, host/pipeline.cpp)
SIGNATURES = {
    "abh_run_new": (_vp, []),
    "abh_run_open": (_vp, [_i, _s, _s, _s]),
    "abh_run_free": (None, [_vp]),
    "abh_run_events": (_s, [_vp]),
    "abh_run_frames": (_s, [_vp, _s, _i]),
    "abh_run_image": (_i, [_vp, _s, _s, _u8p, _i, _ip, _ip]),
    "abh_run_entry_info": (_i, [_vp, _s, _s, _dp]),
    "abh_run_entry_raw": (C.c_longlong, [_vp, _s, _s, _u8p, C.c_longlong]),
    "abh_run_add_event": (_i, [_vp, _s, _i, _u8p, _i, _i, _i, _u8p]),
    "abh_train": (_i, [_vp, _i, _ip, _ip, _u8p, _u8p]),
    "abh_train_device": (_i, [_vp, _i, _ip, _ip, _u8p, _u8p, _i, _dp]),
    "abh_set_model": (_i, [_vp, _i, _u8p, _u8p, _i, _i, _i]),
    "abh_probe_frame_stats": (_i, [_vp, _s, _i, _u8p, _i, _i, _i, _dp]),
    "abh_run_batched": (_i, [_vp, _i, _s, _s, _s] + [_i] * 7 + [_dp]),
    "abh_run_batched_peek": (_i, [_vp, _i, _s, _s, _s] + [_i] * 7 + [_dp, _s, _dp]),
    "abh_peek_planes_host": (None, [_u8p, _u8p, _i, _i, _i, _ip, _i, _u8p, _u8p]),
    "abh_result_rects": (_i, [_vp, _ip, _i]),
    "abh_analyze": (_i, [_vp, _s, _i, _s]),
    "abh_last_error": (_s, [_vp]),
    "abh_run_last": (_vp, [_vp]),
    "abh_result_state": (None, [_vp, _ip]),
    "abh_result_error": (_s, [_vp]),
    "abh_result_ndesc": (_i, [_vp, _i]),
    "abh_result_desc": (None, [_vp, _i, _i, _dp]),
    "abh_result_ndz": (_i, [_vp, _i]),
    "abh_result_dz": (C.c_float, [_vp, _i, _i]),
    "abh_result_dzdt": (C.c_float, [_vp, _i]),
    "abh_result_drdt": (C.c_float, [_vp, _i]),
    "abh_imdecode": (_i, [_u8p, _i, _u8p, _i, _ip, _ip]),
    "abh_abf_encode": (C.c_longlong, [_u8p, _i, _i, _u8p, C.c_longlong]),
    "abh_abf_decode": (_i, [_u8p, C.c_longlong, _u8p, _i, _i]),
    "abh_run_repack": (_i, [_vp, _s, _i, _i, _dp]),
    "abh_run_repack_dev": (_i, [_vp, _s, _i, _i, _i, _dp]),
    "abh_png_huff_encode": (C.c_longlong, [_u8p, _i, _i, _u8p, C.c_longlong]),
    "abh_png_huff_bound": (C.c_longlong, [_i, _i]),
    "abh_png_huff_lengths": (_i, [C.POINTER(C.c_uint64), _i, _i, _u8p]),
    "abh_run_unpack": (_i, [_vp, _s, _i, _i, _dp]),
    "abh_run_unpack_dev": (_i, [_vp, _s, _i, _i, _i, _dp]),
    "abh_run_verify": (_i, [_vp, _vp, _i, _i, _dp, C.c_char_p, _i]),
    "abh_run_verify_dev": (_i, [_vp, _vp, _i, _i, _i, _dp, C.c_char_p, _i]),
    "abh_run_verify_report": (_s, [_vp]),
    "abh_run_repack_archive": (_i, [_vp, _s, _i, _i, _i, _i, _dp]),
    "abh_run_verify_archive": (_i, [_vp, _vp, _i, _i, _i, _dp, C.c_char_p, _i]),
    "abh_run_survey": (_i, [_vp, _s, _i, _i, _dp, C.c_char_p, _i]),
    "abh_run_survey_dev": (_i, [_vp, _s, _i, _i, _i, _dp, C.c_char_p, _i]),
    "abh_run_survey_report": (_s, [_vp]),
    "abh_run_survey_planes": (_i, [_vp, _s, _s, _i, _i, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_planes_dev": (_i, [_vp, _s, _s, _i, _i, _i, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_shift": (_i, [_vp, _s, _s, _s, _i, _i, _i, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_shift_dev": (_i, [_vp, _s, _s, _s, _i, _i, _i, _i, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_frame_shift_host": (_i, [_u8p, _u8p, _i, _i, _i, _u64p]),
    "abh_shift_best": (None, [_u64p, _i, C.POINTER(_i)]),
    "abh_run_survey_field": (_i, [_vp, _s, _s, _s, _i, _s, _i, _i, _i, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_field_dev": (_i, [_vp, _s, _s, _s, _i, _s, _i, _i, _i, _i, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_light": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _i, _i, _dp, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_light_dev": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _i, _i, _i, _dp, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_light_cells_host": (_i, [_u8p, _u8p, _i, _i, _i, _i, _i, _i, _u32p]),
    "abh_light_model_host": (_i, [_u8p, _u8p, _i, _i, _i, _i, _i, _i, _u32p]),
    "abh_light_frame": (None, [_u32p, _u32p, _i, C.POINTER(C.c_longlong)]),
    "abh_run_survey_focus": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_focus_dev": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _i, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_focus_cells_host": (_i, [_u8p, _u8p, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32)]),
    "abh_focus_model_host": (_i, [_u8p, _u8p, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "abh_focus_cell": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_longlong)]),
    "abh_focus_frame": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int64), _i, C.POINTER(C.c_longlong)]),
    "abh_run_survey_noise": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _s, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_char_p, _i]),
    "abh_run_survey_noise_dev": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _s, _i, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_char_p,
                                      _i]),
    "abh_noise_cells_host": (_i, [_u8p, _u8p, _u8p, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32)]),
    "abh_noise_model_host": (_i, [_u8p, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int64)]),
    "abh_noise_cell": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_longlong)]),
    "abh_noise_frame": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int64), _i, C.POINTER(C.c_longlong)]),
    "abh_run_survey_lines": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _s, _s, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_char_p,
                                  _i]),
    "abh_run_survey_lines_dev": (_i, [_vp, _s, _s, _s, _i, _s, _i, _s, _s, _s, _s, _i, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                      C.c_char_p, _i]),
    "abh_lines_host": (_i, [_u8p, _u8p, _u8p, _i, _i, _u32p, _u32p]),
    "abh_lines_model_host": (_i, [_u8p, _u8p, _i, _i, _u32p, _u32p]),
    "abh_lines_rate": (_i, [_u32p, _u32p, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_ulonglong)]),
    "abh_lines_frame": (None, [_u32p, _u32p, _u32p, _u32p, _i, _i, _i, C.POINTER(C.c_longlong), _u8p, _u8p]),
    "abh_field_grid": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "abh_field_cells_host": (_i, [_u8p, _u8p, _i, _i, _i, _u32p, C.POINTER(C.c_int32)]),
    "abh_activity_add_host": (None, [C.POINTER(C.c_uint32), _u8p, _u8p, _u8p, _u8p, C.c_uint64]),
    "abh_frame_stats_host": (None, [_u8p, _u8p, _u8p, _u8p, C.c_uint64, _u64p]),
    "abh_zip_write": (_i, [_s, _i, _u8p, _u32p, _u8p, _u64p]),
    "abh_zip_error": (_s, []),
    "abh_png_walk": (_i, [_u8p, _i, _i, _i, _u32p, _i, _ip, _ip, _u8p]),
    "abh_png_walk_typed": (_i, [_u8p, _i, _i, _i, _u32p, _i, _ip, _ip, _u8p, _u32p]),
    "abh_png_walk_adam7": (_i, [_u8p, _i, _i, _i, _i, _u32p, _i, _ip, _ip, _u8p, _u32p]),
    "abh_bmp_walk": (_i, [_u8p, _i, _i, _i, _u32p, _u8p]),
    "abh_imwrite": (_i, [_s, _u8p, _i, _i]),
    "abh_write_header": (None, [_s, _s, _i, _i]),
    "abh_event_to_file": (_i, [_vp, _s, _i, _i, _s, _s, _s, _i]),
    "abh_writer_probe": (None, [_s, _s, _i, _i, _i, _ip, _ip, _ip, _ip, _dp]),
    "abh_contours": (_i, [_u32p, _i, _i, _i, _ip, _ip, _i, _i]),
    "abh_binarize_threshold": (_i, [_u32p, _i, _i]),
    "abh_entropy": (C.c_float, [_u32p, _i, _i]),
    "abh_blob_stats": (None, [_ip, _i, _dp]),
    "abh_best_match": (None, [_u64p, _u64p, _i, _i, _u8p, _i, _i, _fp, _fp]),
    "abh_sig_new": (_vp, []),
    "abh_sig_free": (None, [_vp]),
    "abh_sig_eval": (C.c_double, [_vp, _u32p, _i, _i, _i, _ip]),
    "abh_pipe_new": (_vp, [_i] * 6 + [_ip, _i, _s]),
    "abh_pipe_free": (None, [_vp]),
    "abh_pipe_error": (_s, []),
    "abh_pipe_set_sigma": (None, [_vp, _vp]),
    "abh_pipe_run": (_i, [_vp] * 5),
    "abh_pipe_run_host": (_i, [_vp] * 4),
    "abh_pipe_stack": (_vp, [_vp, _i]),
    "abh_pipe_timing": (_i, [_vp, _dp]),
    "abh_pipe_set_option": (_i, [_vp, _s, _i]),
    "abh_pipe_blob_stats": (None, [_vp, _dp]),
    "abh_pipe_contour_stats": (None, [_vp, _dp]),
    "abh_pipe_trigger_stats": (None, [_vp, _dp]),
    "abh_pipe_localize_stats": (None, [_vp, _dp]),
    "abh_pipe_trigger_totals": (None, [_dp]),
    "abh_pipe_localize_totals": (None, [_dp]),
    "abh_pipe_bellows": (None, [_vp, _dp]),
}
_lib = None


def build(force=False):
    from . import _lib as hiplib

    hiplib.build(force)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "host"), "-s"])
    return SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(f"{SO} is missing: run __graft_entry__.build()")
        from . import _lib as hiplib

        hiplib.lib()  # the HIP library first, bound to torch's HIP runtime (see _lib.lib)
        L = C.CDLL(SO)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if this table and the library drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


DESC_KEYS = ("x", "y", "w", "h", "area", "radius", "m00", "m10", "m01", "cx", "cy")


def _read_result(res, with_dz):
    """A StackResult (host/stackresult.hpp) handed out by abh_run_last / abh_pipe_stack -> (staged, state, bubbles,
    error text); a bubble's per-frame dz list only where asked for."""
    L = lib()
    o = (C.c_int * 6)()
    L.abh_result_state(res, o)
    state = {"trig": o[1], "status": o[2], "ok": bool(o[4]), "loc_thres": o[3]}
    bubbles = []
    buf = (C.c_double * len(DESC_KEYS))()
    for b in range(o[5]):
        descs = []
        for d in range(L.abh_result_ndesc(res, b)):
            L.abh_result_desc(res, b, d, buf)
            dd = dict(zip(DESC_KEYS, list(buf)))
            for k in ("x", "y", "w", "h"):
                dd[k] = int(dd[k])
            descs.append(dd)
        bub = {"desc": descs, "dzdt": L.abh_result_dzdt(res, b), "drdt": L.abh_result_drdt(res, b)}
        if with_dz:
            bub["dz"] = [L.abh_result_dz(res, b, i) for i in range(L.abh_result_ndz(res, b))]
        bubbles.append(bub)
    return o[0], state, bubbles, L.abh_result_error(res).decode()


def _read_rects(res):
    """StackResult::rects: the boxes (x, y, w, h) of the analyzer's last localizer round, those of _4_BubbleDetected."""
    L = lib()
    n = L.abh_result_rects(res, None, 0)
    buf = (C.c_int * (4 * max(n, 1)))()
    L.abh_result_rects(res, buf, n)
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]


def peek_planes_host(D, trig, cut, rects):
    """The host route's two DebugPeek planes (host/peek.cpp peekPlanesHost, the definition of abub_peek_planes_dev):
    D, trig u8 [H, W] -> (255 where D > cut, trig with cv::rectangle of every (x, y, w, h) drawn)."""
    D, trig = np.ascontiguousarray(D, np.uint8), np.ascontiguousarray(trig, np.uint8)
    H, W = D.shape
    rc = np.ascontiguousarray(np.asarray(rects, np.int64).reshape(-1, 4).astype(np.int32))
    thr, pres = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)
    lib().abh_peek_planes_host(D.ctypes.data_as(_u8p), trig.ctypes.data_as(_u8p), W, H, int(cut), rc.ctypes.data_as(_ip), len(rc),
                               thr.ctypes.data_as(_u8p), pres.ctypes.data_as(_u8p))
    return thr, pres


class Run:
    """A run: in memory (events added per camera), a directory tree (kind="raw") or a zip archive (kind="zip");
    trained per camera, then analysed per (event, camera)."""

    def __init__(self, kind=None, run_folder="", image_folder="Images", image_format="cam%d_image%u.png"):
        L = lib()
        if kind is None:
            self._h = L.abh_run_new()
        else:
            self._h = L.abh_run_open(0 if kind == "raw" else 1, run_folder.encode(), image_folder.encode(),
                                     image_format.encode())
            if not self._h:
                raise RuntimeError(f"cannot open run source {run_folder!r} (status -10 upstream)")

    def events(self):
        return [e for e in lib().abh_run_events(self._h).decode().split("\n") if e]

    def frames(self, event, cam):
        return [f for f in lib().abh_run_frames(self._h, str(event).encode(), cam).decode().split("\n") if f]

    def entry_info(self, event, frame):
        """The archive entry behind a frame (Parser::GetImageEntryInfo): dict of method (0 stored, 8 deflated),
        compress_size, file_size and crc as the archive's central directory states them, or None where there is none to
        describe (a directory run, a run in memory, no such frame, an encrypted entry)."""
        out = (C.c_double * 4)()
        if not lib().abh_run_entry_info(self._h, str(event).encode(), frame.encode(), out):
            return None
        return dict(method=int(out[0]), compress_size=int(out[1]), file_size=int(out[2]), crc=int(out[3]))

    def entry_raw(self, event, frame):
        """The entry's compressed bytes as they lie in the archive (Parser::ReadImageEntryRaw), or None."""
        info = self.entry_info(event, frame)
        if info is None:
            return None
        buf = np.zeros(max(1, info["compress_size"]), np.uint8)
        n = lib().abh_run_entry_raw(self._h, str(event).encode(), frame.encode(), buf.ctypes.data_as(_u8p), info["compress_size"])
        return None if n < 0 else buf[:n].tobytes()

    def image(self, event, frame, cap=1 << 22):
        buf = np.empty(cap, np.uint8)
        w, h = C.c_int(), C.c_int()
        rc = lib().abh_run_image(self._h, str(event).encode(), frame.encode(), buf.ctypes.data_as(_u8p), cap,
                                 C.byref(w), C.byref(h))
        img = buf[: w.value * h.value].reshape(h.value, w.value).copy() if w.value * h.value else None
        return rc, img

    def close(self):
        if self._h:
            lib().abh_run_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_event(self, event, cam, frames, ok=None):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        F, H, W = frames.shape
        okp = None
        if ok is not None:
            ok = np.ascontiguousarray(ok, dtype=np.uint8)
            okp = ok.ctypes.data_as(_u8p)
        lib().abh_run_add_event(self._h, str(event).encode(), cam, frames.ctypes.data_as(_u8p), F, W, H, okp)
        self._shape = (H, W)

    def train(self, cam, shape=None):
        H, W = shape if shape is not None else self._shape
        mu = np.zeros((H, W), np.uint8)
        sg = np.zeros((H, W), np.uint8)
        st, tss = C.c_int(), C.c_int()
        rc = lib().abh_train(self._h, cam, C.byref(st), C.byref(tss), mu.ctypes.data_as(_u8p), sg.ctypes.data_as(_u8p))
        if rc != 0:
            raise RuntimeError(lib().abh_last_error(self._h).decode())
        return st.value, tss.value, mu, sg

    def train_on_gpu(self, ncams, shape=None):
        """Every camera trained in one pass on the device (abub::TrainOnDevice): per camera (status, tss, mu, sigma), the
        same as train(cam).  self.train_path is "device", or "host" where TrainOnDevice declined the run; self.train_stats:
        frames decoded by the GPU decoders / by host threads, decode launches, seconds, and of the first the packed frames
        (frames_gpu_unpacked, abub_abf_decode_dev) and the BMP frames (frames_gpu_bmp, abub_bmp_decode_dev); frames_gpu_unzipped:
        deflated archive entries whose zip layer the GPU inflated (abub_unzip_dev, ABUB_GPU_UNZIP=1)."""
        H, W = shape if shape is not None else self._shape
        L = lib()
        mu = np.zeros((ncams, H, W), np.uint8)
        sg = np.zeros((ncams, H, W), np.uint8)
        st = np.zeros(ncams, np.int32)
        tss = np.zeros(ncams, np.int32)
        stats = np.zeros(7, np.float64)
        rc = L.abh_train_device(self._h, ncams, st.ctypes.data_as(_ip), tss.ctypes.data_as(_ip), mu.ctypes.data_as(_u8p),
                                sg.ctypes.data_as(_u8p), H * W, stats.ctypes.data_as(_dp))
        if rc < 0:
            raise RuntimeError(L.abh_last_error(self._h).decode())
        self.train_path = "device" if rc == 0 else "host"
        self.train_stats = {"frames_gpu_decoded": int(stats[0]), "frames_host_decoded": int(stats[1]),
                            "decode_launches": int(stats[2]), "seconds": float(stats[3]),
                            "frames_gpu_unpacked": int(stats[4]), "frames_gpu_bmp": int(stats[5]),
                            "frames_gpu_unzipped": int(stats[6])}
        return [(int(st[c]), int(tss[c]), mu[c], sg[c]) for c in range(ncams)]

    def set_model(self, cam, mu, sigma, tss):
        mu = np.ascontiguousarray(mu, dtype=np.uint8)
        sigma = np.ascontiguousarray(sigma, dtype=np.uint8)
        H, W = mu.shape
        lib().abh_set_model(self._h, cam, mu.ctypes.data_as(_u8p), sigma.ctypes.data_as(_u8p), W, H, int(tss))

    def probe_frame_stats(self, event, cam, imgs):
        """Test hook (abub::AnalyzerProbe): per image the 128-bin entropy, its z-score over the images so far and the
        256-bin significance, through the private AnalyzerUnit members that the reference compiles but never calls
        (AnalyzerUnit.cpp:386-433) -> float64 [n,3]."""
        L = lib()
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, H, W = imgs.shape
        out = np.zeros((n, 3), np.float64)
        rc = L.abh_probe_frame_stats(self._h, str(event).encode(), cam, imgs.ctypes.data_as(_u8p), n, W, H,
                                     out.ctypes.data_as(_dp))
        if rc != 0:
            raise RuntimeError(f"abh_probe_frame_stats rc={rc}: " + L.abh_last_error(self._h).decode())
        return out

    def run_batched(self, ncams, outdir, run_number, frame_offset, maskdir="", ngpus=1, nthreads=16, decode_threads=16,
                    batch_mb=0, shard=(0, 1), peek_dir=None):
        """Every event of this run through the batched GPU pipeline (host/runbatch.cpp RunBatched): frames decoded (PNG, packed and BMP files: on the GPU, abub_png_decode_dev / abub_abf_decode_dev / abub_bmp_decode_dev with ABUB_GPU_BMP=1, else BMP files by host threads; ABUB_GPU_DECODE=0: by host threads into pinned
        batches), detect, blocks appended to <outdir>abub3hs_<run>.txt in event order.  With ABUB_GPU_UNZIP=1 the zip layer of
        a deflated archive's entries is inflated on the GPU too (abub_unzip_dev; frames_gpu_unzipped counts them).
        peek_dir (abub3hs --peek): the six DebugPeek images of every accepted (event, camera) written to
        <peek_dir>/<run_number>/ by a post-pass per batch, on the GPU (abub_peek_planes_dev, abub_png_encode_dev) or, with
        ABUB_PEEK_GPU=0, on host threads: the same files; the stats then have peek_stacks, peek_files, peek_bytes, peek_gpu
        and peek_s.  -> stats dict."""
        L = lib()
        st = (C.c_double * 17)()
        pk = (C.c_double * 5)()
        rc = L.abh_run_batched_peek(self._h, ncams, maskdir.encode(), outdir.encode(), run_number.encode(), frame_offset, ngpus,
                                    nthreads, decode_threads, batch_mb, shard[0], shard[1], st,
                                    None if peek_dir is None else str(peek_dir).encode(), pk)
        if rc != 0:
            raise RuntimeError(f"abh_run_batched rc={rc}: " + L.abh_last_error(self._h).decode())
        keys = ("total_s", "list_s", "decode_s", "gpu_s", "write_s", "frames", "frames_failed", "batches",
                "events_per_batch", "gpus", "frames_gpu_decoded", "frames_host_decoded", "gpudecode_s", "frames_gpu_unpacked",
                "frames_gpu_bmp", "frames_gpu_unzipped", "unzip_s")
        out = dict(zip(keys, list(st)))
        if peek_dir is not None:
            out.update(zip(("peek_stacks", "peek_files", "peek_bytes", "peek_gpu", "peek_s"), list(pk)))
        return out

    _REPACK_DEV_KEYS = ("frames_gpu_encoded", "frames_gpu_png_decoded", "frames_gpu_unpacked", "frames_host_decoded",
                        "frames_host_route", "batches", "read_s", "decode_s", "encode_s", "copy_s", "write_s", "device",
                        "frames_gpu_bmp_decoded", "frames_gpu_unzipped")

    def _rewrite_archive(self, what, outdir, nthreads, ncams, device, unpack):
        """--archive of repack / unpack: the copy is the one file <outdir>.zip"""
        L = lib()
        st = (C.c_double * 23)()
        rc = L.abh_run_repack_archive(self._h, outdir.encode(), ncams, nthreads, -1 if device is None else int(device), unpack, st)
        if rc != 0:
            raise RuntimeError(f"abh_run_{what} rc={rc}: " + L.abh_last_error(self._h).decode())
        keys = ("packed", "copied", "failed", "bytes_in", "bytes_out", "seconds")
        out = dict(zip(keys, list(st)))
        if device is not None:
            out.update(zip(self._REPACK_DEV_KEYS, list(st)[6:20]))
            out["pack_s"] = st[22]
        out.update(archive_bytes=int(st[20]), archive_entries=int(st[21]))
        return out

    def repack(self, outdir, nthreads=16, ncams=4, device=None, archive=False):
        """abub3hs --repack of this run (opened from a directory or an archive): every frame of cameras 0 .. ncams-1
        written in the packed format (abf_encode) to <outdir>/<event>/<image folder>/<same name>; `outdir` is the new run
        folder, its last component the run ID.  Files that do not decode are copied as they are.  device=None: no GPU.
        device=N (--repack-gpu): the same files, the frames decoded and packed on that GPU (abub_abf_encode_dev); raises
        when there is no such device.  archive=True (--archive): the copy is the one zip archive <outdir>.zip with the same
        files as stored entries ("A run as one archive"); the stats gain archive_bytes and
        archive_entries, with a device pack_s.  -> stats dict; raises if anything could not be written."""
        if archive:
            return self._rewrite_archive("repack", outdir, nthreads, ncams, device, 0)
        L = lib()
        keys = ("packed", "copied", "failed", "bytes_in", "bytes_out", "seconds")
        if device is None:
            st = (C.c_double * 6)()
            rc = L.abh_run_repack(self._h, outdir.encode(), ncams, nthreads, st)
        else:
            keys += ("frames_gpu_encoded", "frames_gpu_png_decoded", "frames_gpu_unpacked", "frames_host_decoded",
                     "frames_host_route", "batches", "read_s", "decode_s", "encode_s", "copy_s", "write_s", "device",
                     "frames_gpu_bmp_decoded", "frames_gpu_unzipped")
            st = (C.c_double * 20)()
            rc = L.abh_run_repack_dev(self._h, outdir.encode(), ncams, nthreads, int(device), st)
        if rc != 0:
            raise RuntimeError(f"abh_run_repack rc={rc}: " + L.abh_last_error(self._h).decode())
        return dict(zip(keys, list(st)))

    def unpack(self, outdir, nthreads=16, ncams=4, device=None, archive=False):
        """abub3hs --unpack of this run (opened from a directory or an archive; packed, PNG, BMP or mixed): the way back
        from repack.  Every frame of cameras 0 .. ncams-1 written as a canonical Huffman-only PNG (png_huff_encode) to
        <outdir>/<event>/<image folder>/<same name>; layout, event file and refusals as repack.  device=None: no GPU.
        device=N (--unpack-gpu): the same files, the frames decoded and encoded on that GPU (abub_png_encode_dev); raises
        when there is no such device.  archive=True: as for repack.  -> the stats dict of repack ("packed": PNG files
        written)."""
        if archive:
            return self._rewrite_archive("unpack", outdir, nthreads, ncams, device, 1)
        L = lib()
        keys = ("packed", "copied", "failed", "bytes_in", "bytes_out", "seconds")
        if device is None:
            st = (C.c_double * 6)()
            rc = L.abh_run_unpack(self._h, outdir.encode(), ncams, nthreads, st)
        else:
            keys += ("frames_gpu_encoded", "frames_gpu_png_decoded", "frames_gpu_unpacked", "frames_host_decoded",
                     "frames_host_route", "batches", "read_s", "decode_s", "encode_s", "copy_s", "write_s", "device",
                     "frames_gpu_bmp_decoded", "frames_gpu_unzipped")
            st = (C.c_double * 20)()
            rc = L.abh_run_unpack_dev(self._h, outdir.encode(), ncams, nthreads, int(device), st)
        if rc != 0:
            raise RuntimeError(f"abh_run_unpack rc={rc}: " + L.abh_last_error(self._h).decode())
        return dict(zip(keys, list(st)))

    def verify(self, other, nthreads=16, ncams=4, device=None, archive=False):
        """abub3hs --verify-repack: is the run `other` (another Run opened from a directory or an archive) pixel for pixel
        this one?  Every frame this run lists for cameras 0 .. ncams-1 gets one verdict: same (identical pixels, the other
        file is a packed frame), same_not_packed, copied (this file does not decode, the other has its bytes), and the
        failures differ, missing, undecodable; a frame or an event only `other` lists is extra, a failure too.
        device=None: host threads (cv::imdecode + memcmp).  device=N (--verify-gpu): the same answer, the frames decoded on
        both sides and compared (abub_frames_compare_dev) on that GPU; raises when there is no such device.
        -> dict: rc (0 = verified, 1 = something failed), the counters, event_file ("same", "differs", "missing", "not
        compared"), the device route's counters and legs (device -1: it was not taken; src_gpu_bmp_decoded /
        other_gpu_bmp_decoded: frames of each side decoded by abub_bmp_decode_dev), and findings: every failure and
        every same_not_packed frame in task order, then the extras and the event file, each a dict of event, name, verdict,
        ndiff, x, y, max_abs (and w, h, other_w, other_h where the sizes differ).  archive=True (--archive): `other` is
        opened from the archive repack(archive=True) wrote, and the event file is compared as bytes with its <run>.txt
        entry."""
        L = lib()
        st = (C.c_double * 29)()
        cap = 1 << 16
        buf = C.create_string_buffer(cap)
        if archive:
            rc = L.abh_run_verify_archive(self._h, other._h, ncams, nthreads, -1 if device is None else int(device), st, buf, cap)
        elif device is None:
            rc = L.abh_run_verify(self._h, other._h, ncams, nthreads, st, buf, cap)
        else:
            rc = L.abh_run_verify_dev(self._h, other._h, ncams, nthreads, int(device), st, buf, cap)
        if rc not in (0, 1):
            raise RuntimeError(f"abh_run_verify rc={rc}: " + L.abh_last_error(self._h).decode())
        text = buf.value if st[11] < cap else L.abh_run_verify_report(self._h)
        keys = ("events", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra")
        res = {"rc": rc, **{k: int(v) for k, v in zip(keys, list(st))}}
        res["event_file"] = ("same", "differs", "missing", "not compared")[int(st[9])]
        res["seconds"] = st[10]
        keys = ("frames_kernel", "frames_host_route", "src_gpu_png_decoded", "src_gpu_unpacked", "src_host_decoded",
                "other_gpu_png_decoded", "other_gpu_unpacked", "other_host_decoded", "batches")
        res.update({k: int(v) for k, v in zip(keys, list(st)[12:21])})
        res.update(read_s=st[21], decode_s=st[22], compare_s=st[23], device=int(st[24]))
        res.update(src_gpu_bmp_decoded=int(st[25]), other_gpu_bmp_decoded=int(st[26]))
        res.update(src_gpu_unzipped=int(st[27]), other_gpu_unzipped=int(st[28]), frames_gpu_unzipped=int(st[27]) + int(st[28]))
        cols = ("ndiff", "x", "y", "max_abs", "w", "h", "other_w", "other_h")
        res["findings"] = []
        for line in text.decode().split("\n"):
            if line:
                f = line.split("\t")
                res["findings"].append(dict(event=f[0], name=f[1], verdict=f[2], **{k: int(v) for k, v in zip(cols, f[3:])}))
        return res

    _SURVEY_KEYS = ("events", "frames", "ok", "undecodable", "missing", "other_size", "frames_kernel", "frames_host_route",
                    "gpu_png_decoded", "gpu_unpacked", "gpu_bmp_decoded", "host_decoded", "reread", "frames_gpu_unzipped", "device",
                    "W", "H", "batches", "model_cams")

    def survey(self, path=None, nthreads=16, ncams=4, device=None, planes=None, shift=None, shift_radius=4, field=None,
               field_radius=4, light=None, focus=None, noise=None, lines=None):
        """abub3hs --survey of this run (opened from a directory or an archive): the run is listed and trained as for
        detect, then every frame of cameras 0 .. ncams-1 is measured without analysing any; the report (DESIGN section 3,
        "Surveying a run") is written to `path` (None: it is not written).  device=None: host threads (cv::imdecode and
        byte loops, the definition).  device=N (--survey-gpu): the same report, byte for byte, the frames decoded and
        measured (abub_frame_stats_dev) on that GPU; raises when there is no such device.
        -> (stats dict: rc (0, or 1 if a frame is not ok), the counters of the states, frames_kernel / frames_host_route,
        the decoder lanes' counts, batches, device (-1: its route was not taken), W, H, model_cams and the legs read_s,
        decode_s, stats_s, seconds; the report's text).
        planes (--survey-planes): the directory (the CLI's DIR/<run_ID>) that gets the per-pixel activity planes (DESIGN
        section 3, "Surveying a run per pixel"): cam<c>_activity.npy, cam<c>_moved.png, activity.txt, the same bytes on
        both routes; the stats then also have plane_rows_kernel / plane_rows_host and the legs activity_s, planes_copy_s,
        planes_write_s.  The report does not change.
        shift (--survey-shift): the file that gets the shift search ("Surveying a run for movement"): per
        ok frame of a camera with a model its best displacement against mu within shift_radius (1 to 8), the same bytes on
        both routes; the stats then also have shift_frames_kernel / shift_frames_host, shift_launches and the legs shift_s
        (the device route's) and shift_host_s (the host threads', summed).  The report and the planes do not change.
        field (--survey-field): the directory (the CLI's DIR/<run_ID>) that gets the per-cell shift field (DESIGN section 3,
        "Surveying a run for local movement"): cam<c>_field.npy and field.txt, the same rows searched per cell of 128 x 128
        pixels within field_radius (1 to 8), the same bytes on both routes; the stats then also have field_frames_kernel /
        field_frames_host, field_launches and the legs field_s and field_host_s.  Nothing else changes.
        light (--survey-light): the directory (the CLI's DIR/<run_ID>) that gets the per-cell light records (DESIGN section 3,
        "Surveying a run for lighting changes"): cam<c>_light.npy, cam<c>_light_model.npy and light.txt, the same rows summed
        per cell of the field's grid at field_radius (whether or not field is given), the same bytes on both routes; the
        stats then also have light_frames_kernel / light_frames_host, light_launches and the legs light_s and light_host_s.
        Nothing else changes.
        focus (--survey-focus): the directory (the CLI's DIR/<run_ID>) that gets the per-cell focus records (DESIGN section 3,
        "Surveying a run for lost focus"): cam<c>_focus.npy, cam<c>_focus_model.npy and focus.txt, the same rows compared
        per cell of the field's grid at field_radius (whether or not field or light is given), the same bytes on both routes;
        the stats then also have focus_frames_kernel / focus_frames_host, focus_launches and the legs focus_s and
        focus_host_s.  Nothing else changes.
        noise (--survey-noise): the directory (the CLI's DIR/<run_ID>) that gets the per-cell noise records (DESIGN section 3,
        "Surveying a run for noise changes"): cam<c>_noise.npy, cam<c>_noise_model.npy and noise.txt, of the same rows those
        whose reference frame (the frame two before) is another ok frame, each against that frame per cell of the field's
        grid at field_radius, the same bytes on both routes; the stats then also have noise_frames_kernel /
        noise_frames_host, noise_launches and the legs noise_s and noise_host_s.  Nothing else changes.
        lines (--survey-lines): the directory (the CLI's DIR/<run_ID>) that gets the per-line records (DESIGN section 3,
        "Surveying a run for torn, repeated and banded frames"): cam<c>_lines_rows.npy, cam<c>_lines_cols.npy, the two model
        files and lines.txt, the same rows summed along every image row and column (no grid, any size), against the frame
        two before where that is another ok frame, the same bytes on both routes; the stats then also have
        lines_frames_kernel / lines_frames_host, lines_launches and the legs lines_s and lines_host_s.  Nothing else
        changes."""
        L = lib()
        st, pst = (C.c_double * 24)(), (C.c_double * 5)()
        products = [(v, (C.c_double * 5)(), k) for v, k in ((shift, "shift"), (field, "field"), (light, "light"), (focus, "focus"),
                                                                 (noise, "noise"), (lines, "lines"))]
        cap = 1 << 16
        buf = C.create_string_buffer(cap)
        # the widest entry takes every product; a NULL path: that product is not made
        to, pd, sp, fd, ld, od, nd, nl = (None if p is None else str(p).encode()
                                          for p in (path, planes, shift, field, light, focus, noise, lines))
        args = (self._h, to, pd, sp, int(shift_radius), fd, int(field_radius), ld, od, nd, nl, ncams, nthreads)
        out = (st, pst, *(a for _, a, _ in products), buf, cap)
        if device is None:
            rc = L.abh_run_survey_lines(*args, *out)
        else:
            rc = L.abh_run_survey_lines_dev(*args, int(device), *out)
        if rc not in (0, 1):
            raise RuntimeError(f"abh_run_survey rc={rc}: " + L.abh_last_error(self._h).decode())
        text = buf.value if st[23] < cap else L.abh_run_survey_report(self._h)
        res = {"rc": rc, **{k: int(v) for k, v in zip(self._SURVEY_KEYS, list(st))}}
        res.update(read_s=st[19], decode_s=st[20], stats_s=st[21], seconds=st[22])
        if planes is not None:
            res.update(plane_rows_kernel=int(pst[0]), plane_rows_host=int(pst[1]), activity_s=pst[2], planes_copy_s=pst[3],
                       planes_write_s=pst[4])
        for want, a, k in products:
            if want is not None:
                res.update({f"{k}_frames_kernel": int(a[0]), f"{k}_frames_host": int(a[1]), f"{k}_launches": int(a[2]), f"{k}_s": a[3],
                            f"{k}_host_s": a[4]})
        return res, text.decode()

    def analyze(self, event, cam, maskdir=""):
        L = lib()
        staged = L.abh_analyze(self._h, str(event).encode(), cam, maskdir.encode())
        if staged == -100:
            raise RuntimeError(L.abh_last_error(self._h).decode())
        return _read_result(L.abh_run_last(self._h), with_dz=True)


FRAME_STATS_KEYS = ("min", "max", "n_zero", "n_sat", "n_out", "n_moved", "flags", "sum", "sumsq", "sum_out", "sum_moved")


def frame_stats_host(cur, ref=None, mu=None, sigma6=None):
    """abub::frameStatsHost (host/survey.cpp), the definition of abub_frame_stats_dev: cur u8 (any shape), ref / mu / sigma6
    of its size or None (sigma6 = min(6 sigma, 255) goes with mu) -> dict of FRAME_STATS_KEYS; flags bit 0: n_out / sum_out
    are valid (there is a model), bit 1: n_moved / sum_moved are (a model and a reference frame)."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (cur, ref, mu, sigma6)]
    n = arrs[0].size
    assert all(a is None or a.size == n for a in arrs) and (arrs[2] is None) == (arrs[3] is None)
    out = np.zeros(11, np.uint64)
    lib().abh_frame_stats_host(*[None if a is None else a.ctypes.data_as(_u8p) for a in arrs], n, out.ctypes.data_as(_u64p))
    return dict(zip(FRAME_STATS_KEYS, (int(v) for v in out)))


def activity_add_host(planes, cur, ref=None, mu=None, sigma6=None):
    """abub::activityAddHost (host/survey.cpp), the definition of abub_pixel_activity_dev: one frame `cur` (u8, n pixels)
    ADDED in place to planes (uint32, contiguous, 6 * n words: n_zero, n_sat, n_out, sum_out, n_moved, sum_moved); ref / mu /
    sigma6 of cur's size or None (sigma6 goes with mu)."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (cur, ref, mu, sigma6)]
    n = arrs[0].size
    assert all(a is None or a.size == n for a in arrs) and (arrs[2] is None) == (arrs[3] is None)
    assert planes.dtype == np.uint32 and planes.flags["C_CONTIGUOUS"] and planes.size == 6 * n
    lib().abh_activity_add_host(planes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                *[None if a is None else a.ctypes.data_as(_u8p) for a in arrs], n)


def frame_shift_host(p, m, R):
    """abub::frameShiftHost (host/survey.cpp), the definition of abub_frame_shift_dev: the frame p and the model plane m, u8
    [H, W], at radius R -> the SAD surface, uint64 [2 R + 1, 2 R + 1], entry [dy + R, dx + R]."""
    p, m = (np.ascontiguousarray(a, dtype=np.uint8) for a in (p, m))
    assert p.ndim == 2 and p.shape == m.shape
    sad = np.zeros((2 * R + 1, 2 * R + 1), np.uint64)
    if lib().abh_frame_shift_host(p.ctypes.data_as(_u8p), m.ctypes.data_as(_u8p), p.shape[1], p.shape[0], int(R), sad.ctypes.data_as(_u64p)):
        raise ValueError(f"abh_frame_shift_host refuses {p.shape[1]}x{p.shape[0]} at radius {R}")
    return sad


def shift_best(sad, R):
    """abub::shiftBest (host/survey.cpp), the tie rule of both survey routes: a surface of radius R -> (dx, dy, at_edge)."""
    sad = np.ascontiguousarray(sad, dtype=np.uint64).reshape(-1)
    assert sad.size == (2 * R + 1) ** 2
    out = (C.c_int * 3)()
    lib().abh_shift_best(sad.ctypes.data_as(_u64p), int(R), out)
    return out[0], out[1], bool(out[2])


def field_grid(W, H, R):
    """abub_frame_cells_grid (the GPU library's, the one copy of the rule) through the host library: the whole 128 x 128 cells
    of a W x H frame's interior at radius R -> (ncx, ncy, x0, y0); ncx * ncy == 0: the frame has no field."""
    out = (C.c_int * 4)()
    if lib().abh_field_grid(int(W), int(H), int(R), out):
        raise ValueError(f"abh_field_grid refuses {W}x{H} at radius {R}")
    return tuple(out)


def field_cells_host(p, m, R):
    """abub::fieldCellsHost and abub::fieldCell (host/survey.cpp), the definition of abub_frame_shift_cells_dev and what a
    surface says: the frame p and the model plane m, u8 [H, W], at radius R -> (the cells' surfaces, uint32
    [ncy, ncx, 2 R + 1, 2 R + 1], entry [dy + R, dx + R]; their records, int32 [ncy, ncx, 5]: dx, dy, sad0, sad_best, sad_max)."""
    p, m = (np.ascontiguousarray(a, dtype=np.uint8) for a in (p, m))
    assert p.ndim == 2 and p.shape == m.shape
    try:
        ncx, ncy, _, _ = field_grid(p.shape[1], p.shape[0], R)
    except ValueError:
        ncx = ncy = 0
    sad = np.zeros((ncy, ncx, 2 * R + 1, 2 * R + 1), np.uint32)
    rec = np.zeros((ncy, ncx, 5), np.int32)
    if ncx * ncy == 0 or lib().abh_field_cells_host(p.ctypes.data_as(_u8p), m.ctypes.data_as(_u8p), p.shape[1], p.shape[0], int(R),
                                                    sad.ctypes.data_as(_u32p), rec.ctypes.data_as(C.POINTER(C.c_int32))) != ncx * ncy:
        raise ValueError(f"abh_field_cells_host refuses {p.shape[1]}x{p.shape[0]} at radius {R}")
    return sad, rec


LIGHT_KINDS = ("blind", "steady", "level", "uneven")


def _light_call(fn, a, b, x0, y0, ncx, ncy, words):
    a, b = (np.ascontiguousarray(v, dtype=np.uint8) for v in (a, b))
    assert a.ndim == 2 and a.shape == b.shape
    rec = np.zeros((max(ncy, 0), max(ncx, 0), words), np.uint32)
    if fn(a.ctypes.data_as(_u8p), b.ctypes.data_as(_u8p), a.shape[1], a.shape[0], int(x0), int(y0), int(ncx), int(ncy),
          rec.ctypes.data_as(_u32p)) != ncx * ncy or ncx * ncy <= 0:
        raise ValueError(f"the grid {ncx}x{ncy} from ({x0}, {y0}) does not lie inside {a.shape[1]}x{a.shape[0]}")
    return rec


def light_cells_host(p, m, x0, y0, ncx, ncy):
    """abub::lightCellsHost (host/survey.cpp), the definition of abub_frame_light_cells_dev: the frame p and the model
    plane m, u8 [H, W], on the grid of ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> uint32 [ncy, ncx, 6]: the
    sums of p, p^2, p m and |p - m|, the pixels with p == 0 and with p == 255."""
    return _light_call(lib().abh_light_cells_host, p, m, x0, y0, ncx, ncy, 6)


def light_model_host(mu, sigma6, x0, y0, ncx, ncy):
    """abub::lightModelHost: the model planes mu and sigma6, u8 [H, W], on the same grid -> uint32 [ncy, ncx, 3]: the sums
    of mu, mu^2 and sigma6."""
    return _light_call(lib().abh_light_model_host, mu, sigma6, x0, y0, ncx, ncy, 3)


def light_frame(rec, model):
    """abub::lightFrame: what a frame's records [..., 6] say against the model's [..., 3] -> dict: rated, clipped, changed,
    up, down, kind (a word of LIGHT_KINDS), and level_milli, ratio_min, ratio_max, gain_milli, offset_milli (None where
    light.txt has '-')."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 6)
    model = np.ascontiguousarray(model, dtype=np.uint32).reshape(-1, 3)
    assert len(rec) == len(model)
    out = (C.c_longlong * 12)()
    lib().abh_light_frame(rec.ctypes.data_as(_u32p), model.ctypes.data_as(_u32p), len(rec), out)
    v = list(out)
    blind, gain = v[5] == 0, bool(v[6])
    return {"rated": v[0], "clipped": v[1], "changed": v[2], "up": v[3], "down": v[4], "kind": LIGHT_KINDS[v[5]],
            "level_milli": None if blind else v[7], "ratio_min": None if blind else v[8], "ratio_max": None if blind else v[9],
            "gain_milli": v[10] if gain else None, "offset_milli": v[11] if gain else None}


FOCUS_KINDS = ("blind", "steady", "soft", "uneven")
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _focus_call(fn, a, b, x0, y0, ncx, ncy, words, dtype, ptr):
    a, b = (np.ascontiguousarray(v, dtype=np.uint8) for v in (a, b))
    assert a.ndim == 2 and a.shape == b.shape
    rec = np.zeros((max(ncy, 0), max(ncx, 0), words), dtype)
    if fn(a.ctypes.data_as(_u8p), b.ctypes.data_as(_u8p), a.shape[1], a.shape[0], int(x0), int(y0), int(ncx), int(ncy),
          rec.ctypes.data_as(ptr)) != ncx * ncy or ncx * ncy <= 0:
        raise ValueError(f"the grid {ncx}x{ncy} from ({x0}, {y0}) and its ring do not lie inside {a.shape[1]}x{a.shape[0]}")
    return rec


def focus_cells_host(p, m, x0, y0, ncx, ncy):
    """abub::focusCellsHost (host/survey.cpp), the definition of abub_frame_focus_cells_dev: the frame p and the model
    plane m, u8 [H, W], on the grid of ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> int32 [ncy, ncx, 5]: the sums of
    gx^2, gy^2, gx hx and gy hy (central differences of p and of m), the pixels with p == 0 or p == 255."""
    return _focus_call(lib().abh_focus_cells_host, p, m, x0, y0, ncx, ncy, 5, np.int32, _i32p)


def focus_model_host(mu, sigma6, x0, y0, ncx, ncy):
    """abub::focusModelHost: the model planes mu and sigma6, u8 [H, W], on the same grid -> int64 [ncy, ncx, 3]: the sums
    of hx^2 and hy^2, and nv, the sum over the cell and its ring of (sigma6 c)^2."""
    return _focus_call(lib().abh_focus_model_host, mu, sigma6, x0, y0, ncx, ncy, 3, np.int64, _i64p)


def focus_cell(rec, model):
    """abub::focusCell: what one cell's record [5] says against its model's [3] -> dict: rated, clipped, changed, softer
    (bool), keep, energy (None where the cell is not rated)."""
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(5)
    model = np.ascontiguousarray(model, dtype=np.int64).reshape(3)
    out = (C.c_longlong * 6)()
    lib().abh_focus_cell(rec.ctypes.data_as(_i32p), model.ctypes.data_as(_i64p), out)
    v = list(out)
    return {"rated": bool(v[0]), "clipped": bool(v[1]), "changed": bool(v[2]), "softer": bool(v[3]),
            "keep": v[4] if v[0] else None, "energy": v[5] if v[0] else None}


def focus_frame(rec, model):
    """abub::focusFrame: what a frame's records [..., 5] say against the model's [..., 3] -> dict: rated, clipped, changed,
    softer, harder, kind (a word of FOCUS_KINDS), and keep_milli, keep_min, keep_max, energy_milli (None where focus.txt has
    '-')."""
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 5)
    model = np.ascontiguousarray(model, dtype=np.int64).reshape(-1, 3)
    assert len(rec) == len(model)
    out = (C.c_longlong * 10)()
    lib().abh_focus_frame(rec.ctypes.data_as(_i32p), model.ctypes.data_as(_i64p), len(rec), out)
    v = list(out)
    blind = v[5] == 0
    return {"rated": v[0], "clipped": v[1], "changed": v[2], "softer": v[3], "harder": v[4], "kind": FOCUS_KINDS[v[5]],
            "keep_milli": None if blind else v[6], "keep_min": None if blind else v[7], "keep_max": None if blind else v[8],
            "energy_milli": None if blind else v[9]}


NOISE_STATES = ("clipped", "busy", "nobase", "noisy", "quiet", "same")
NOISE_KINDS = ("blind", "busy", "steady", "noisy", "quiet", "uneven")


def noise_cells_host(p, r, sigma6, x0, y0, ncx, ncy):
    """abub::noiseCellsHost (host/survey.cpp), the definition of abub_frame_noise_cells_dev: the frame p, its reference
    frame r and the plane sigma6, u8 [H, W], on the grid of ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> int32
    [ncy, ncx, 6]: n_over, n_clip, s1_in, s2_in, sad, s2_all of d = p - r."""
    p, r, sigma6 = (np.ascontiguousarray(v, dtype=np.uint8) for v in (p, r, sigma6))
    assert p.ndim == 2 and p.shape == r.shape == sigma6.shape
    rec = np.zeros((max(ncy, 0), max(ncx, 0), 6), np.int32)
    if lib().abh_noise_cells_host(p.ctypes.data_as(_u8p), r.ctypes.data_as(_u8p), sigma6.ctypes.data_as(_u8p), p.shape[1], p.shape[0],
                                  int(x0), int(y0), int(ncx), int(ncy), rec.ctypes.data_as(_i32p)) != ncx * ncy or ncx * ncy <= 0:
        raise ValueError(f"the grid {ncx}x{ncy} from ({x0}, {y0}) does not lie inside {p.shape[1]}x{p.shape[0]}")
    return rec


def noise_model_host(sigma6, recs, x0, y0, ncx, ncy):
    """abub::noiseModelHost: the plane sigma6, u8 [H, W], and the records [n, ncy, ncx, 6] (n may be 0) of the camera's
    rows at stack position 1 on the same grid -> int64 [ncy, ncx, 5]: BE, BN, B, the sum of sigma6^2, the pixels with
    sigma6 == 0."""
    sigma6 = np.ascontiguousarray(sigma6, dtype=np.uint8)
    recs = np.ascontiguousarray(recs, dtype=np.int32).reshape(-1, max(ncy, 0), max(ncx, 0), 6)
    assert sigma6.ndim == 2
    rec = np.zeros((max(ncy, 0), max(ncx, 0), 5), np.int64)
    if lib().abh_noise_model_host(sigma6.ctypes.data_as(_u8p), sigma6.shape[1], sigma6.shape[0], int(x0), int(y0), int(ncx), int(ncy),
                                  recs.ctypes.data_as(_i32p) if len(recs) else None, len(recs),
                                  rec.ctypes.data_as(_i64p)) != ncx * ncy or ncx * ncy <= 0:
        raise ValueError(f"the grid {ncx}x{ncy} from ({x0}, {y0}) does not lie inside {sigma6.shape[1]}x{sigma6.shape[0]}")
    return rec


def noise_cell(rec, model):
    """abub::noiseCell: what one cell's record [6] says against its model's [5] -> dict: state (a word of NOISE_STATES),
    q_milli (None where the cell is not rated), all_milli, model_milli."""
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(6)
    model = np.ascontiguousarray(model, dtype=np.int64).reshape(5)
    out = (C.c_longlong * 4)()
    lib().abh_noise_cell(rec.ctypes.data_as(_i32p), model.ctypes.data_as(_i64p), out)
    v = list(out)
    return {"state": NOISE_STATES[v[0]], "q_milli": v[1] if v[0] >= 3 else None, "all_milli": v[2], "model_milli": v[3]}


def noise_frame(rec, model):
    """abub::noiseFrame: what a frame's records [..., 6] say against the model's [..., 5] -> dict: rated, clipped, busy,
    noisy, quiet, kind (a word of NOISE_KINDS), q_milli, q_min, q_max (None where noise.txt has '-') and all_milli."""
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 6)
    model = np.ascontiguousarray(model, dtype=np.int64).reshape(-1, 5)
    assert len(rec) == len(model)
    out = (C.c_longlong * 10)()
    lib().abh_noise_frame(rec.ctypes.data_as(_i32p), model.ctypes.data_as(_i64p), len(rec), out)
    v = list(out)
    none = v[0] == 0
    return {"rated": v[0], "clipped": v[1], "busy": v[2], "noisy": v[3], "quiet": v[4], "kind": NOISE_KINDS[v[5]],
            "q_milli": None if none else v[6], "q_min": None if none else v[7], "q_max": None if none else v[8], "all_milli": v[9]}


LINE_STATES = ("unrated", "rated", "off")
LINES_KINDS = ("blind", "repeated", "torn", "banded", "striped", "steady")


def lines_host(p, mu, r=None):
    """abub::linesHost (host/survey.cpp), the definition of abub_frame_lines_dev: the frame p, the plane mu and the
    reference frame r (None: none), u8 [H, W] -> (rows uint32 [H, 5]: sum p, sum |p - mu|, n_clip, sum |p - r|, n_same;
    cols uint32 [W, 3]: the first three per column)."""
    p, mu = (np.ascontiguousarray(v, dtype=np.uint8) for v in (p, mu))
    r = None if r is None else np.ascontiguousarray(r, dtype=np.uint8)
    assert p.ndim == 2 and p.shape == mu.shape and (r is None or r.shape == p.shape)
    H, W = p.shape
    rows, cols = np.zeros((H, 5), np.uint32), np.zeros((W, 3), np.uint32)
    if lib().abh_lines_host(p.ctypes.data_as(_u8p), None if r is None else r.ctypes.data_as(_u8p), mu.ctypes.data_as(_u8p), W, H,
                            rows.ctypes.data_as(_u32p), cols.ctypes.data_as(_u32p)) != H:
        raise ValueError(f"a frame of {W}x{H} has a side outside [1, 65535]")
    return rows, cols


def lines_model_host(mu, sigma6):
    """abub::linesModelHost: the planes mu and sigma6, u8 [H, W] -> (rows uint32 [H, 3], cols uint32 [W, 3]): sum mu, T = sum
    sigma6, the pixels with sigma6 == 0."""
    mu, sigma6 = (np.ascontiguousarray(v, dtype=np.uint8) for v in (mu, sigma6))
    assert mu.ndim == 2 and mu.shape == sigma6.shape
    H, W = mu.shape
    rows, cols = np.zeros((H, 3), np.uint32), np.zeros((W, 3), np.uint32)
    if lib().abh_lines_model_host(mu.ctypes.data_as(_u8p), sigma6.ctypes.data_as(_u8p), W, H, rows.ctypes.data_as(_u32p),
                                  cols.ctypes.data_as(_u32p)) != H:
        raise ValueError(f"a plane of {W}x{H} has a side outside [1, 65535]")
    return rows, cols


def line_rate(rec, model, N, n, S):
    """abub::lineRate: what one line of N pixels says, from its record (the first three words are read), its model record
    [3], the number n of the frame's rated lines and the sum S of their D -> dict: state (a word of LINE_STATES), num and den
    (e^2 N and (n T)^2 as Python ints; None where the line is unrated).  The line is off when num > 4 den."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1)
    model = np.ascontiguousarray(model, dtype=np.uint32).reshape(3)
    assert rec.size >= 3
    out = (C.c_ulonglong * 4)()
    state = lib().abh_lines_rate(rec.ctypes.data_as(_u32p), model.ctypes.data_as(_u32p), int(N), int(n), int(S), out)
    return {"state": LINE_STATES[state], "num": (out[0] | out[1] << 64) if state else None,
            "den": (out[2] | out[3] << 64) if state else None}


def lines_frame(rows, cols, model_rows, model_cols, has_ref):
    """abub::linesFrame: what a frame's records (rows [H, 5], cols [W, 3]) say against the model's ([H, 3], [W, 3]) -> dict:
    rated_rows, off_rows, stale_rows, first_stale, last_stale, rated_cols, off_cols, first_off_row, last_off_row,
    first_off_col, last_off_col (None where lines.txt has '-'), level_milli, kind (a word of LINES_KINDS), row_state [H] and
    col_state [W] (uint8: 0 unrated, 1 rated, 2 off, 3 stale)."""
    rows, cols, model_rows, model_cols = (np.ascontiguousarray(v, dtype=np.uint32) for v in (rows, cols, model_rows, model_cols))
    H, W = rows.shape[0], cols.shape[0]
    assert rows.shape == (H, 5) and cols.shape == (W, 3) and model_rows.shape == (H, 3) and model_cols.shape == (W, 3)
    out = (C.c_longlong * 13)()
    rs, cs = np.zeros(H, np.uint8), np.zeros(W, np.uint8)
    lib().abh_lines_frame(rows.ctypes.data_as(_u32p), cols.ctypes.data_as(_u32p), model_rows.ctypes.data_as(_u32p),
                          model_cols.ctypes.data_as(_u32p), W, H, int(bool(has_ref)), out, rs.ctypes.data_as(_u8p), cs.ctypes.data_as(_u8p))
    v = list(out)
    keys = ("rated_rows", "off_rows", "stale_rows", "first_stale", "last_stale", "rated_cols", "off_cols", "first_off_row",
            "last_off_row", "first_off_col", "last_off_col")
    res = {k: (None if k.startswith(("first", "last")) and x < 0 else x) for k, x in zip(keys, v)}
    res.update(level_milli=v[11], kind=LINES_KINDS[v[12]], row_state=rs, col_state=cs)
    return res


def zip_write(path, entries):
    """The host writer of the canonical archive (host/zipwrite.cpp) alone: entries, a list of (name, bytes), written to
    `path` in that order; raises where it cannot be written (and leaves no file)."""
    L = lib()
    n = len(entries)
    names = b"".join(name.encode() if isinstance(name, str) else name for name, _ in entries)
    data = b"".join(d for _, d in entries)
    name_len = (C.c_uint32 * max(n, 1))(*[len(name.encode() if isinstance(name, str) else name) for name, _ in entries])
    lens = (C.c_uint64 * max(n, 1))(*[len(d) for _, d in entries])
    nb = (C.c_uint8 * max(len(names), 1)).from_buffer_copy(names or b"\0")
    db = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    if L.abh_zip_write(str(path).encode(), n, nb, name_len, db, lens) != 0:
        raise RuntimeError("abh_zip_write: " + L.abh_zip_error().decode())


def imdecode(data, cap=1 << 22):
    L = lib()
    src = np.frombuffer(data, np.uint8)
    out = np.empty(cap, np.uint8)
    w, h = C.c_int(), C.c_int()
    rc = L.abh_imdecode(src.ctypes.data_as(_u8p), len(src), out.ctypes.data_as(_u8p), cap, C.byref(w), C.byref(h))
    if rc != 0:
        return None
    return out[: w.value * h.value].reshape(h.value, w.value).copy()


def abf_encode(img):
    """cv::abfEncode (host/abf.cpp): an 8-bit grey image [H, W] -> the bytes of its packed file ("ABF1", DESIGN section 3, "Packed frames")."""
    L = lib()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    cap = 64 + 8 * H + H * ((W + 63) // 64) + W * H
    out = np.empty(cap, np.uint8)
    n = L.abh_abf_encode(img.ctypes.data_as(_u8p), W, H, out.ctypes.data_as(_u8p), cap)
    if n < 0 or n > cap:
        raise ValueError(f"abf_encode: a {W} x {H} image cannot be packed")
    return out[:n].tobytes()


def png_huff_encode(img):
    """cv::pngHuffEncode (host/pnghuff.cpp): an 8-bit grey image [H, W] -> the bytes of its canonical Huffman-only PNG
    ("Unpacking a run")."""
    L = lib()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    cap = int(L.abh_png_huff_bound(W, H))
    if cap <= 0:
        raise ValueError(f"png_huff_encode: a {W} x {H} image cannot be written")
    out = np.empty(cap, np.uint8)
    n = L.abh_png_huff_encode(img.ctypes.data_as(_u8p), W, H, out.ctypes.data_as(_u8p), cap)
    if n < 0 or n > cap:
        raise ValueError(f"png_huff_encode: a {W} x {H} image cannot be written")
    return out[:n].tobytes()


def png_huff_lengths(counts, limit):
    """cv::pngHuffLengths: the format's length-limited code lengths of `counts` -> (lengths u8 [n], depth of the unlimited tree)"""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    out = np.zeros(len(c), np.uint8)
    depth = lib().abh_png_huff_lengths(c.ctypes.data_as(C.POINTER(C.c_uint64)), len(c), limit, out.ctypes.data_as(_u8p))
    if depth < 0:
        raise ValueError("png_huff_lengths: bad arguments")
    return out, depth


def abf_decode(data, W, H):
    """cv::abfDecodeStatus: the bytes of a packed file -> (status, image [H, W]); status 0 = decoded, else the code the GPU
    decoder gives the same file (ABUB_ABF_E_*); the image of a refused file may be half written."""
    L = lib()
    src = np.frombuffer(bytes(data) or b"\0", np.uint8)
    out = np.zeros((H, W), np.uint8)
    rc = L.abh_abf_decode(src.ctypes.data_as(_u8p), len(data), out.ctypes.data_as(_u8p), W, H)
    return rc, out


def png_walk(data, W, H, cap=4096):
    """host/pngwalk.hpp::pngWalk: None for a file the GPU decoder does not take, else (IDAT segments [(offset, length)],
    palette -> grey table (bytes) or None)"""
    L = lib()
    src = np.frombuffer(data, np.uint8)
    segs = (C.c_uint32 * (2 * cap))()
    n, pal = C.c_int(), C.c_int()
    lut = np.zeros(256, np.uint8)
    if not L.abh_png_walk(src.ctypes.data_as(_u8p), len(src), W, H, segs, cap, C.byref(n), C.byref(pal), lut.ctypes.data_as(_u8p)):
        return None
    return [(segs[2 * i], segs[2 * i + 1]) for i in range(min(n.value, cap))], (lut.tobytes() if pal.value else None)


def png_walk_typed(data, W, H, cap=4096):
    """pngWalk with typed = true (what ABUB_GPU_PNG_TYPES=1 sends to the GPU decoder): None for a file it does not take, else
    (IDAT segments, palette -> grey table (bytes) or None, kind) with kind = 0 for an 8-bit grey / palette file, else
    colour type | bit depth << 8 (abub_png_frame.kind)"""
    L = lib()
    src = np.frombuffer(data, np.uint8)
    segs = (C.c_uint32 * (2 * cap))()
    n, pal, kind = C.c_int(), C.c_int(), C.c_uint32()
    lut = np.zeros(256, np.uint8)
    if not L.abh_png_walk_typed(src.ctypes.data_as(_u8p), len(src), W, H, segs, cap, C.byref(n), C.byref(pal),
                                lut.ctypes.data_as(_u8p), C.byref(kind)):
        return None
    return ([(segs[2 * i], segs[2 * i + 1]) for i in range(min(n.value, cap))], (lut.tobytes() if pal.value else None),
            int(kind.value))


def png_walk_adam7(data, W, H, typed=False, cap=4096):
    """pngWalk with adam7 = true (what ABUB_GPU_PNG_ADAM7=1 sends to the GPU decoder; typed: ABUB_GPU_PNG_TYPES=1 as well):
    as png_walk_typed, and an Adam7-interlaced file of a kind the walk takes anyway is accepted, its kind with bit 16
    (ABUB_PNG_KIND_ADAM7) set"""
    L = lib()
    src = np.frombuffer(data, np.uint8)
    segs = (C.c_uint32 * (2 * cap))()
    n, pal, kind = C.c_int(), C.c_int(), C.c_uint32()
    lut = np.zeros(256, np.uint8)
    if not L.abh_png_walk_adam7(src.ctypes.data_as(_u8p), len(src), W, H, 1 if typed else 0, segs, cap, C.byref(n), C.byref(pal),
                                lut.ctypes.data_as(_u8p), C.byref(kind)):
        return None
    return ([(segs[2 * i], segs[2 * i + 1]) for i in range(min(n.value, cap))], (lut.tobytes() if pal.value else None),
            int(kind.value))


def bmp_walk(data, W, H):
    """host/bmpwalk.hpp::bmpWalk: None for a file the host decoder does not read as a W x H BMP, else the dict of
    hip.bmp_parse (data_off, stride, bpp, top_down, identity, lut)."""
    L = lib()
    src = np.frombuffer(bytes(data) or b"\0", np.uint8)
    f = (C.c_uint32 * 5)()
    lut = np.zeros(256, np.uint8)
    if not L.abh_bmp_walk(src.ctypes.data_as(_u8p), len(data), W, H, f, lut.ctypes.data_as(_u8p)):
        return None
    return dict(data_off=int(f[0]), stride=int(f[1]), bpp=int(f[2]), top_down=bool(f[3]), identity=bool(f[4]), lut=lut.tobytes())


def imwrite(path, img):
    """cvlite's cv::imwrite (debug image write-out): 8-bit grey PNG, or BMP when the name ends in .bmp."""
    L = lib()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return L.abh_imwrite(path.encode(), img.ctypes.data_as(_u8p), img.shape[1], img.shape[0]) == 0


def write_header(outdir, run_number, frame_offset, ncams):
    """OutputWriter::writeHeader -> <outdir>abub3hs_<run>.txt (outdir is used as a prefix, like upstream)."""
    lib().abh_write_header(outdir.encode(), run_number.encode(), frame_offset, ncams)


def event_to_file(run, event, actual_event_number, ncams, outdir, run_number, frame_offset, maskdir=""):
    """One iteration of the reference's event loop: analyse every camera, append the block to the file."""
    rc = lib().abh_event_to_file(run._h, str(event).encode(), int(actual_event_number), ncams, maskdir.encode(),
                                 outdir.encode(), run_number.encode(), frame_offset)
    if rc != 0:
        raise RuntimeError("abh_event_to_file failed")


def writer_probe(outdir, run_number, frame_offset, event, cams):
    """cams: list of (status, frame0, bubbles) with bubbles = list of descriptor-row lists (11 numbers each)."""
    L = lib()
    n = len(cams)
    status = (C.c_int * n)(*[c[0] for c in cams])
    frame0 = (C.c_int * n)(*[c[1] for c in cams])
    nbub = (C.c_int * n)(*[len(c[2]) for c in cams])
    nd = [len(b) for c in cams for b in c[2]]
    ndesc = (C.c_int * max(1, len(nd)))(*nd)
    rows = [float(v) for c in cams for b in c[2] for d in b for v in d]
    desc = (C.c_double * max(1, len(rows)))(*rows)
    L.abh_writer_probe(outdir.encode(), run_number.encode(), frame_offset, n, event, status, frame0, nbub, ndesc, desc)


# ---- host-logic probes (CPU only) ---------------------------------------------------------------
def contours_from_indices(idx, W, H):
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    npts = np.zeros(4096, np.int32)
    xy = np.zeros((1 << 18, 2), np.int32)
    n = lib().abh_contours(idx.ctypes.data_as(_u32p), len(idx), W, H, npts.ctypes.data_as(_ip),
                           xy.ctypes.data_as(_ip), len(npts), len(xy))
    if n < 0:
        raise RuntimeError("contour probe capacity exceeded")
    out, o = [], 0
    for k in range(n):
        out.append(xy[o:o + npts[k]].copy())
        o += npts[k]
    return out


def binarize_threshold(hist, P, tozero):
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    return int(lib().abh_binarize_threshold(hist.ctypes.data_as(_u32p), int(P), int(tozero)))


def entropy(hist, nbins, P):
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    return float(lib().abh_entropy(hist.ctypes.data_as(_u32p), nbins, int(P)))


def blob_stats(xy):
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    out = (C.c_double * 8)()
    lib().abh_blob_stats(xy.ctypes.data_as(_ip), len(xy), out)
    return dict(zip(("x", "y", "w", "h", "area", "m00", "m10", "m01"), list(out)))


def best_match(num, wsum2, tmpl):
    L = lib()
    num = np.ascontiguousarray(num, dtype=np.uint64)
    wsum2 = np.ascontiguousarray(wsum2, dtype=np.uint64)
    tmpl = np.ascontiguousarray(tmpl, dtype=np.uint8)
    rh, rw = num.shape
    bx, by = C.c_float(), C.c_float()
    L.abh_best_match(num.ctypes.data_as(_u64p), wsum2.ctypes.data_as(_u64p), rw, rh, tmpl.ctypes.data_as(_u8p),
                     tmpl.shape[1], tmpl.shape[0], C.byref(bx), C.byref(by))
    return bx.value, by.value


def localize_totals():
    """(stacks localised on the device, stacks on the host route) with the "localize" knob on, over every pipeline run of
    this process so far -- see trigger_totals()."""
    out = (C.c_double * 2)()
    lib().abh_pipe_localize_totals(out)
    return int(out[0]), int(out[1])


def trigger_totals():
    """(stacks searched on the device, stacks on the host route) with the "trigger" knob on, over every pipeline run of
    this process so far -- Run.run_batched owns its pipelines, so a caller takes the difference around it."""
    out = (C.c_double * 2)()
    lib().abh_pipe_trigger_totals(out)
    return int(out[0]), int(out[1])


class Significance:
    def __init__(self, tss):
        self._h = lib().abh_sig_new()
        self.tss = tss
        self.loc_thres = C.c_int(3)

    def __call__(self, hist, P, store):
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        return float(lib().abh_sig_eval(self._h, hist.ctypes.data_as(_u32p), int(P), 1 if store else 0, self.tss,
                                        C.byref(self.loc_thres)))

    def __del__(self):
        try:
            lib().abh_sig_free(self._h)
        except Exception:
            pass


class Pipeline:
    """Run-level batched detect over an HBM-resident slab [E][C][F][H][W] (host/pipeline.cpp)."""

    def __init__(self, device, W, H, F, E, ncams, tss, nthreads=16, maskdir=""):
        L = lib()
        t = (C.c_int * len(tss))(*tss)
        self.S = E * ncams
        self._h = L.abh_pipe_new(device, W, H, F, E, ncams, t, nthreads, maskdir.encode())
        if not self._h:
            raise RuntimeError("abh_pipe_new failed (see stderr)")

    def close(self):
        if self._h:
            lib().abh_pipe_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sigma(self, sigma):
        """sigma image(s) (not 6 sigma) on the device: needed only by stacks that fall back to the drop-in path."""
        lib().abh_pipe_set_sigma(self._h, sigma.data_ptr() if hasattr(sigma, "data_ptr") else int(sigma))

    def run(self, frames, mu, sigma6, stream=0, sigma=None):
        """frames/mu/sigma6 (and optionally sigma, needed only if a stack falls back to the drop-in path for the
        bellows veto): device pointers (ints) or torch tensors."""
        p = [x.data_ptr() if hasattr(x, "data_ptr") else int(x) for x in (frames, mu, sigma6)]
        if sigma is not None:
            self.set_sigma(sigma)
        rc = lib().abh_pipe_run(self._h, p[0], p[1], p[2], stream)
        if rc != 0:
            raise RuntimeError("pipeline: " + lib().abh_pipe_error().decode())

    def run_host(self, frames_host, mu, sigma6):
        """Streamed mode: `frames_host` is a HOST tensor / pointer ([E][C][F][H][W], pinned for full PCIe rate);
        stack groups are uploaded and processed in a pipeline."""
        L = lib()
        p =[x.data_ptr() if hasattr(x, "data_ptr") else int(x) for x in (frames_host, mu, sigma6)]
        if L.abh_pipe_run_host(self._h, p[0], p[1], p[2]) != 0:
            raise RuntimeError("pipeline: " + L.abh_pipe_error().decode())

    def timing(self):
        out = (C.c_double * 12)()
        rounds = lib().abh_pipe_timing(self._h, out)
        return dict(zip(("stage1_ms", "stage2_ms", "stage3_ms", "stage4_ms", "total_ms", "s3_gpu_ms", "s3_list_ms",
                         "s3_bucket_ms", "pairs", "trigger_jobs", "dropin_stacks", "jobs_completed_on_demand"), list(out)),
                    rounds=rounds)

    def set_option(self, name, value):
        """Run-time knob of this pipeline object: "blobs" 0 (default, from ABUB_PIPE_BLOBS) or 1 -- label the foreground on
        the GPU and ship only the pixels of the components the localizer can use; "contours" 0 (default, from
        ABUB_PIPE_CONTOURS) or 1 -- also trace the contours of those components on the GPU (K5) and ship their vertices,
        whatever "blobs" says; "trigger" 0 (default, from ABUB_PIPE_TRIGGER) or 1 -- run the trigger search of every
        stack inside the kernel's limits on the GPU (K6) from the histograms that are already there, instead of
        FindTriggerFrame on host threads; read at the start of a run; "localize" 0 (default, from ABUB_PIPE_LOCALIZE) or 1
        -- also describe the contours and run the localizer's decisions per stack on the GPU (K7), whatever "contours"
        and "blobs" say; a stack the kernels decline keeps the host route.  Results never depend on them."""
        L = lib()
        if L.abh_pipe_set_option(self._h, name.encode(), int(value)) != 0:
            raise ValueError(L.abh_pipe_error().decode())

    def blob_stats(self):
        """Blob labelling of the last run (zeros when the "blobs" knob was off), summed over stack groups and rounds."""
        out = (C.c_double * 8)()
        lib().abh_pipe_blob_stats(self._h, out)
        v = list(out)
        keys = ("candidates", "foreground", "kept", "components", "kept_components", "large_slots")
        d = {k: int(x) for k, x in zip(keys, v)}
        d.update(otsu_ms=v[6], k4b_ms=v[7])
        return d

    def contour_stats(self):
        """Contour tracing of the last run (zeros when the "contours" knob was off), summed over stack groups and rounds:
        slots traced on the device, slots left to the host route, contours, vertices, ms of the K5 launches."""
        out = (C.c_double * 5)()
        lib().abh_pipe_contour_stats(self._h, out)
        v = list(out)
        d = {k: int(x) for k, x in zip(("traced", "host_route", "contours", "vertices"), v)}
        d["k5_ms"] = v[4]
        return d

    def localize_stats(self):
        """Device localizer of the last run (zeros when the "localize" knob was off), summed over stack groups and rounds:
        stacks localised on the device; stacks on the host route (host_route, and by reason: over a limit, with a declined
        slot or an undecodable frame, with every genesis contour in the bellows mask, other: an Otsu mismatch); bubbles and
        descriptors of the device's tracks; ms of the K7 launches; list_bytes: what stage 3 copied to the host of the kept-pixel,
        contour, vertex, record, box and track lists (counted with the "contours" knob alone, too); regrows: batches redone
        because the record list, or the box and track lists, had to grow."""
        out = (C.c_double * 10)()
        lib().abh_pipe_localize_stats(self._h, out)
        v = list(out)
        keys = ("device", "host_limits", "host_slot", "host_bellows", "host_other", "bubbles", "descriptors")
        d = {k: int(x) for k, x in zip(keys, v)}
        d["host_route"] = d["host_limits"] + d["host_slot"] + d["host_bellows"] + d["host_other"]
        d["k7_ms"] = v[7]
        d["list_bytes"] = int(v[8])
        d["regrows"] = int(v[9])
        return d

    def trigger_stats(self):
        """Device trigger search of the last run (zeros when the "trigger" knob was off), summed over stack groups and
        rounds: stacks searched on the device, stacks on the host route (beyond the kernel's limits), search launches,
        NEED_FRAMES answers, NEED_FINAL answers, ms of the K6 launches."""
        out = (C.c_double * 6)()
        lib().abh_pipe_trigger_stats(self._h, out)
        v = list(out)
        d = {k: int(x) for k, x in zip(("device", "host_route", "launches", "need_frames", "need_final"), v)}
        d["k6_ms"] = v[5]
        return d

    def bellows_stats(self):
        """Bellows veto of the last run: stacks vetoed inside the batch, template-match jobs and launches, residual
        images, wall time of the veto rounds (ms)."""
        out = (C.c_double * 5)()
        lib().abh_pipe_bellows(self._h, out)
        v = list(out)
        return {"vetoed": int(v[0]), "match_jobs": int(v[1]), "match_launches": int(v[2]), "residual_images": int(v[3]),
                "veto_ms": v[4]}

    def result(self, s):
        return _read_result(lib().abh_pipe_stack(self._h, s), with_dz=False)

    def rects(self, s):
        """the boxes (x, y, w, h) of stack s's last localizer round (StackResult::rects)"""
        return _read_rects(lib().abh_pipe_stack(self._h, s))

    def summary(self):
        """(staged, trig, nbubbles) for every stack -- cheap fingerprint of a run."""
        L = lib()
        o = (C.c_int * 6)()
        out = []
        for s in range(self.S):
            L.abh_result_state(L.abh_pipe_stack(self._h, s), o)
            out.append((o[0], o[1], o[5]))
        return out


class PipelineRing:
    """N pipeline objects, each driven by its own host thread: batch k runs on pipeline k % N, so the host stages of
    one batch (trigger state machines, contour tracing, tracking) run while the GPU is busy with the kernels of the
    next.  Every batch still goes through the complete path; only their stages interleave.  N = 1 is a plain loop."""

    def __init__(self, n, device, W, H, F, E, ncams, tss, nthreads=16, maskdir=""):
        self.device = device
        self.pipes = [Pipeline(device, W, H, F, E, ncams, tss, nthreads=nthreads, maskdir=maskdir) for _ in range(max(1, n))]

    def close(self):
        for p in self.pipes:
            p.close()

    def run_batches(self, batches, mu, sigma6, stream=0, on_done=None, host=False):
        """batches: sequence of frame slabs (device tensors / pointers, each [E][C][F][H][W]); with host=True they are
        HOST slabs (pinned for full PCIe rate) and every pipeline streams its batch in (Pipeline.run_host), so the upload
        of one run overlaps the detect stages of the previous one (BASELINE configs[4]: many runs streamed host -> HBM).
        Returns the per-batch timing dicts in completion order; `on_done(k, pipeline)` is called on the driving thread
        right after batch k finished, while its results are still the pipeline's current ones."""
        import threading

        n = len(self.pipes)
        tms, errs = [], []
        lock = threading.Lock()

        def drive(i):
            try:
                try:
                    import torch

                    torch.cuda.set_device(self.device)
                except ImportError:
                    pass
                for k in range(i, len(batches), n):
                    if host:
                        self.pipes[i].run_host(batches[k], mu, sigma6)
                    else:
                        self.pipes[i].run(batches[k], mu, sigma6, stream)
                    if on_done:
                        on_done(k, self.pipes[i])
                    with lock:
                        tms.append(self.pipes[i].timing())
            except BaseException as e:  # noqa: BLE001 -- re-raised on the caller's thread
                errs.append(e)

        if n == 1:
            drive(0)
        else:
            th = [threading.Thread(target=drive, args=(i,)) for i in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        if errs:
            raise errs[0]
        return tms
