"""CPU-side checks of the contour tracing kernel's entries (K5, abub_contours.hip) and its pipeline knob: declared, exported
and bound; sizes and limits answer without a device; bad arguments and bad knob values are refused before the device."""
import ctypes as C
import os
import re

import pytest

from autobub3hs_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("abub_trace_contours_dev", "abub_trace_contours_scratch_bytes", "abub_trace_contours_limits")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def test_new_entries_declared_exported_and_bound():
    from autobub3hs_amd import hip

    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(_lib.build())
    for name in NEW:
        m = re.search(r"\b%s\s*\(" % name, txt)
        assert m, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        # the comment in front of the declaration cites the reference's contour calls
        before = hdr[:hdr.index(name + "(")]
        assert "L3Localizer.cpp:264, 374, 793" in before[before.rindex("/*"):], name
    assert callable(hip.trace_contours) and callable(hip.trace_contours_limits)
    assert "abh_pipe_contour_stats" in host.SIGNATURES and callable(host.Pipeline.contour_stats)


def test_scratch_size_and_limits_need_no_device():
    lib = _lib.lib()
    assert lib.abub_trace_contours_scratch_bytes(10, 1 << 20) > 0
    assert lib.abub_trace_contours_scratch_bytes(0, 1 << 20) == 0
    assert lib.abub_trace_contours_scratch_bytes(-3, 16) == 0
    mp, mc = C.c_int(-1), C.c_int(-1)
    assert lib.abub_trace_contours_limits(C.byref(mp), C.byref(mc)) == 0
    assert mp.value == 2048
    assert mc.value >= 1024
    assert lib.abub_trace_contours_limits(None, None) == 0


def test_trace_contours_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    z = C.c_void_p(0)
    one = C.c_void_p(256)  # never dereferenced: every call below is refused while the arguments are checked
    # (kept_off, kept_idx, in_cap, nslots, W, H, status, ncont, cont_off, cont_npts, cont_cap, pt_off, pts, pts_cap, stats,
    #  scratch, scratch_bytes, stream)
    good = [one, one, 16, 4, 64, 64, one, one, one, one, 16, one, one, 64, one, one, 1 << 20, None]
    for pos, bad in ((0, z), (1, z), (6, z), (9, z), (12, z), (14, z), (15, z),  # null pointers
                     (2, 0), (3, 0), (3, -1), (4, 0), (5, 0), (4, 65536), (5, 65536), (10, 0), (13, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.abub_trace_contours_dev(*args) == -1, pos
        assert b"bad arguments" in lib.abub_last_error(), pos
    args = list(good)
    args[16] = 8  # scratch too small
    assert lib.abub_trace_contours_dev(*args) == -1
    assert b"scratch" in lib.abub_last_error()
    args = list(good)
    args[15] = C.c_void_p(264)  # scratch not 256-byte aligned
    assert lib.abub_trace_contours_dev(*args) == -1
    assert b"scratch" in lib.abub_last_error()


def test_pipeline_option_contours_is_known_and_validated():
    L = host.lib()
    L.abh_pipe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.abh_pipe_error.restype = C.c_char_p
    assert L.abh_pipe_set_option(None, b"contours", 1) == -1  # valid name and value, but no pipeline
    assert b"no pipeline" in L.abh_pipe_error()
    assert b"unknown option" not in L.abh_pipe_error()
    for v in (-1, 2):
        assert L.abh_pipe_set_option(None, b"contours", v) == -1
        assert b"0 or 1" in L.abh_pipe_error()
