"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/abub_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

from autobub3hs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(abub_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_every_declared_symbol():
    so = _lib.build()
    L = ctypes.CDLL(so)
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/abub_hip.h but not exported"
    # and the Python signature table covers exactly the header
    assert sorted(_lib.SIGNATURES) == syms


def test_no_cpu_fallback_without_device():
    import torch

    from autobub3hs_amd import hip

    if torch.cuda.is_available():
        return
    L = _lib.lib()
    assert L.abub_device_count() == 0
    h = ctypes.c_void_p()
    rc = L.abub_ctx_create(ctypes.byref(h), 0, 64, 64, 4)
    assert rc == -3 and b"no such HIP device" in L.abub_last_error()
    t = torch.zeros((4, 4), dtype=torch.uint8)
    try:
        hip.sigma6(t)
        raise AssertionError("CPU tensor must be refused")
    except _lib.AbubError:
        pass


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "autobub3hs_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                src = open(os.path.join(dp, f), errors="replace").read()
                assert "pyoracle" not in src and "abub_oracle" not in src and "liboracle" not in src, f


def test_option_setters_refuse_bad_names_and_values():
    """abub_k2_set_option / abub_k3_set_option validate before anything else (no device needed): unknown and null
    names and out-of-range values are refused with ABUB_E_INVALID and leave the options as they were."""
    L = _lib.lib()
    for setter in (L.abub_k2_set_option, L.abub_k3_set_option):
        assert setter(None, 1) == -1
        assert b"null name" in L.abub_last_error()
        assert setter(b"no_such_option", 1) == -1
        assert b"unknown option" in L.abub_last_error()
        assert setter(b"chunks", -1) == -1 and setter(b"chunks", 4097) == -1
    for name, value in ((b"scan", 2), (b"scan", -1), (b"list", 2), (b"budget", -1), (b"budget", 513), (b"pf", 1)):
        assert L.abub_k3_set_option(name, value) == -1, name
    assert L.abub_k2_set_option(b"budget", 0) == -1


def test_context_calls_refuse_null_arguments_before_the_device():
    """Every abub_ctx_* call validates its pointers before it touches the device: a NULL context, and a NULL among the
    buffers a call needs, give ABUB_E_INVALID and a text for abub_last_error().  No device needed."""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()  # stands for any host buffer; never read or written by a refused call
    B = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 2)(B, B)
    n = ctypes.c_int(-7)
    # a context without frames and without a model: all fields zero (also max_frames, so nothing fits in it)
    blank = (ctypes.c_uint8 * 4096)()
    X = ctypes.addressof(blank)

    def refused(name, *args):
        assert L.abub_k3_set_option(b"scan", 1) == 0  # (a successful call in between does not clear the text ...)
        assert L.abub_k2_set_option(None, 0) == -1    # (... so put a different one there first)
        assert b"null name" in L.abub_last_error()
        assert getattr(L, name)(*args) == -1, name
        err = L.abub_last_error()
        assert name.encode() in err or b"frame index" in err or b"no model" in err, (name, err)

    for ctx in (None, X):
        # with ctx = NULL every argument is otherwise valid; with the blank context one other pointer is NULL
        null = (lambda v: v) if ctx is None else (lambda v: None)
        refused("abub_ctx_train", ctx, null(ptrs), 2, B, B)
        refused("abub_ctx_train", ctx, ptrs, 2, null(B), B)
        refused("abub_ctx_train", ctx, ptrs, 2, B, null(B))
        refused("abub_ctx_pair_hist", ctx, null(B), B, B)
        refused("abub_ctx_pair_hist", ctx, B, null(B), B)
        refused("abub_ctx_pair_hist", ctx, B, B, null(B))
        refused("abub_ctx_set_model", ctx, null(B), B)
        refused("abub_ctx_set_model", ctx, B, null(B))
        refused("abub_ctx_upload_stack", ctx, null(ptrs), 2)
        refused("abub_ctx_diff_hist_batch", ctx, 1, 0, 0, null(B))
        refused("abub_ctx_foreground", ctx, 0, null(B), 16, ctypes.byref(n))
        refused("abub_ctx_foreground", ctx, 0, B, 16, None if ctx else ctypes.byref(n))
        refused("abub_ctx_match_template", ctx, 0, null(B), 1, 1, B, B)
        refused("abub_ctx_match_template", ctx, 0, B, 1, 1, null(B), B)
        refused("abub_ctx_match_template", ctx, 0, B, 1, 1, B, null(B))
        refused("abub_ctx_subtract_image", ctx, null(B), B)
        refused("abub_ctx_set_image", ctx, null(B))
        refused("abub_ctx_fetch_image", ctx, null(B))
    # calls whose outputs may be NULL: the NULL context, and on the blank context no frame index is in range
    for ctx in (None, X):
        refused("abub_ctx_diff_frame", ctx, 0, 0, B, B)
        refused("abub_ctx_diff_frame_roi", ctx, 0, 0, 0, 0, 1, 1, B, B)
        refused("abub_ctx_posttrig", ctx, 0, B, B)
    # null pointers among the frames, and a count the blank context cannot hold
    refused("abub_ctx_train", X, (ctypes.c_void_p * 3)(B, None, B), 3, B, B)
    refused("abub_ctx_train", X, ptrs, 0, B, B)
    refused("abub_ctx_upload_stack", X, ptrs, 2)
    refused("abub_ctx_foreground", X, 0, B, 0, ctypes.byref(n))
    assert n.value == -7 and not any(buf) and not any(blank)
    refused("abub_ctx_create", None, 0, 64, 64, 4)
    h = ctypes.c_void_p()
    for W, H, F in ((0, 64, 4), (64, 0, 4), (64, 64, 0), (-1, 64, 4)):
        refused("abub_ctx_create", ctypes.byref(h), 0, W, H, F)
        assert not h.value
    L.abub_ctx_destroy(None)  # a no-op
