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
