"""The GPU BMP decoder on the CPU side: abub_bmp_decode_dev is declared, exported and bound, its descriptor is the 32
bytes the header states, it validates its arguments before anything touches a device, and there is no host fall-back."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bmpfiles
from autobub3hs_amd import _lib, hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


class BmpFrame(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint32), ("len", ctypes.c_uint32), ("data_off", ctypes.c_uint32), ("stride", ctypes.c_uint32),
                ("bpp", ctypes.c_uint16), ("flags", ctypes.c_uint16), ("lut", ctypes.c_uint32), ("dst", ctypes.c_uint64)]


def test_decoder_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_bmp_decode_dev(const uint8_t *files, size_t files_bytes, const abub_bmp_frame *frames, int nframes," in hdr
    assert "typedef struct abub_bmp_frame {" in hdr and "} abub_bmp_frame;" in hdr
    assert "#define ABUB_BMP_E_DESC 1 " in hdr
    assert "RawParser.cpp:34-47" in hdr and "ZipParser.cpp:186-239" in hdr  # the reference lines it replaces
    for field in ("uint32_t off, len;", "uint32_t data_off;", "uint32_t stride;", "uint16_t bpp, flags;", "uint32_t lut;", "uint64_t dst;"):
        assert field in hdr.split("typedef struct abub_bmp_frame {")[1].split("} abub_bmp_frame;")[0], field
    assert ctypes.sizeof(BmpFrame) == 32 and BmpFrame.dst.offset == 24 and BmpFrame.lut.offset == 20
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_bmp_decode_dev") and "abub_bmp_decode_dev" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["abub_bmp_decode_dev"][1]) == 12
    assert callable(hip.bmp_decode) and callable(hip.bmp_parse) and callable(host.bmp_walk)
    assert hasattr(ctypes.CDLL(host.SO), "abh_bmp_walk") and "abh_bmp_walk" in host.SIGNATURES
    assert "abub_bmp.hip" in open(os.path.join(ROOT, "autobub3hs_amd", "csrc", "Makefile")).read()


def test_decoder_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    ok = dict(files=p, files_bytes=2048, frames=p, nframes=1, luts=p, nluts=1, W=8, H=2, out=p, out_bytes=4096, status=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_bmp_decode_dev(a["files"], a["files_bytes"], a["frames"], a["nframes"], a["luts"], a["nluts"], a["W"], a["H"],
                                     a["out"], a["out_bytes"], a["status"], a["stream"])

    bad = [dict(files=None), dict(frames=None), dict(out=None), dict(status=None), dict(luts=None), dict(luts=None, nluts=3),
           dict(nframes=-1), dict(nluts=-1), dict(W=0), dict(H=0), dict(W=65536), dict(H=65536), dict(W=-4), dict(H=-1)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_bmp_decode_dev" in L.abub_last_error(), kw
    assert not any(buf)


def test_no_frames_is_ok_and_touches_nothing():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
    p = ctypes.addressof(buf)
    assert L.abub_bmp_decode_dev(p, 256, p, 0, None, 0, 8, 2, p, 256, p, None) == 0
    assert L.abub_bmp_decode_dev(p, 256, p, 0, p, 1, 65535, 65535, p, 256, p, None) == 0
    assert bytes(buf) == bytes([0x5A]) * 256


def test_no_host_fallback():
    """a CPU tensor is refused by the wrapper; without a device a launch is an error and writes nothing"""
    W, H = 8, 2
    data = bmpfiles.make_bmp(np.arange(16).reshape(H, W), 8)
    info = hip.bmp_parse(data, W, H)
    files = torch.frombuffer(bytearray(data + bytes(-len(data) % 16)), dtype=torch.uint8)
    out = torch.full((W * H,), 0x5A, dtype=torch.uint8)
    desc = [(0, len(data), info["data_off"], info["stride"], 8, 0, 0xFFFFFFFF, 0)]
    with pytest.raises(_lib.AbubError, match="no CPU fallback"):
        hip.bmp_decode(files, desc, None, W, H, out)
    assert bool((out == 0x5A).all())
    if torch.cuda.is_available():
        return
    L = _lib.lib()
    assert L.abub_device_count() == 0
    fr = BmpFrame(0, len(data), info["data_off"], info["stride"], 8, 0, 0xFFFFFFFF, 0)
    status = (ctypes.c_int32 * 1)(77)
    rc = L.abub_bmp_decode_dev(files.data_ptr(), files.numel(), ctypes.addressof(fr), 1, None, 0, W, H, out.data_ptr(), out.numel(),
                               ctypes.addressof(status), None)
    assert rc != 0 and rc != E_INVALID
    assert bool((out == 0x5A).all()) and status[0] == 77
