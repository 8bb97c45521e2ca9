"""The GPU encoder of the canonical Huffman-only PNG on the CPU side: abub_png_encode_dev and its sizing helpers are
declared, exported, bound and validate their arguments without a device; abub_png_file_bound against the format's formula;
and --unpack-gpu / Run.unpack(device=...) refuse to run without a device instead of encoding on the host."""
import ctypes
import os
import subprocess

import pytest
import torch

import pnghuffref as ref
from autobub3hs_amd import _lib, hip, host
from test_abf_format import make_run_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
RUN_ID = "20200925_1"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def test_encoder_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_png_encode_dev(" in hdr and "cv::pngHuffEncode" in hdr
    assert "size_t abub_png_file_bound(int W, int H);" in hdr
    assert "size_t abub_png_encode_scratch_bytes(int nframes, int W, int H);" in hdr
    L = ctypes.CDLL(_lib.build())
    for name in ("abub_png_file_bound", "abub_png_encode_scratch_bytes", "abub_png_encode_dev"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["abub_png_encode_dev"] == _lib.SIGNATURES["abub_abf_encode_dev"]  # (the same conventions)
    assert callable(hip.png_encode)
    for name in ("abh_png_huff_encode", "abh_run_unpack", "abh_run_unpack_dev"):
        assert hasattr(host.lib(), name), name


def test_encoder_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    need = L.abub_png_encode_scratch_bytes(1, 8, 2)
    assert 0 < need <= 8192 and need % 16 == 0
    ok = dict(pixels=p, pixels_bytes=64, src=p, nframes=1, W=8, H=2, out=p, out_cap=8192, files=p, total=p, scratch=p,
              scratch_bytes=8192, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_png_encode_dev(a["pixels"], a["pixels_bytes"], a["src"], a["nframes"], a["W"], a["H"], a["out"], a["out_cap"],
                                     a["files"], a["total"], a["scratch"], a["scratch_bytes"], a["stream"])

    bad = [dict(pixels=None), dict(src=None), dict(out=None), dict(files=None), dict(total=None), dict(scratch=None),
           dict(nframes=-1), dict(W=0), dict(H=0), dict(W=65536), dict(H=65536), dict(W=-4),
           dict(W=65535, H=65535, scratch_bytes=1 << 40),  # abub_png_file_bound == 0
           dict(scratch_bytes=need - 1), dict(scratch_bytes=0),
           dict(scratch=p + 4), dict(src=p + 4), dict(files=p + 2), dict(total=p + 1)]  # misaligned
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_png_encode_dev" in L.abub_last_error(), kw
    assert call(nframes=0) == 0  # nothing to do, nothing touched
    assert not any(buf)
    assert L.abub_png_encode_scratch_bytes(-1, 8, 2) == 0 and L.abub_png_encode_scratch_bytes(1, 0, 2) == 0
    assert L.abub_png_encode_scratch_bytes(1, 65535, 65535) == 0
    assert L.abub_png_encode_scratch_bytes(0, 8, 2) <= L.abub_png_encode_scratch_bytes(300, 64, 3)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 40), (2, 33), (3, 5), (7, 65), (64, 3), (129, 3), (1280, 1024), (1680, 1050), (65535, 1),
                                 (1, 65535), (65535, 34952)])
def test_file_bound_is_the_formula(W, H):
    L = _lib.lib()
    want = 63 + (1880 + 15 * (H * (W + 1) + 1) + 7) // 8
    assert want < 1 << 32
    assert L.abub_png_file_bound(W, H) == want == ref.file_bound(W, H) == host.lib().abh_png_huff_bound(W, H)


def test_file_bound_is_zero_from_4_gb_on_and_outside_the_sizes():
    L = _lib.lib()
    # 65535 x 34953 is the first height at which the bound reaches 2^32
    assert 63 + (1880 + 15 * (34953 * 65536 + 1) + 7) // 8 >= 1 << 32 > 63 + (1880 + 15 * (34952 * 65536 + 1) + 7) // 8
    for W, H in ((65535, 34953), (65535, 65535), (0, 4), (4, 65536), (65536, 4), (4, 0), (-1, 4)):
        assert L.abub_png_file_bound(W, H) == 0 == ref.file_bound(W, H), (W, H)
        assert host.lib().abh_png_huff_bound(W, H) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: the device route is tested in test_gpu_png_encode.py")
def test_unpack_gpu_is_refused_without_a_device(tmp_path):
    """there is no silent fall-back to the host route (as test_abi.test_no_cpu_fallback_without_device)"""
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="2")
    rd, _ = make_run_dir(str(tmp_path / "data"), F=2, nev=1)
    data = os.path.dirname(rd)
    out = str(tmp_path / "unpacked")
    r = subprocess.run([exe, "-d", data, "-r", RUN_ID, "--unpack", out, "--unpack-gpu"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "no such HIP device" in r.stderr, r.stdout + r.stderr
    assert not [f for _, _, fs in os.walk(out) for f in fs], "a file was written"
    run = host.Run("raw", rd + "/", "Images")
    try:
        with pytest.raises(RuntimeError, match="no such HIP device"):
            run.unpack(str(tmp_path / "unpacked2" / RUN_ID), nthreads=2, ncams=2, device=0)
        assert not os.path.exists(str(tmp_path / "unpacked2"))
        st = run.unpack(str(tmp_path / "unpacked3" / RUN_ID), nthreads=2, ncams=2)  # device=None: the host route
        assert st["packed"] == 4 and set(st) == {"packed", "copied", "failed", "bytes_in", "bytes_out", "seconds"}
    finally:
        run.close()
