"""The GPU encoder of the packed frame format on the CPU side: abub_abf_encode_dev and its sizing helpers are declared,
exported, bound and validate their arguments without a device; abub_abf_file_bound against the numpy restatement of the
format (tests/abfref.py); and --repack-gpu / Run.repack(device=...) refuse to run without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import abfref
from autobub3hs_amd import _lib, hip, host, synth
from test_abf_format import all_contents, make_run_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1), (2, 1), (63, 2), (64, 3), (65, 3), (127, 2), (128, 9), (129, 9), (257, 9), (1280, 9), (2050, 2), (4100, 1)]  # W x H
E_INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def sources():
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = synth.render_event(320, 128, spec, 300, 0)[spec.F - 1]
    return {"sample": sample, "synth": np.ascontiguousarray(frame)}


def worst(W, H):
    """every difference is +-128, which zigzags to 255: every block 8 bits wide"""
    return np.ascontiguousarray(np.broadcast_to((128 * (np.arange(W) & 1)).astype(np.uint8), (H, W)))


def test_encoder_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_abf_encode_dev(" in hdr and "typedef struct abub_abf_file {" in hdr and "cv::abfEncode" in hdr
    assert "size_t abub_abf_file_bound(int W, int H);" in hdr
    assert "size_t abub_abf_encode_scratch_bytes(int nframes, int W, int H);" in hdr
    assert "#define ABUB_ABF_ENC_E_SRC 1 " in hdr and "#define ABUB_ABF_ENC_E_CAP 2 " in hdr
    L = ctypes.CDLL(_lib.build())
    for name in ("abub_abf_file_bound", "abub_abf_encode_scratch_bytes", "abub_abf_encode_dev"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert callable(hip.abf_encode)


def test_encoder_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    need = L.abub_abf_encode_scratch_bytes(1, 8, 2)
    assert 0 < need <= 4096
    ok = dict(pixels=p, pixels_bytes=64, src=p, nframes=1, W=8, H=2, out=p, out_cap=4096, files=p, total=p, scratch=p,
              scratch_bytes=4096, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_abf_encode_dev(a["pixels"], a["pixels_bytes"], a["src"], a["nframes"], a["W"], a["H"], a["out"], a["out_cap"],
                                     a["files"], a["total"], a["scratch"], a["scratch_bytes"], a["stream"])

    bad = [dict(pixels=None), dict(src=None), dict(out=None), dict(files=None), dict(total=None), dict(scratch=None),
           dict(nframes=-1), dict(W=0), dict(H=0), dict(W=65536), dict(H=65536), dict(W=-4),
           dict(W=65535, H=65535, scratch_bytes=1 << 40),  # abub_abf_file_bound == 0
           dict(scratch_bytes=need - 1), dict(scratch_bytes=0)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_abf_encode_dev" in L.abub_last_error(), kw
    assert call(nframes=0) == 0  # nothing to do, nothing touched
    assert not any(buf)
    assert L.abub_abf_encode_scratch_bytes(-1, 8, 2) == 0 and L.abub_abf_encode_scratch_bytes(1, 0, 2) == 0
    assert L.abub_abf_encode_scratch_bytes(0, 8, 2) <= L.abub_abf_encode_scratch_bytes(300, 64, 3)


@pytest.mark.parametrize("W,H", SHAPES)
def test_file_bound_is_the_largest_file(sources, W, H):
    L = _lib.lib()
    bound = L.abub_abf_file_bound(W, H)
    nblk = (W + 63) // 64
    assert bound == 32 + 8 * H + ((H * nblk + 3) & ~3) + W * H
    ref = abfref.encode(worst(W, H))
    assert bound == len(ref)
    assert host.abf_encode(worst(W, H)) == ref
    for name, img in all_contents(sources, W, H, seed=W).items():
        assert len(abfref.encode(img)) <= bound, name


def test_file_bound_refuses_what_the_header_cannot_hold():
    L = _lib.lib()
    for W, H in ((65535, 65535), (0, 4), (4, 65536), (65536, 4), (4, 0), (-1, 4)):
        assert L.abub_abf_file_bound(W, H) == 0, (W, H)
    assert L.abub_abf_file_bound(65535, 1) == 32 + 8 + 1024 + 65535


def test_repack_gpu_is_refused_without_a_device(tmp_path):
    """there is no silent fall-back to the host route (as test_abi.test_no_cpu_fallback_without_device)"""
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="2")
    r = subprocess.run([exe, "-h"], env=env, capture_output=True, text=True)
    assert "--repack-gpu" in r.stdout
    rd, _ = make_run_dir(str(tmp_path / "data"), F=2, nev=1)
    data = os.path.dirname(rd)
    # the flag alone is refused, device or not
    r = subprocess.run([exe, "-d", data, "-r", "20200925_1", "-o", str(tmp_path), "--repack-gpu"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "--repack-gpu is valid only together with --repack" in r.stderr, r.stderr
    if torch.cuda.is_available():
        return
    out = str(tmp_path / "packed")
    r = subprocess.run([exe, "-d", data, "-r", "20200925_1", "--repack", out, "--repack-gpu"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "no such HIP device" in r.stderr, r.stdout + r.stderr
    assert not [f for _, _, fs in os.walk(out) for f in fs], "a file was written"
    run = host.Run("raw", rd + "/", "Images")
    try:
        with pytest.raises(RuntimeError, match="no such HIP device"):
            run.repack(str(tmp_path / "packed2" / "20200925_1"), nthreads=2, ncams=2, device=0)
        assert not os.path.exists(str(tmp_path / "packed2"))
        st = run.repack(str(tmp_path / "packed3" / "20200925_1"), nthreads=2, ncams=2)  # device=None: the host route as before
        assert st["packed"] == 4 and set(st) == {"packed", "copied", "failed", "bytes_in", "bytes_out", "seconds"}
    finally:
        run.close()
