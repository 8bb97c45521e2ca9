"""abub_peek_planes_dev on the CPU side: the entry is declared, exported and bound, its records have the layout of the
header, it validates its arguments before anything touches a device, and there is no fall-back without one; the numpy
restatement of tests/peekref.py, which the GPU tests hold the kernel against, agrees with cv::rectangle drawn by hand and
with the host route's planes (peekPlanesHost) on a handful of shapes; abub3hs refuses --peek with the modes it does not
belong to."""
import ctypes
import os
import re

import numpy as np
import pytest

import peekref
from autobub3hs_amd import _lib, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
CTYPES = {"uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32}


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    decl = re.search(r"int abub_peek_planes_dev\((.*?)\);", hdr, re.S)
    assert decl, "abub_peek_planes_dev is not declared in include/abub_hip.h"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["diff", "diff_bytes", "frames", "frames_bytes", "items", "nitems", "rects",
                                                         "nrects", "W", "H", "out", "out_bytes", "status", "stream"]
    res, args = _lib.SIGNATURES["abub_peek_planes_dev"]
    assert res is ctypes.c_int and len(args) == len(params)
    for p, a in zip(params, args):  # pointers as void *, sizes as size_t, counts as int
        assert a is (ctypes.c_void_p if "*" in p else ctypes.c_size_t if p.startswith("size_t") else ctypes.c_int), p
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_peek_planes_dev")
    assert callable(hip.peek_planes)
    # the item record: the header's fields in the header's order, 48 bytes
    body = hdr.split("typedef struct abub_peek_item {")[1].split("} abub_peek_item;")[0]
    fields = re.findall(r"^\s*(uint64_t|int32_t)\s+(\w+);", body, re.M)
    assert [(n, CTYPES[t]) for t, n in fields] == list(_lib.PeekItem._fields_)
    assert ctypes.sizeof(_lib.PeekItem) == 48 and _lib.PeekItem.thr.offset == 32
    assert "typedef struct abub_peek_rect { int32_t x, y, w, h; } abub_peek_rect;" in hdr
    codes = dict(re.findall(r"#define ABUB_PEEK_E_(\w+) (\d+)", hdr))
    assert codes == {"SRC": str(peekref.E_SRC), "DST": str(peekref.E_DST), "RECT": str(peekref.E_RECT)}
    # hip.peek_items writes the same record
    raw = hip.peek_items([(1, 2, 48, 96, -7, 5, 6)])
    it = _lib.PeekItem.from_buffer_copy(raw.tobytes())
    assert (it.diff, it.frame, it.thr_out, it.pres_out, it.thr, it.rect_begin, it.rect_count, it.reserved) == (1, 2, 48, 96, -7, 5, 6, 0)


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(diff=p, diff_bytes=1024, frames=p + 1024, frames_bytes=1024, items=p + 2048, nitems=1, rects=p + 3072, nrects=1, W=8, H=8,
              out=p + 4096, out_bytes=1024, status=p + 6144, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_peek_planes_dev(*[a[k] for k in ok])

    bad = [dict(diff=None), dict(frames=None), dict(items=None), dict(out=None), dict(status=None), dict(rects=None), dict(nitems=-1),
           dict(nrects=-1), dict(nitems=-3, diff=None), dict(W=0), dict(H=0), dict(W=-4), dict(W=65536), dict(H=65536), dict(H=-1),
           dict(items=p + 2048 + 4), dict(rects=p + 3072 + 2), dict(status=p + 6144 + 1), dict(out=p + 4096 + 8),
           dict(nitems=0, W=0), dict(nitems=0, out=None)]  # (no items excuse nothing)
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_peek_planes_dev" in L.abub_last_error(), kw
    assert not any(buf)


def test_no_items_is_ok_and_touches_nothing():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 512)(*([0x5A] * 512))
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.abub_peek_planes_dev(p, 64, p, 64, p, 0, p, 3, 1280, 1024, p, 64, p, None) == 0
    assert L.abub_peek_planes_dev(p, 64, p, 64, p, 0, None, 0, 65535, 65535, p, 64, p, None) == 0  # (no list of rectangles at all)
    assert bytes(buf) == bytes([0x5A]) * 512


def test_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        return
    src = torch.zeros(64, dtype=torch.uint8)
    out = torch.full((64,), 0x5A, dtype=torch.uint8)
    with pytest.raises(_lib.AbubError, match="no CPU fallback"):
        hip.peek_planes(src, src, [(0, 0, 0, 16, 3, 0, 0)], [], 4, 4, out)
    assert bool((out == 0x5A).all())
    # and the entry itself, told to launch without a device, reports the failure: nothing is computed on the host
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 1024)(*([0x5A] * 1024))
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.abub_peek_planes_dev(p, 64, p, 64, p + 128, 1, None, 0, 4, 4, p + 256, 64, p + 512, None) < 0
    assert bytes(buf) == bytes([0x5A]) * 1024


def test_restatement_draws_what_cv_rectangle_draws():
    """peekref against pictures written out by hand: the rows y and y + h - 1 and the columns x and x + w - 1, clipped."""
    def pic(*rows):
        return np.array([[255 if ch == "#" else 0 for ch in r] for r in rows], np.uint8)

    z = np.zeros((4, 6), np.uint8)
    assert np.array_equal(peekref.presentation(z, [(1, 0, 4, 3)]), pic(".####.", ".#..#.", ".####.", "......"))
    assert np.array_equal(peekref.presentation(z, [(-1, 1, 3, 9)]), pic("......", "##....", ".#....", ".#...."))
    assert np.array_equal(peekref.presentation(z, [(4, -1, 5, 3)]), pic("....#.", "....##", "......", "......"))
    assert np.array_equal(peekref.presentation(z, [(-1, -1, 8, 6)]), z)  # around the frame: no pixel of the outline inside
    assert np.array_equal(peekref.presentation(z, [(2, 3, 1, 1), (0, 0, 0, 4), (0, 0, 4, -1), (6, 0, 2, 2), (0, 4, 2, 2)]),
                          pic("......", "......", "......", "..#..."))
    assert np.array_equal(peekref.presentation(z, [(0, 0, 2, 2), (1, 1, 2, 2)]), pic("##....", "###...", ".##...", "......"))
    assert np.array_equal(peekref.thresholded(np.array([0, 1, 2, 254, 255]), 1), [0, 0, 255, 255, 255])
    assert np.array_equal(peekref.thresholded(np.array([0, 255]), 255), [0, 0]) and np.array_equal(peekref.thresholded(np.array([0, 255]), -1), [255, 255])
    # a refused item keeps its planes; a good one next to it gets both
    out = np.full(160, 0x5A, np.uint8)
    src = np.arange(64, dtype=np.uint8)
    got, st = peekref.planes(src, src, [(0, 0, 0, 16, 7, 0, 0), (60, 0, 32, 48, 7, 0, 0), (0, 0, 96, 120, 7, 0, 0)], [], 4, 4, out)
    assert list(st) == [0, peekref.E_SRC, peekref.E_DST]
    assert np.array_equal(got[0:16], np.where(np.arange(16) > 7, 255, 0)) and np.array_equal(got[16:32], src[:16]) and (got[32:] == 0x5A).all()


def test_cli_refuses_peek_with_the_modes_it_does_not_belong_to(tmp_path):
    """--peek is the batched path's: every combination below is refused before anything is read or written."""
    import subprocess

    from autobub3hs_amd import host

    host.build()
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    base = ["-d", str(tmp_path), "-r", "20200101_0", "-o", str(tmp_path / "out"), "--peek", str(tmp_path / "peek")]
    for extra, word in ((["-e", "1"], "-e/--event"), (["--debug", "100"], "--debug"), (["--per-event"], "--per-event"),
                        (["--merge", "2"], "--merge"), (["--repack", str(tmp_path / "r")], "--repack"),
                        (["--unpack", str(tmp_path / "u")], "--unpack"), (["--verify-repack", str(tmp_path / "v")], "--verify-repack")):
        p = subprocess.run([exe] + base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 255 and f"--peek cannot be combined with {word}" in p.stderr, (extra, p.stderr)
    p = subprocess.run([exe, "-d", str(tmp_path), "-r", "20200101_0", "-o", str(tmp_path / "out"), "--peek="], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 255 and "--peek needs the directory" in p.stderr
    assert "--peek" in subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert not os.path.exists(tmp_path / "out") and not os.path.exists(tmp_path / "peek")
    hdr = open(os.path.join(ROOT, "autobub3hs_amd", "host", "runbatch.hpp")).read()
    assert "std::string peekDir;" in hdr and "peekStacks" in hdr and "peekFiles" in hdr and "peekBytes" in hdr


@pytest.mark.parametrize("W,H", [(4, 1), (5, 3), (60, 2), (68, 5), (160, 33)])
def test_host_route_planes_are_the_restatement(W, H):
    """peekPlanesHost (host/peek.cpp), the definition the GPU route is held to, against tests/peekref.py."""
    from autobub3hs_amd import host

    host.build()
    rs = np.random.RandomState(W * 100 + H)
    big = 2 ** 31 - 1
    rects = [(W // 2, H // 2, 1, 1), (0, 0, W, H), (-3, H // 3, 6, 3), (W - 2, 0, 5, 2), (1, -2, 3, 4), (0, H - 1, 3, 5),
             (-1, -1, W + 2, H + 2), (W, 0, 3, 3), (-5, -5, 3, 3), (1, 0, 0, 3), (0, 0, 2, -1), (0, 0, 3, 3), (1, 0, 3, 2),
             (big - 10, 0, 5, 5), (-big - 1, 0, big, 2)]
    for cut in (0, 1, 100, 254, 255, -1):
        D = rs.randint(0, 256, (H, W)).astype(np.uint8)
        D.reshape(-1)[::2] = np.clip(cut, 0, 255)
        D.reshape(-1)[1::2] = np.clip(cut + 1, 0, 255)
        D.reshape(-1)[rs.rand(W * H) < 0.3] = rs.randint(0, 256)
        frame = rs.randint(0, 255, (H, W)).astype(np.uint8)
        for use in (rects, [], rects[:1]):
            thr, pres = host.peek_planes_host(D, frame, cut, use)
            assert np.array_equal(thr, peekref.thresholded(D, cut)), (cut, len(use))
            assert np.array_equal(pres, peekref.presentation(frame, use)), (cut, len(use))
