"""The Adam7 route of the GPU PNG decoder (abub_png_decode_adam7_dev through hip.png_decode(..., types=True, adam7=True)):
interlaced files of all 15 kinds decoded to exactly the pixels the samples of tests/pngtypes.py define (tests/pngadam7.py
writes the files).  Every comparison is exact.

One batch per size holds every kind five times as an interlaced file, file k of a kind filtered with
pngadam7.pass_filters(k): each of the five filter types on the first row of every pass that has pixels (the row above is
zeros, whatever the last row of the pass before was: the samples are random), and over the five files each type after every
other.  Non-interlaced frames ride in every batch -- 8-bit grey and palette (k_png_unfilter's), RGB 8, grey 16 and palette 2
(k_png_unfilter_typed's) -- and every frame goes to a place of its own in `out`, in scrambled order, with canary bytes
between the frames and behind the last one: k_png_unfilter_adam7 stores single bytes at a stride of up to 8, and a store that
misses its pixel lands in a canary or in another frame.

Sizes (W, H).  k_png_unfilter_adam7 runs one wave per (frame, pass); lane l of a wave owns the units [l * chunk, (l + 1) *
chunk) of a pass row, chunk = ceil(units / 64), and converts the pass pixels l, l + 64, ...:
  (4, 1)      passes 1, 4, 6 only, one or two pixels per pass row; sub-byte rows are one byte that is mostly padding
  (4, 2)      pass 7 appears (a whole image row, stored as dwords); passes 2, 3, 5 absent
  (8, 3)      pass 2 appears with one pixel, pass 5 with one row; pass 3 absent
  (12, 5)     all seven passes, pass 3 with one row of three pixels
  (64, 8)     one full tile row: pass 7 is 64 units of one pixel, passes 1 and 2 eight pixels in one row
  (68, 9)     pass 7 rows of 68 pixels: chunk 2, 34 lanes; passes 1 .. 6 partly filled waves; H = 9 gives pass 1 a second row
  (264, 10)   chunk up to 5 with a partly filled last lane; more than 64 pass pixels per row in passes 5 .. 7 (two rounds of
              the conversion loop, the second partly filled)
  (2048, 10)  64 full lanes in every pass, chunk 32 in pass 7, the widest row and the largest LDS allocation
The refusals sit between good frames in a batch of their own and in a launch with a raw stride that only the non-interlaced
frames fit.  The widest batch and the refusals run once more through the one-wave inflate (ABUB_PNG_WAVES=1, read once per
process) in a fresh child."""
import functools
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pngadam7 as a7  # noqa: E402
import pngtypes as pt  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = ((4, 1), (4, 2), (8, 3), (12, 5), (64, 8), (68, 9), (264, 10), (2048, 10))
PLAIN = ((0, 8), (3, 8), (2, 8), (0, 16), (3, 2))  # the non-interlaced frames of every batch
GAP = 64  # canary bytes in front of every frame
CANARY = 4096  # and behind the last one
FILL = 0xA5


def status_codes():
    text = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ABUB_PNG_E_(\w+) (\d+)", text)}


def one_file(rs, ctype, depth, W, H, fts, interlaced=True):
    """-> (file, expected pixels)"""
    pal = pt.random_palette(rs, (1 << min(depth, 8)) - 3 if depth > 1 else 2) if ctype == 3 else None  # (short: indices reach past it)
    s = pt.random_samples(rs, ctype, depth, W, H)
    data = a7.make_adam7(s, ctype, depth, fts, pal) if interlaced else pt.make_png(s, ctype, depth, fts, pal)
    return data, pt.expected(s, ctype, depth, pal)


@functools.lru_cache(None)
def batch_of(W, H):
    """-> (names, files, expected [n, H, W])"""
    rs = np.random.RandomState(2000 + 16 * W + H)
    names, files, want = [], [], []
    for ctype, depth in a7.ALL_KINDS:
        for first in range(5):
            f, e = one_file(rs, ctype, depth, W, H, a7.pass_filters(first))
            names.append(f"adam7 {pt.kind_name(ctype, depth)} {W}x{H} first filter {first}")
            files.append(f)
            want.append(e)
    for k, (ctype, depth) in enumerate(PLAIN):  # spread among the interlaced ones
        f, e = one_file(rs, ctype, depth, W, H, (pt.filter_sequence(k) * 2)[:H], interlaced=False)
        at = (k + 1) * len(files) // (len(PLAIN) + 1)
        names.insert(at, f"plain {pt.kind_name(ctype, depth)} {W}x{H}")
        files.insert(at, f)
        want.insert(at, e)
    return names, files, np.stack(want)


def scattered(n, P, seed):
    """byte offsets of n frames of P bytes in scrambled order, GAP canary bytes in front of each: -> (dsts, bytes used)"""
    order = np.random.RandomState(seed).permutation(n)
    return [int(order[i]) * (P + GAP) + GAP for i in range(n)], n * (P + GAP)


def outside(out, dsts, P):
    """the bytes of `out` that belong to no frame"""
    mask = np.ones(len(out), bool)
    for d in dsts:
        mask[d:d + P] = False
    return out[mask]


@functools.lru_cache(None)
def decode_batch(W, H):
    import torch
    from autobub3hs_amd import hip
    names, files, want = batch_of(W, H)
    n, P = len(files), W * H
    dsts, used = scattered(n, P, W + H)
    out = torch.full((used + CANARY,), FILL, dtype=torch.uint8, device="cuda:0")
    _, st = hip.png_decode(files, W, H, types=True, adam7=True, dsts=dsts, out=out, out_bytes=used)
    torch.cuda.synchronize()
    return names, want, out.cpu().numpy(), st, dsts


def refusal_batch():
    """good frames at the even places, one refusal between each two: -> (W, H, names, files, expected, kinds, dsts, codes)"""
    W, H = 68, 10
    rs = np.random.RandomState(78)
    fts = a7.pass_filters(4)
    goods = [one_file(rs, c, d, W, H, fts, il) if il else one_file(rs, c, d, W, H, [4, 1, 3, 2, 0, 4, 3, 1, 2, 0], il)
             for c, d, il in ((2, 8, True), (0, 16, False), (6, 16, True), (3, 2, True), (0, 8, False), (0, 8, True), (4, 8, True))]
    rgb = pt.random_samples(rs, 2, 8, W, H)
    flag = a7.ADAM7_FLAG
    assert a7.a7_size(W, H, 2, 8) > H * (pt.row_bytes(W, 2, 8) + 1)
    refused = [
        # (name, file, kind in the descriptor or None = the file's, dst or None = its place, status)
        ("filter type 5 in pass 6", a7.make_adam7(rgb, 2, 8, lambda p, r: 5 if (p, r) == (5, 2) else fts(p, r)), None, None, "FILTER"),
        ("a non-interlaced stream under a flagged kind", pt.make_png(rgb, 2, 8, [0] * H), pt.kind_code(2, 8) | flag, None, "TOOLITTLE"),
        ("an interlaced stream under an unflagged kind", a7.make_adam7(rgb, 2, 8, fts), pt.kind_code(2, 8), None, "TOOMUCH"),
        ("kind 2 | 4 << 8 | 1 << 16", a7.make_adam7(rgb, 2, 8, fts), 2 | 4 << 8 | flag, None, "DESC"),
        ("a frame that would end behind out", a7.make_adam7(rgb, 2, 8, fts), None, "last", "DESC"),
    ]
    names, files, want, kinds, dsts, codes = [], [], [], [], [], []
    for k, (f, e) in enumerate(goods):
        names.append(f"good {k}")
        files.append(f)
        want.append(e)
        kinds.append(None)
        dsts.append(None)
        codes.append(None)
        if k < len(refused):
            name, file, kind, dst, code = refused[k]
            names.append(name)
            files.append(file)
            want.append(None)
            kinds.append(kind)
            dsts.append(dst)
            codes.append(code)
    n, P = len(files), W * H
    dsts = [(n * P - P + 4 if d == "last" else d) for d in dsts]  # (four bytes of it would lie behind out's n * P)
    return W, H, names, files, want, kinds, dsts, codes


@functools.lru_cache(None)
def decode_refusals():
    import torch
    from autobub3hs_amd import hip
    W, H, names, files, want, kinds, dsts, codes = refusal_batch()
    n, P = len(files), W * H
    out = torch.zeros(n * P + CANARY, dtype=torch.uint8, device="cuda:0")
    out[n * P:] = FILL
    _, st = hip.png_decode(files, W, H, types=True, adam7=True, kinds=kinds, dsts=dsts, out=out, out_bytes=n * P)
    torch.cuda.synchronize()
    return names, want, codes, out.cpu().numpy(), st, (n, P)


@pytest.mark.parametrize("W,H", SIZES)
def test_every_kind_decodes_to_the_pixels_of_its_samples(W, H):
    names, want, out, st, dsts = decode_batch(W, H)
    assert len(names) == 5 * 15 + len(PLAIN)
    for k, name in enumerate(names):
        assert st[k] == 0, (name, int(st[k]))
        got = out[dsts[k]:dsts[k] + W * H].reshape(H, W)
        assert np.array_equal(got, want[k]), (name, np.argwhere(got != want[k])[:4].tolist())
    assert (outside(out, dsts, W * H) == FILL).all()


def test_refused_frames_carry_the_documented_status():
    names, _, codes, _, st, _ = decode_refusals()
    table = status_codes()
    assert sum(c is not None for c in codes) == 5
    for k, code in enumerate(codes):
        if code is not None:
            assert st[k] == table[code], (names[k], int(st[k]), code)


def test_neighbours_of_refused_frames_and_the_bytes_behind_out_stay_intact():
    names, want, codes, out, st, (n, P) = decode_refusals()
    for k, code in enumerate(codes):
        if code is None:
            assert st[k] == 0, (names[k], int(st[k]))
            assert np.array_equal(out[k * P:(k + 1) * P].reshape(want[k].shape), want[k]), names[k]
    assert (out[n * P:] == FILL).all()
    for name in ("kind 2 | 4 << 8 | 1 << 16", "a non-interlaced stream under a flagged kind"):
        k = names.index(name)
        assert not out[k * P:(k + 1) * P].any(), name  # (refused before anything was written)


def stride_launch(typed_entry):
    """three 1-bit grey frames, the middle one interlaced, in a launch whose raw stride is abub_png_raw_stride_kind's: the
    non-interlaced frames fit it, the passes of the interlaced one do not.  typed_entry: through abub_png_decode_typed_dev,
    where the flagged kind is outside the table."""
    import torch
    from autobub3hs_amd import _lib, hip
    W, H = 68, 10
    L = _lib.lib()
    small, large = int(L.abub_png_raw_stride_kind(W, H, pt.kind_code(0, 1))), int(L.abub_png_raw_stride_adam7(W, H, pt.kind_code(0, 1) | a7.ADAM7_FLAG))
    assert 0 < small < large
    rs = np.random.RandomState(5)
    fts = [2, 4, 1, 3, 0, 4, 2, 1, 3, 0]
    s = pt.random_samples(rs, 0, 1, W, H)
    files = [one_file(rs, 0, 1, W, H, fts, False), (pt.make_png(s, 0, 1, fts) if typed_entry else a7.make_adam7(s, 0, 1, a7.pass_filters(1)), None),
             one_file(rs, 0, 1, W, H, fts, False)]
    P = W * H
    out = torch.full((3 * P + CANARY,), FILL, dtype=torch.uint8, device="cuda:0")
    if typed_entry:
        _, st = hip.png_decode([f for f, _ in files], W, H, types=True, kinds=[None, pt.kind_code(0, 1) | a7.ADAM7_FLAG, None], out=out, out_bytes=3 * P)
    else:
        _, st = hip.png_decode([f for f, _ in files], W, H, types=True, adam7=True, raw_stride=small, out=out, out_bytes=3 * P)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert [int(v) for v in st] == [0, status_codes()["DESC"], 0]
    for k in (0, 2):
        assert np.array_equal(out[k * P:(k + 1) * P].reshape(H, W), files[k][1])
    assert (out[P:2 * P] == FILL).all() and (out[3 * P:] == FILL).all()  # (refused before anything was written)


def test_a_raw_stride_too_small_for_the_passes_is_refused():
    stride_launch(False)


def test_typed_entry_still_refuses_a_flagged_kind():
    stride_launch(True)


def summary():
    """what the two inflate routes must agree on: statuses and a digest of the bytes of the widest batch and of the refusals
    (without the refused frames' own bytes: which passes of a frame with a bad filter type were stored before one of them
    reported it is not defined)"""
    _, _, out, st, _ = decode_batch(*SIZES[-1])
    _, _, codes, rout, rst, (n, P) = decode_refusals()
    kept = b"".join(rout[k * P:(k + 1) * P].tobytes() for k in range(n) if codes[k] is None) + rout[n * P:].tobytes()
    return {"status": [int(v) for v in st], "pixels": hashlib.sha256(out.tobytes()).hexdigest(),
            "refusal_status": [int(v) for v in rst], "refusal_pixels": hashlib.sha256(kept).hexdigest()}


def test_one_wave_route_gives_the_same_statuses_and_pixels():
    """ABUB_PNG_WAVES=1 (k_png_inflate<false>) is read once per process: a fresh child decodes the widest batch and the
    refusals and reports statuses and digests."""
    env = dict(os.environ, ABUB_PNG_WAVES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == summary()


if __name__ == "__main__":
    print(json.dumps(summary()))
