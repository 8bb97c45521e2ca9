"""The typed route of the GPU PNG decoder (abub_png_decode_typed_dev through hip.png_decode(..., types=True)): the 13 kinds
the 8-bit route refuses -- grey at 1, 2, 4 and 16 bits, palette at 1, 2 and 4, grey+alpha, RGB and RGBA at 8 and 16 -- decoded
to exactly the pixels the samples of tests/pngtypes.py define.  Every comparison is exact.

One batch per width holds every kind five times, H = 10 rows, file k of a kind filtered with pngtypes.filter_sequence(k): each
of the five filter types on the first row (the row above is zeros), and over the five files each type after every other.  All
bits of all samples are random, so the low bytes of 16-bit samples and the alpha are unlike the bytes a pixel comes from; RGB
frames also hold the triples at which the grey conversion's rounding steps (pngtypes.rgb_extremes).  Two 8-bit frames, grey
and palette, ride in every batch and go through the kernels of the 8-bit route.

Widths.  k_png_unfilter_typed gives lane l the units [l * chunk, (l + 1) * chunk) of a row, chunk = ceil(units / 64); a unit is
one pixel (its filter distance in bytes) or, below 8 bits per pixel, one byte.  A seam between two lanes is where Sub's carry,
and Average's and Paeth's left and upper-left pixel, cross from one lane to the next:
  4     one unit per lane, four lanes; below 8 bits one lane only, and a 1-bit row is one byte with four padding bits
  12    twelve lanes of one unit; a 1-bit row is two bytes, the second half padding
  64    every lane owns exactly one unit: the wave scan at its full width with nothing inside a lane
  68    chunk 2, 34 full lanes: a seam behind every second pixel (4-bit rows: 34 one-byte lanes)
  140   chunk 3, 47 lanes, the last one partly filled (2 of 3 units)
  264   chunk 5, 53 lanes, the last one partly filled (4 of 5); 2-bit rows 66 bytes: chunk 2
  2048  chunk 32, 64 full lanes, the widest row (16,384 bytes for RGBA 16) and the largest LDS allocation
The refusals sit in a batch of their own between good frames: a refused frame must leave its neighbours and the bytes behind
`out` as they are.  The widest batch and the refusals run once more through the one-wave inflate (ABUB_PNG_WAVES=1, read once
per process) in a fresh child."""
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

import pngtypes as pt  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (4, 12, 64, 68, 140, 264, 2048)
H = 10
CANARY = 4096


def status_codes():
    text = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ABUB_PNG_E_(\w+) (\d+)", text)}


def one_file(rs, ctype, depth, W, Hh, fts):
    """-> (file, expected pixels)"""
    pal = pt.random_palette(rs, (1 << min(depth, 8)) - 3 if depth > 1 else 2) if ctype == 3 else None  # (short: indices reach past it)
    s = pt.random_samples(rs, ctype, depth, W, Hh)
    return pt.make_png(s, ctype, depth, fts, pal), pt.expected(s, ctype, depth, pal)


def batch_of(W):
    """-> (names, files, expected [n, H, W])"""
    rs = np.random.RandomState(1000 + W)
    names, files, want = [], [], []
    for ctype, depth in pt.EIGHT_BIT_KINDS[:1] + pt.TYPED_KINDS + pt.EIGHT_BIT_KINDS[1:]:
        for first in range(5 if (ctype, depth) in pt.TYPED_KINDS else 1):
            f, e = one_file(rs, ctype, depth, W, H, pt.filter_sequence(first))
            names.append(f"{pt.kind_name(ctype, depth)} W={W} first filter {first}")
            files.append(f)
            want.append(e)
    return names, files, np.stack(want)


def decode_batch(W):
    import torch
    from autobub3hs_amd import hip
    names, files, want = batch_of(W)
    out, st = hip.png_decode(files, W, H, types=True)
    torch.cuda.synchronize()
    return names, want, out.cpu().numpy(), st


def refusal_batch():
    """good frames at the even places, one refusal between each two: -> (names, files, expected, kinds, dsts, codes)"""
    W, Hh = 68, 7
    rs = np.random.RandomState(77)
    fts = [4, 1, 3, 2, 0, 4, 3]
    goods = [one_file(rs, c, d, W, Hh, fts) for c, d in ((2, 8), (0, 16), (6, 16), (3, 2), (0, 8), (4, 8))]
    rgb = pt.random_samples(rs, 2, 8, W, Hh)
    g16 = pt.random_samples(rs, 0, 16, W, Hh)
    refused = [
        # (name, file, kind in the descriptor or None = the file's, dst or None = its place, status)
        ("filter type 5 in a middle row", pt.make_png(rgb, 2, 8, [4, 1, 3, 5, 0, 4, 3]), None, None, "FILTER"),
        ("an RGB stream under a grey-16 kind", pt.make_png(rgb, 2, 8, fts), pt.kind_code(0, 16), None, "TOOMUCH"),
        ("a grey-16 stream under an RGB kind", pt.make_png(g16, 0, 16, fts), pt.kind_code(2, 8), None, "TOOLITTLE"),
        ("kind 2 | 4 << 8", pt.make_png(rgb, 2, 8, fts), 2 | 4 << 8, None, "DESC"),
        ("a frame that would end behind out", pt.make_png(rgb, 2, 8, fts), None, "last", "DESC"),
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
    n, P = len(files), W * Hh
    dsts = [(n * P - P + 4 if d == "last" else d) for d in dsts]  # (four bytes of it would lie behind out's n * P)
    return W, Hh, names, files, want, kinds, dsts, codes


def decode_refusals():
    import torch
    from autobub3hs_amd import hip
    W, Hh, names, files, want, kinds, dsts, codes = refusal_batch()
    n, P = len(files), W * Hh
    out = torch.zeros(n * P + CANARY, dtype=torch.uint8, device="cuda:0")
    out[n * P:] = 0xA5
    _, st = hip.png_decode(files, W, Hh, types=True, kinds=kinds, dsts=dsts, out=out, out_bytes=n * P)
    torch.cuda.synchronize()
    return names, want, codes, out.cpu().numpy(), st, (n, P)


@pytest.fixture(scope="module")
def refusals():
    return decode_refusals()


@pytest.mark.parametrize("W", WIDTHS)
def test_every_kind_decodes_to_the_pixels_of_its_samples(W):
    names, want, px, st = decode_batch(W)
    assert len(names) == 5 * len(pt.TYPED_KINDS) + 2
    for k, name in enumerate(names):
        assert st[k] == 0, (name, int(st[k]))
        assert np.array_equal(px[k], want[k]), (name, np.argwhere(px[k] != want[k])[:4].tolist())


def test_refused_frames_carry_the_documented_status(refusals):
    names, _, codes, _, st, _ = refusals
    table = status_codes()
    assert sum(c is not None for c in codes) == 5
    for k, code in enumerate(codes):
        if code is not None:
            assert st[k] == table[code], (names[k], int(st[k]), code)


def test_neighbours_of_refused_frames_and_the_bytes_behind_out_stay_intact(refusals):
    names, want, codes, out, st, (n, P) = refusals
    for k, code in enumerate(codes):
        if code is None:
            assert st[k] == 0, (names[k], int(st[k]))
            assert np.array_equal(out[k * P:(k + 1) * P].reshape(want[k].shape), want[k]), names[k]
    assert (out[n * P:] == 0xA5).all()
    k = names.index("kind 2 | 4 << 8")
    assert not out[k * P:(k + 1) * P].any()  # (refused before anything was written)


def summary(W):
    """what the two inflate routes must agree on: statuses and a digest of the pixels of the batch of width W and of the
    refusals"""
    _, _, px, st = decode_batch(W)
    _, _, _, out, rst, _ = decode_refusals()
    return {"status": [int(v) for v in st], "pixels": hashlib.sha256(px.tobytes()).hexdigest(),
            "refusal_status": [int(v) for v in rst], "refusal_pixels": hashlib.sha256(out.tobytes()).hexdigest()}


def test_one_wave_route_gives_the_same_statuses_and_pixels():
    """ABUB_PNG_WAVES=1 (k_png_inflate<false>) is read once per process: a fresh child decodes the widest batch and the
    refusals and reports statuses and digests."""
    env = dict(os.environ, ABUB_PNG_WAVES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == summary(WIDTHS[-1])


if __name__ == "__main__":
    print(json.dumps(summary(WIDTHS[-1])))
