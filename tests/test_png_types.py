"""Every non-interlaced PNG type on the host: the decoder (host.imdecode) gives the 8-bit grey value tests/pngtypes.py defines
from the samples a file was written from, Pillow agrees on the types it reads, and the typed walk (host.png_walk_typed, what
ABUB_GPU_PNG_TYPES=1 sends to the GPU decoder) accepts exactly the files the host decoder reads, names their kind and refuses
the rest, while host.png_walk keeps refusing everything but the two 8-bit types.  No GPU."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import pngtypes as pt
from autobub3hs_amd import hip, host

ALL_KINDS = pt.TYPED_KINDS + pt.EIGHT_BIT_KINDS
H = 10


def files_of(ctype, depth):
    """every width class, each filter type on the first row: -> [(W, first, file, expected, palette, samples)]"""
    rs = np.random.RandomState(100 * ctype + depth)
    out = []
    for W in (4, 12, 68, 260):
        for first in range(5):
            pal = pt.random_palette(rs, max(1, (1 << depth) - 3)) if ctype == 3 else None
            s = pt.random_samples(rs, ctype, depth, W, H)
            out.append((W, first, pt.make_png(s, ctype, depth, pt.filter_sequence(first), pal), pt.expected(s, ctype, depth, pal), pal, s))
    return out


@pytest.mark.parametrize("ctype,depth", ALL_KINDS)
def test_host_decoder_follows_the_rule(ctype, depth):
    for W, first, data, want, _, _ in files_of(ctype, depth):
        got = host.imdecode(data)
        assert got is not None and got.shape == (H, W), (W, first)
        assert np.array_equal(got, want), (W, first, np.argwhere(got != want)[:4].tolist())


def test_the_rule_on_hand_made_values():
    """a few pixels worked out by hand, so that the rule itself is pinned by more than its own code"""
    s = np.array([[[0], [1], [2], [3]]], np.uint16)
    assert pt.expected(s, 0, 2).tolist() == [[0, 85, 170, 255]]
    assert pt.expected(np.array([[[0], [1]]], np.uint16), 0, 1).tolist() == [[0, 255]]
    assert pt.expected(np.array([[[0], [7], [15]]], np.uint16), 0, 4).tolist() == [[0, 119, 255]]
    assert pt.expected(np.array([[[0x12FF], [0xFF00]]], np.uint16), 0, 16).tolist() == [[0x12, 0xFF]]
    assert pt.expected(np.array([[[0x80, 0x11], [0x7F, 0xEE]]], np.uint16), 4, 8).tolist() == [[0x80, 0x7F]]
    # (255 * 9797 + 16384) >> 15 = 76; (255 * 19234 + 16384) >> 15 = 150; (255 * 3737 + 16384) >> 15 = 29; white stays white
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]]], np.uint16)
    assert pt.expected(rgb, 2, 8).tolist() == [[76, 150, 29, 255]]
    assert pt.expected(rgb << 8 | 0x5A, 2, 16).tolist() == [[76, 150, 29, 255]]
    rgba = np.concatenate([rgb, np.full((1, 4, 1), 7, np.uint16)], axis=2)
    assert pt.expected(rgba, 6, 8).tolist() == [[76, 150, 29, 255]]
    pal = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    assert pt.expected(np.array([[[0], [1], [2], [3]]], np.uint16), 3, 2, pal).tolist() == [[76, 29, 0, 0]]  # (past the palette: 0)
    assert len(pt.rgb_extremes()) >= 100
    packed = pt.pack_rows(np.array([[[1], [0], [1], [1], [0]]], np.uint16), 1)
    assert packed.tolist() == [[0b10110111]]  # MSB first, the three padding bits set


@pytest.mark.parametrize("ctype,depth", [(0, 1), (3, 1), (3, 2), (3, 4), (4, 8), (2, 8), (6, 8), (0, 16)])
def test_pillow_reads_the_same_samples(ctype, depth):
    """the writer against an independent reader, on the types Pillow reads (L;1, P;1/2/4, LA, RGB, RGBA, I;16)"""
    for W, first, data, _, pal, s in files_of(ctype, depth):
        im = Image.open(io.BytesIO(data))
        im.load()
        a = np.asarray(im)
        if ctype == 0 and depth == 1:
            assert np.array_equal(a.astype(np.uint8), s[:, :, 0].astype(np.uint8)), (W, first)
        elif ctype == 3:
            assert im.mode == "P" and np.array_equal(a, s[:, :, 0]), (W, first)
            assert bytes(im.getpalette()[:3 * len(pal)]) == pal.tobytes()
        elif depth == 16:
            assert np.array_equal(a.astype(np.uint16), s[:, :, 0]), (W, first, im.mode)
        else:
            assert a.shape == s.shape and np.array_equal(a, s), (W, first, im.mode)


@pytest.mark.parametrize("ctype,depth", ALL_KINDS)
def test_typed_walk_accepts_every_kind_and_names_it(ctype, depth):
    for W, first, data, _, pal, _ in files_of(ctype, depth)[::5]:
        w = host.png_walk_typed(data, W, H)
        assert w is not None, (W, first)
        segs, lut, kind = w
        assert kind == pt.kind_code(ctype, depth) == hip.png_kind(ctype, depth)
        assert (kind == 0) == ((ctype, depth) in pt.EIGHT_BIT_KINDS)
        assert len(segs) == 1 and data[segs[0][0] - 4:segs[0][0]] == b"IDAT" and struct.unpack(">I", data[segs[0][0] - 8:segs[0][0] - 4])[0] == segs[0][1]
        if ctype == 3:
            table = np.zeros(256, np.uint8)
            table[:len(pal)] = pt.rgb2grey(pal[:, 0].astype(int), pal[:, 1].astype(int), pal[:, 2].astype(int))
            assert lut == table.tobytes()
        else:
            assert lut is None
        assert hip.png_parse(data, W, H, types=True) == (segs, lut, kind)  # the Python restatement
        old = host.png_walk(data, W, H)
        if kind == 0:
            assert old == (segs, lut) == hip.png_parse(data, W, H)
        else:
            assert old is None and hip.png_parse(data, W, H) is None


def test_typed_walk_refusals():
    rs = np.random.RandomState(9)
    W = 12
    rgb = pt.random_samples(rs, 2, 8, W, H)
    fts = pt.filter_sequence(2)
    good = pt.make_png(rgb, 2, 8, fts, idat=3, extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", bytes(6))])
    w = host.png_walk_typed(good, W, H)
    assert w is not None and len(w[0]) == 3 and w[2] == (2 | 8 << 8)  # (ancillary chunks are ignored, as on the host)
    assert np.array_equal(host.imdecode(good), pt.expected(rgb, 2, 8))
    stream = pt.filter_rows(pt.pack_rows(rgb, 8), 3, fts).tobytes()
    refused = {
        "interlace 1": pt.png_file(W, H, 2, 8, stream, interlace=1),
        "another size": pt.make_png(pt.random_samples(rs, 2, 8, W + 4, H), 2, 8, fts),
        "RGB at depth 4": pt.png_file(W, H, 2, 4, stream),
        "palette at depth 16": pt.png_file(W, H, 3, 16, stream, palette=pt.random_palette(rs, 4)),
        "grey+alpha at depth 2": pt.png_file(W, H, 4, 2, stream),
        "colour type 5": pt.png_file(W, H, 5, 8, stream),
        "depth 3": pt.png_file(W, H, 0, 3, stream),
        "cut inside a chunk": good[:len(good) - 20],
        "no IDAT": good[:33] + pt.chunk(b"IEND", b""),
        "not a PNG": b"BM" + good[2:],
    }
    for name, data in refused.items():
        assert host.png_walk_typed(data, W, H) is None, name
        assert hip.png_parse(data, W, H, types=True) is None, name
        assert host.png_walk(data, W, H) is None, name
    for name in ("interlace 1", "RGB at depth 4", "palette at depth 16", "grey+alpha at depth 2", "colour type 5", "depth 3", "cut inside a chunk"):
        assert host.imdecode(refused[name]) is None, name  # (the host decoder refuses them too)


def test_raw_stride_of_every_kind():
    """abub_png_raw_stride_kind: H x (row bytes + 1) rounded up to 16, plus 16; 0 outside the table; kind 0 as ever"""
    from autobub3hs_amd import _lib
    L = _lib.lib()
    for W, Hh in ((4, 5), (12, 11), (1280, 1024), (2048, 7)):
        assert L.abub_png_raw_stride_kind(W, Hh, 0) == L.abub_png_raw_stride(W, Hh) == ((Hh * (W + 1) + 15) & ~15) + 16
        for ctype, depth in pt.TYPED_KINDS:
            want = ((Hh * (pt.row_bytes(W, ctype, depth) + 1) + 15) & ~15) + 16
            assert L.abub_png_raw_stride_kind(W, Hh, pt.kind_code(ctype, depth)) == want, (W, Hh, ctype, depth)
        for kind in (2 | 4 << 8, 3 | 16 << 8, 4 | 2 << 8, 5 | 8 << 8, 0 | 3 << 8, 0 | 8 << 8, 1 << 16, 2 | 8 << 8 | 1 << 16):
            assert L.abub_png_raw_stride_kind(W, Hh, kind) == 0, hex(kind)
    assert L.abub_png_raw_stride_kind(0, 5, 0) == 0 and L.abub_png_raw_stride_kind(4, 0, 2 | 8 << 8) == 0
