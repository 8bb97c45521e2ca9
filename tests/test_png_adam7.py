"""Adam7-interlaced PNG files on the host: the decoder (host.imdecode) gives, for all 15 kinds, the 8-bit grey value
tests/pngtypes.py defines from the samples a file was written from (tests/pngadam7.py writes the files), Pillow reads the same
samples from the kinds it knows, a stream that is not exactly the passes' bytes, a filter type above 4 in a pass and another
interlace method are refused; the walk with adam7 (host.png_walk_adam7, what ABUB_GPU_PNG_ADAM7=1 sends to the GPU decoder)
accepts the files and names their kind with bit 16 while the walks without it refuse them as ever;
abub_png_raw_stride_adam7 follows its formula; and a run of interlaced files repacks and verifies on the host.  No GPU.

Sizes: passes vanish one by one as an image shrinks -- (1,1) has pass 1 only, (2,1) passes 1 and 6, (3,2) 1, 4, 6, 7, (4,5)
all but 2, (5,7) and up all seven; (8,8) is one full Adam7 tile, (9,9) one pixel more, (12,10) the size whose byte
count DESIGN works out (380 for RGB 8), (68,10) the widest.  The filter type of row r of pass p is
pngadam7.pass_filters(first): over first = 0 .. 4 each of the five types stands on the first row of every pass that has
pixels, and each type follows every other.  The samples are random, so the last row of the pass before is never the zeros
a pass's first row has above it."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import pngadam7 as a7
import pngtypes as pt
from autobub3hs_amd import _lib, hip, host, synth

SIZES = ((1, 1), (2, 1), (3, 2), (4, 5), (5, 7), (8, 8), (9, 9), (12, 10), (68, 10))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")


def palette_of(rs, ctype, depth):
    return pt.random_palette(rs, max(2, (1 << depth) - 3)) if ctype == 3 else None  # (short: indices reach past it)


def files_of(ctype, depth):
    """-> [(W, H, first, file, expected, palette, samples)]"""
    rs = np.random.RandomState(7000 + 100 * ctype + depth)
    out = []
    for W, H in SIZES:
        for first in range(5):
            pal = palette_of(rs, ctype, depth)
            s = pt.random_samples(rs, ctype, depth, W, H)
            out.append((W, H, first, a7.make_adam7(s, ctype, depth, a7.pass_filters(first), pal), pt.expected(s, ctype, depth, pal), pal, s))
    return out


def test_geometry_and_filter_sequences():
    """the helper itself: a byte count worked out by hand, every pixel in exactly one pass, which passes the sizes drop, and
    what the filter sequences cover"""
    assert a7.a7_size(12, 10, 2, 8) == 380 and 10 * (pt.row_bytes(12, 2, 8) + 1) == 370
    assert [a7.present(W, H) for W, H in SIZES[:5]] == [[0], [0, 5], [0, 3, 5, 6], [0, 2, 3, 4, 5, 6], list(range(7))]
    for W, H in SIZES:
        seen = np.zeros((H, W), int)
        for p in a7.present(W, H):
            x0, y0, dx, dy = a7.PASSES[p]
            seen[y0::dy, x0::dx] += 1
        assert (seen == 1).all(), (W, H)
    pairs = set()
    for first in range(5):
        fts = a7.pass_filters(first)
        for p in a7.present(12, 10):
            rows = [fts(p, r) for r in range(a7.pass_dims(12, 10, p)[1])]
            assert rows[0] == first
            pairs |= set(zip(rows, rows[1:]))
    assert pairs == {(a, b) for a in range(5) for b in range(5)}


@pytest.mark.parametrize("ctype,depth", a7.ALL_KINDS)
def test_host_decoder_follows_the_rule(ctype, depth):
    for W, H, first, data, want, _, _ in files_of(ctype, depth):
        got = host.imdecode(data)
        assert got is not None and got.shape == (H, W), (W, H, first)
        assert np.array_equal(got, want), (W, H, first, np.argwhere(got != want)[:4].tolist())


# Pillow reads L;1/2/4/8, P;1/2/4/8, LA, RGB, RGBA and I;16; it has no mode for grey+alpha 16, RGB 16 and RGBA 16 (it strips
# them to 8 bits): those three are left out
@pytest.mark.parametrize("ctype,depth", [(0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (2, 8), (6, 8), (0, 16)])
def test_pillow_reads_the_same_samples(ctype, depth):
    for W, H, first, data, _, pal, s in files_of(ctype, depth):
        im = Image.open(io.BytesIO(data))
        im.load()
        a = np.asarray(im)
        if ctype == 0 and depth == 1:
            assert np.array_equal(a.astype(np.uint8), s[:, :, 0].astype(np.uint8)), (W, H, first)
        elif ctype == 0 and depth in (2, 4):  # (Pillow expands to 8 bits, as the rule does)
            assert np.array_equal(a, pt.expected(s, ctype, depth)), (W, H, first)
        elif ctype == 3:
            assert im.mode == "P" and np.array_equal(a, s[:, :, 0]), (W, H, first)
            assert bytes(im.getpalette()[:3 * len(pal)]) == pal.tobytes()
        elif ctype == 0:
            assert np.array_equal(a.astype(np.uint16), s[:, :, 0]), (W, H, first, im.mode)
        else:
            assert a.shape == s.shape and np.array_equal(a, s), (W, H, first, im.mode)


def test_refusals_beside_an_intact_neighbour():
    rs = np.random.RandomState(11)
    W, H = 12, 10
    for ctype, depth in ((2, 8), (0, 8), (0, 2), (6, 16)):
        s = pt.random_samples(rs, ctype, depth, W, H)
        fts = a7.pass_filters(3)
        stream = a7.adam7_stream(s, ctype, depth, fts)
        assert np.array_equal(host.imdecode(pt.png_file(W, H, ctype, depth, stream, interlace=1)), pt.expected(s, ctype, depth))
        bad5 = a7.adam7_stream(s, ctype, depth, lambda p, r: 5 if (p, r) == (2, 0) else fts(p, r))  # (pass 3's only row at H = 10)
        assert len(bad5) == len(stream) and bad5 != stream
        refused = {
            "one byte short": pt.png_file(W, H, ctype, depth, stream[:-1], interlace=1),
            "one byte long": pt.png_file(W, H, ctype, depth, stream + b"\0", interlace=1),
            "filter type 5 on a pass-3 row": pt.png_file(W, H, ctype, depth, bad5, interlace=1),
            "interlace 2": pt.png_file(W, H, ctype, depth, stream, interlace=2),
            "a non-interlaced stream": pt.png_file(W, H, ctype, depth, pt.filter_rows(pt.pack_rows(s, depth), pt.filter_distance(ctype, depth), [0] * H).tobytes(), interlace=1),
        }
        for name, data in refused.items():
            assert host.imdecode(data) is None, (ctype, depth, name)
        assert host.png_walk_adam7(refused["interlace 2"], W, H, typed=True) is None
        assert hip.png_parse(refused["interlace 2"], W, H, types=True, adam7=True) is None


@pytest.mark.parametrize("ctype,depth", a7.ALL_KINDS)
def test_adam7_walk_accepts_every_kind_and_names_it(ctype, depth):
    eight = (ctype, depth) in pt.EIGHT_BIT_KINDS
    for W, H, first, data, _, pal, s in files_of(ctype, depth)[2::5]:
        w = host.png_walk_adam7(data, W, H, typed=True)
        assert w is not None, (W, H, first)
        segs, lut, kind = w
        assert kind == pt.kind_code(ctype, depth) | a7.ADAM7_FLAG == hip.png_kind(ctype, depth) | hip.PNG_KIND_ADAM7
        assert len(segs) == 1 and data[segs[0][0] - 4:segs[0][0]] == b"IDAT" and struct.unpack(">I", data[segs[0][0] - 8:segs[0][0] - 4])[0] == segs[0][1]
        if ctype == 3:
            table = np.zeros(256, np.uint8)
            table[:len(pal)] = pt.rgb2grey(pal[:, 0].astype(int), pal[:, 1].astype(int), pal[:, 2].astype(int))
            assert lut == table.tobytes()
        else:
            assert lut is None
        assert hip.png_parse(data, W, H, types=True, adam7=True) == w  # the Python restatement
        # the 8-bit kinds without `typed`, the others only with it
        assert host.png_walk_adam7(data, W, H) == hip.png_parse(data, W, H, adam7=True) == (w if eight else None)
        # the walks without adam7 refuse a valid interlaced file as ever
        assert host.png_walk(data, W, H) is None and host.png_walk_typed(data, W, H) is None
        assert hip.png_parse(data, W, H) is None and hip.png_parse(data, W, H, types=True) is None
        # and with adam7 a non-interlaced file is what it was
        plain = pt.make_png(s, ctype, depth, [0] * H, pal)
        assert host.png_walk_adam7(plain, W, H, typed=True) == host.png_walk_typed(plain, W, H) == hip.png_parse(plain, W, H, types=True, adam7=True)
        assert host.png_walk_adam7(plain, W, H, typed=True)[2] == pt.kind_code(ctype, depth)


def test_raw_stride_adam7():
    """A7 rounded up to 16, plus 16, with bit 16; abub_png_raw_stride_kind's answer without it; 0 outside the table"""
    L = _lib.lib()
    for W, H in ((4, 1), (12, 11), (1280, 1024), (2048, 7)):
        for ctype, depth in a7.ALL_KINDS:
            kind = pt.kind_code(ctype, depth)
            want = ((a7.a7_size(W, H, ctype, depth) + 15) & ~15) + 16
            assert L.abub_png_raw_stride_adam7(W, H, kind | a7.ADAM7_FLAG) == want, (W, H, ctype, depth)
            assert L.abub_png_raw_stride_adam7(W, H, kind) == L.abub_png_raw_stride_kind(W, H, kind) > 0
        for kind in (2 | 4 << 8, 3 | 16 << 8, 5 | 8 << 8, 0 | 8 << 8, 1 << 17, 2 | 8 << 8 | 1 << 17):
            assert L.abub_png_raw_stride_adam7(W, H, kind) == 0 and L.abub_png_raw_stride_adam7(W, H, kind | a7.ADAM7_FLAG) == 0, hex(kind)
    assert L.abub_png_raw_stride_adam7(0, 5, a7.ADAM7_FLAG) == 0 and L.abub_png_raw_stride_adam7(4, 0, 2 | 8 << 8 | a7.ADAM7_FLAG) == 0


def test_host_repack_of_an_interlaced_run_verifies(tmp_path):
    host.build()
    W, H, F, NEV, NCAMS, run_id = 96, 64, 6, 2, 2, "20200925_1"
    rd = tmp_path / "data" / run_id
    rs = np.random.RandomState(3)
    for e in range(NEV):
        for c in range(NCAMS):
            st = synth.render_event(W, H, synth.random_spec(W, H, F, 40 + e, c, margin=10), 40 + e, c)
            d = rd / str(e) / "Images"
            d.mkdir(parents=True, exist_ok=True)
            for k in range(F):
                fts = [rs.randint(0, 5, H) for _ in range(7)]
                data = a7.make_adam7(st[k][:, :, None].astype(np.uint16), 0, 8, fts)
                assert np.array_equal(host.imdecode(data), st[k])
                (d / f"cam{c}_image{30 + k}.png").write_bytes(data)
    (rd / (run_id + ".txt")).write_text("".join(f"{run_id} {e} a b c d e f g h i\n" for e in range(NEV)))
    out = tmp_path / "packed"
    env = dict(os.environ, ABUB_NUM_CAMS=str(NCAMS), ABUB_THREADS="4")
    r = subprocess.run([EXE, "-d", str(rd.parent), "-r", run_id, "--repack", str(out), "--verify-repack", str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    src, other = host.Run("raw", str(rd) + "/", "Images"), host.Run("raw", str(out / run_id) + "/", "Images")
    try:
        v = src.verify(other, nthreads=4, ncams=NCAMS)
    finally:
        src.close()
        other.close()
    total = F * NEV * NCAMS
    assert v["rc"] == 0 and v["frames"] == v["same"] == total and v["undecodable"] == v["copied"] == v["differ"] == 0, v
