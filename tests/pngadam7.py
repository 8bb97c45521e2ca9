"""Adam7-interlaced PNG files of every kind, written from samples the test chose (tests/pngtypes.py writes the non-interlaced
ones; the expected pixels are pngtypes.expected of the same samples: interlace changes where a pixel lies in the stream, not
its value).

PNG specification, section 8.2: pass p holds the pixels (y0 + r * dy, x0 + c * dx) of the image; a pass with pixels is an
image of its own -- pw x ph pixels, packed into scanlines that start on a byte boundary, filtered with zeros above its first
row -- and the stream is the scanlines of the passes one after the other; a pass without pixels is not in it.  The writer is
the encoder side and knows nothing of any decoder."""
import pngtypes as pt

# (x0, y0, dx, dy) of pass 1 .. 7
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
ADAM7_FLAG = 1 << 16  # ABUB_PNG_KIND_ADAM7
ALL_KINDS = pt.EIGHT_BIT_KINDS + pt.TYPED_KINDS


def pass_dims(W, H, p):
    """(pw, ph) of pass p = 0 .. 6"""
    x0, y0, dx, dy = PASSES[p]
    return (-(-(W - x0) // dx) if W > x0 else 0), (-(-(H - y0) // dy) if H > y0 else 0)


def present(W, H):
    """the passes that have pixels"""
    return [p for p in range(7) if all(pass_dims(W, H, p))]


def a7_size(W, H, ctype, depth):
    """bytes of the inflated stream: the scanlines (filter type + row) of the passes that have pixels"""
    n = 0
    for p in present(W, H):
        pw, ph = pass_dims(W, H, p)
        n += ph * (pt.row_bytes(pw, ctype, depth) + 1)
    return n


def pass_filters(first):
    """fts(p, r), the filter type of row r of pass p: pngtypes.filter_sequence(first) entered at 2 * p, so `first` is on the
    first row of every pass, and the type that follows it differs from pass to pass"""
    seq = pt.filter_sequence(first)
    return lambda p, r: seq[(2 * p + r) % len(seq)]


def adam7_stream(samples, ctype, depth, fts):
    """the filtered scanlines of the passes of samples [H, W, S]; fts(p, r) or fts[p][r] is the filter type of row r of pass p"""
    H, W, _ = samples.shape
    out = b""
    for p in present(W, H):
        x0, y0, dx, dy = PASSES[p]
        sub = samples[y0::dy, x0::dx]
        assert sub.shape[:2] == pass_dims(W, H, p)[::-1]
        types = [fts(p, r) if callable(fts) else fts[p][r] for r in range(sub.shape[0])]
        out += pt.filter_rows(pt.pack_rows(sub, depth), pt.filter_distance(ctype, depth), types).tobytes()
    assert len(out) == a7_size(W, H, ctype, depth)
    return out


def make_adam7(samples, ctype, depth, fts, palette=None, **kw):
    """the Adam7-interlaced PNG file of the samples [H, W, S]"""
    H, W, _ = samples.shape
    return pt.png_file(W, H, ctype, depth, adam7_stream(samples, ctype, depth, fts), palette, interlace=1, **kw)
