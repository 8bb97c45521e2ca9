"""PNG files of every non-interlaced type, written from samples the test chose, and the 8-bit grey value each pixel must get.

The writer takes the samples [H, W, samples per pixel], the colour type, the bit depth and one filter type per row; it is the
encoder side of the PNG specification (section 9: the filters work on bytes, at a distance of one pixel's bytes, one byte
below 8 bits per pixel) and knows nothing of any decoder.  `expected` is the rule a decoder to 8-bit grey follows
(cv::imdecode(..., 0) as host/cvlite.cpp restates it): the expected pixels of a test come from its samples, not from a decoder."""
import functools
import struct
import zlib

import numpy as np

SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# the 13 kinds abub_png_decode_typed_dev adds to the two 8-bit ones of abub_png_decode_dev: (colour type, bit depth)
TYPED_KINDS = [(0, 1), (0, 2), (0, 4), (0, 16), (3, 1), (3, 2), (3, 4), (4, 8), (4, 16), (2, 8), (2, 16), (6, 8), (6, 16)]
EIGHT_BIT_KINDS = [(0, 8), (3, 8)]


def kind_code(ctype, depth):
    """abub_png_frame.kind"""
    return 0 if (ctype, depth) in EIGHT_BIT_KINDS else ctype | depth << 8


def kind_name(ctype, depth):
    return {0: "grey", 2: "rgb", 3: "palette", 4: "grey+alpha", 6: "rgba"}[ctype] + str(depth)


def row_bytes(W, ctype, depth):
    return (W * SAMPLES[ctype] * depth + 7) // 8


def filter_distance(ctype, depth):
    return max(1, SAMPLES[ctype] * depth // 8)


def rgb2grey(r, g, b):
    return (np.asarray(r, np.int64) * 9797 + np.asarray(g, np.int64) * 19234 + np.asarray(b, np.int64) * 3737 + 16384) >> 15


# RGB triples at the conversion's extremes: black, white, the primaries, and neighbours (r, g, b) / (r + 1, g, b) ... across
# which (r * 9797 + g * 19234 + b * 3737 + 16384) >> 15 steps up (the weighted sum passes k * 32768 + 16384)
@functools.lru_cache(None)
def rgb_extremes():
    out = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    for r in range(256):
        for g in (0, 1, 127, 254, 255):
            for b in (0, 128, 255):
                if r + 1 < 256 and rgb2grey(r, g, b) != rgb2grey(r + 1, g, b):
                    out += [(r, g, b), (r + 1, g, b)]
    return tuple(out[:200])


def random_samples(rs, ctype, depth, W, H):
    """[H, W, samples] uint16: every bit of every sample random (so the low bytes of 16-bit samples and the alpha differ from
    what a pixel's grey comes from); half of the pixels of a colour image, at most, are the triples of rgb_extremes."""
    s = rs.randint(0, 1 << depth, size=(H, W, SAMPLES[ctype])).astype(np.uint16)
    if ctype in (2, 6) and W * H >= 16:
        ext = np.array(rgb_extremes(), np.uint16)
        n = min(len(ext), W * H // 2)
        flat = s.reshape(-1, SAMPLES[ctype])
        at = rs.choice(W * H, n, replace=False)
        low = rs.randint(0, 256, size=(n, 3)).astype(np.uint16) if depth == 16 else 0
        flat[at, :3] = (ext[:n] << 8 | low) if depth == 16 else ext[:n]
    return s


def random_palette(rs, n):
    return rs.randint(0, 256, size=(n, 3)).astype(np.uint8)


def expected(samples, ctype, depth, palette=None):
    """the 8-bit grey image [H, W] of the samples"""
    s = samples.astype(np.int64)
    if ctype == 3:
        npal = 0 if palette is None else len(palette)
        table = np.zeros(1 << depth, np.int64)
        if npal:
            p = np.asarray(palette, np.int64)[:1 << depth]
            table[:len(p)] = rgb2grey(p[:, 0], p[:, 1], p[:, 2])
        return table[s[:, :, 0]].astype(np.uint8)
    hi = s >> 8 if depth == 16 else s  # (16 -> 8 bits: the high byte)
    if ctype in (0, 4):
        v = hi[:, :, 0]
        if depth < 8:
            v = v * 255 // ((1 << depth) - 1)
        return v.astype(np.uint8)
    return rgb2grey(hi[:, :, 0], hi[:, :, 1], hi[:, :, 2]).astype(np.uint8)


def pack_rows(samples, depth, pad_bits=1):
    """[H, W, S] samples -> the unfiltered scanlines [H, row bytes] (u8): big-endian 16-bit samples, pixels below 8 bits MSB
    first within a byte, the unused low bits of a row's last byte filled with pad_bits (they belong to no pixel)"""
    H, W, S = samples.shape
    if depth == 16:
        return np.stack([samples >> 8, samples & 255], axis=-1).astype(np.uint8).reshape(H, W * S * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(H, W * S)
    bits = ((samples.reshape(H, W * S, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1)) & 1).reshape(H, W * S * depth)
    pad = (-bits.shape[1]) % 8
    if pad:
        bits = np.concatenate([bits, np.full((H, pad), pad_bits, np.uint8)], axis=1)
    return np.packbits(bits, axis=1)


def filter_rows(rows, bpp, fts):
    """the scanlines filtered, row y with filter type fts[y] (a type above 4 leaves the bytes as they are): -> the bytes of
    the stream a PNG's IDAT chunks deflate, H x (1 + row bytes)"""
    H, n = rows.shape
    out = np.zeros((H, n + 1), np.uint8)
    r = rows.astype(np.int64)
    for y in range(H):
        cur = r[y]
        up = r[y - 1] if y else np.zeros(n, np.int64)
        # the byte one filter distance to the left, in this row and in the row above (zeros before the row's first pixel)
        left = np.concatenate([np.zeros(bpp, np.int64), cur])[:n]
        upleft = np.concatenate([np.zeros(bpp, np.int64), up])[:n]
        ft = int(fts[y])
        if ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - up
        elif ft == 3:
            f = cur - ((left + up) >> 1)
        elif ft == 4:
            p = left + up - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
            f = cur - pred
        else:
            f = cur
        out[y, 0] = ft
        out[y, 1:] = (f & 255).astype(np.uint8)
    return out


def chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xFFFFFFFF)


def png_file(W, H, ctype, depth, stream, palette=None, interlace=0, idat=1, extra=()):
    """a PNG file around the (already filtered) scanline bytes `stream`: IHDR, `extra` chunks [(type, data)], PLTE for a
    palette, the zlib stream cut into `idat` IDAT chunks, IEND"""
    z = zlib.compress(bytes(stream), 6)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))
    for typ, data in extra:
        out += chunk(typ, data)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    cut = [len(z) * k // idat for k in range(idat + 1)]
    for k in range(idat):
        out += chunk(b"IDAT", z[cut[k]:cut[k + 1]])
    return out + chunk(b"IEND", b"")


def make_png(samples, ctype, depth, fts, palette=None, **kw):
    """the PNG file of the samples [H, W, S], row y filtered with type fts[y]"""
    H, W, _ = samples.shape
    rows = pack_rows(samples, depth)
    assert rows.shape[1] == row_bytes(W, ctype, depth)
    return png_file(W, H, ctype, depth, filter_rows(rows, filter_distance(ctype, depth), fts).tobytes(), palette, **kw)


def filter_sequence(first):
    """ten filter types that start with `first` and hold `first` followed by each of the five types (first, 0, first, 1, ...):
    the five sequences together hold every type after every other"""
    return [t for b in range(5) for t in (first, b)]
