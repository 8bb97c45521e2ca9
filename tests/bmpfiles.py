"""BMP files built by hand for the tests of the BMP walk and the GPU BMP decoder, and a numpy decode from the walk's
fields (host/bmpwalk.hpp; the definition is decodeBMP, host/cvlite.cpp)."""
import io
import struct

import numpy as np
from PIL import Image


def grey_palette(n=256):
    v = (np.arange(n) * 255 // max(n - 1, 1)).astype(np.uint8)
    return np.stack([v, v, v, np.zeros(n, np.uint8)], axis=1)


def make_bmp(pix, bpp, top_down=False, hdr=40, comp=0, ncol=0, palette=None, gap=0, fill=0xA5):
    """pix: [H, W] indices (bpp 1, 4, 8) or [H, W, 3 | 4] bytes in file order (b, g, r[, x]); palette: [n, 4] (b, g, r, 0)
    written behind the header as it is (None: a grey ramp of 1 << bpp entries; bpp > 8: none); ncol: the header's colour
    count as it is; gap: bytes between palette and pixels; rows are padded with `fill`."""
    pix = np.asarray(pix, np.uint8)
    H, W = pix.shape[:2]
    stride = (W * bpp + 31) // 32 * 4
    rows = np.full((H, stride), fill, np.uint8)
    if bpp == 8:
        rows[:, :W] = pix
    elif bpp == 4:
        p = np.zeros((H, (W + 1) // 2 * 2), np.uint8)
        p[:, :W] = pix & 15
        rows[:, :(W + 1) // 2] = (p[:, 0::2] << 4) | p[:, 1::2]
    elif bpp == 1:
        rows[:, :(W + 7) // 8] = np.packbits(pix & 1, axis=1)
    else:
        rows[:, :W * (bpp // 8)] = pix.reshape(H, -1)
    if not top_down:
        rows = rows[::-1]
    if palette is None:
        palette = grey_palette(1 << bpp) if bpp <= 8 else np.zeros((0, 4), np.uint8)
    pal = np.asarray(palette, np.uint8).tobytes()
    data_off = 14 + hdr + len(pal) + gap
    head = struct.pack("<2sIHHI", b"BM", data_off + rows.size, 0, 0, data_off)
    info = struct.pack("<IiiHHIIiiII", hdr, W, -H if top_down else H, 1, bpp, comp, rows.size, 2835, 2835, ncol, 0)
    info += bytes(hdr - 40)
    return head + info + pal + bytes([0x5A]) * gap + rows.tobytes()


def pillow_bmp(img, mode, palette_seed=None):
    """img u8 [H, W] saved by Pillow as mode L, P (palette shuffled with palette_seed), 1 or RGB"""
    im = Image.fromarray(img)
    if mode == "1":
        im = Image.fromarray(img > 127)
    elif mode == "P":
        im = im.convert("P")
        if palette_seed is not None:
            rng = np.random.RandomState(palette_seed)
            im.putpalette(rng.randint(0, 256, 768).astype(np.uint8).tobytes())
    elif mode != "L":
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, format="BMP")
    return b.getvalue()


def decode_with(info, data, W, H):
    """the image from the walk's fields (data_off, stride, bpp, top_down, lut) alone"""
    a = np.frombuffer(data, np.uint8)
    off, stride, bpp = info["data_off"], info["stride"], info["bpp"]
    rows = a[off:off + stride * H].reshape(H, stride)
    if not info["top_down"]:
        rows = rows[::-1]
    lut = np.frombuffer(info["lut"], np.uint8)
    if bpp == 8:
        return lut[rows[:, :W]]
    if bpp == 4:
        idx = np.stack([rows >> 4, rows & 15], axis=2).reshape(H, -1)[:, :W]
        return lut[idx]
    if bpp == 1:
        return lut[np.unpackbits(rows, axis=1)[:, :W]]
    n = bpp // 8
    p = rows[:, :W * n].reshape(H, W, n).astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)
