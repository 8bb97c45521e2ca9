"""The packed frame format "ABF1" restated in numpy, from its description alone ("Packed frames"): an encoder (canonical, or
with wider-than-needed widths), a decoder with the acceptance rules and the status codes of include/abub_hip.h, and a
seeded generator of damaged files.  Nothing here calls the project's codec: the tests compare against it.

Layout, little-endian: "ABF1", u32 W, H, nblk = ceil(W / 64), payload_bytes, 3 reserved words; H x {u32 off, u32 check};
H * nblk width bytes padded to a multiple of 4; payload.  Block (y, k): first pixel raw, then the zigzagged differences of
neighbours at widths[y, k] bits each, packed LSB first."""
import struct

import numpy as np

E_DESC, E_HEADER, E_SIZE, E_WIDTH, E_ROWS, E_CHECK = 1, 2, 3, 4, 5, 6


def _zigzag(d):
    s = d.astype(np.uint8).astype(np.int8).astype(np.int32)
    return ((s << 1) ^ (s >> 7)) & 0xFF


def _unzigzag(z):
    z = z.astype(np.int32)
    return ((z >> 1) ^ -(z & 1)) & 0xFF


def _bits_needed(zmax):
    return int(zmax).bit_length()


def regions(W, H):
    """(start of the row table, of the widths, of the payload)"""
    nblk = (W + 63) // 64
    return 32, 32 + 8 * H, 32 + 8 * H + ((H * nblk + 3) & ~3)


def encode(img, extra_bits=0):
    """img u8 [H, W] -> bytes.  extra_bits: every block of fewer than 8 bits gets that many more (non-minimal widths)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    nblk = (W + 63) // 64
    widths = np.zeros((H, nblk), np.uint8)
    table = np.zeros((H, 2), np.uint32)
    payload = bytearray()
    xs = np.arange(1, W + 1, dtype=np.uint64)
    for y in range(H):
        row = img[y]
        table[y, 0] = len(payload)
        table[y, 1] = int((xs * row.astype(np.uint64)).sum() & 0xFFFFFFFF)
        for k in range(nblk):
            p = row[64 * k:64 * k + 64].astype(np.int32)
            n = len(p)
            z = _zigzag((p[1:] - p[:-1]) & 0xFF)
            b = _bits_needed(z.max()) if n > 1 else 0
            b = min(8, b + extra_bits)
            widths[y, k] = b
            bits = np.zeros(((n - 1) * b + 7) // 8 * 8, np.uint8)
            for i in range(b):  # bit i of residual j is bit (j - 1) * b + i of the string
                bits[np.arange(n - 1) * b + i] = (z >> i) & 1
            payload.append(int(p[0]))
            payload += np.packbits(bits, bitorder="little").tobytes()
    wb = widths.tobytes()
    wb += b"\0" * (-len(wb) % 4)
    head = b"ABF1" + struct.pack("<7I", W, H, nblk, len(payload), 0, 0, 0)
    return head + table.astype("<u4").tobytes() + wb + bytes(payload)


def decode(data, W, H):
    """-> (status, image u8 [H, W]).  0 = accepted.  Header and size errors end the decode; of the row-level errors the
    largest code is reported, and a row whose widths or offsets are refused is not read."""
    img = np.zeros((H, W), np.uint8)
    data = bytes(data)
    nblk = (W + 63) // 64
    if len(data) < 32 or data[:4] != b"ABF1":
        return E_HEADER, img
    w, h, nb, payload_bytes = struct.unpack("<4I", data[4:20])
    if w != W or h != H or nb != nblk:
        return E_HEADER, img
    t0, w0, p0 = regions(W, H)
    if p0 + payload_bytes != len(data):
        return E_SIZE, img
    table = np.frombuffer(data, "<u4", 2 * H, t0).reshape(H, 2).astype(np.int64)
    widths = np.frombuffer(data, np.uint8, H * nblk, w0).reshape(H, nblk).astype(np.int64)
    pay = np.frombuffer(data, np.uint8, payload_bytes, p0)
    ns = np.minimum(64, W - 64 * np.arange(nblk))
    xs = np.arange(1, W + 1, dtype=np.uint64)
    err = 0
    for y in range(H):
        if (widths[y] > 8).any():
            err = max(err, E_WIDTH)
            continue
        sizes = 1 + ((ns - 1) * widths[y] + 7) // 8
        off, nxt = int(table[y, 0]), int(table[y + 1, 0]) if y + 1 < H else payload_bytes
        if (y == 0 and off != 0) or off + int(sizes.sum()) != nxt or off + int(sizes.sum()) > payload_bytes:
            err = max(err, E_ROWS)
            continue
        at = off
        for k in range(nblk):
            n, b = int(ns[k]), int(widths[y, k])
            blk = pay[at:at + int(sizes[k])]
            bits = np.unpackbits(blk[1:], bitorder="little")[:(n - 1) * b].reshape(n - 1, b) if b else np.zeros((n - 1, 0), np.uint8)
            z = (bits.astype(np.int32) << np.arange(b)).sum(axis=1) if b else np.zeros(n - 1, np.int32)
            d = np.concatenate([[int(blk[0])], _unzigzag(z)])
            img[y, 64 * k:64 * k + n] = np.cumsum(d) & 0xFF
            at += int(sizes[k])
        if int((xs * img[y].astype(np.uint64)).sum() & 0xFFFFFFFF) != int(table[y, 1]):
            err = max(err, E_CHECK)
    return err, img


KINDS = ("cut", "trailing", "width9", "rowoff", "check", "magic", "w4")
# where a file is cut: inside the magic, inside the header, at every region boundary, and inside the payload
CUTS = ("empty", "magic", "header", "table", "widths", "widths_end", "payload", "mid_payload")


def cut_position(name, W, H, size, rs):
    """byte count left of a file of `size` bytes cut at the named place; None where the file has no such place (a payload of
    a single byte has no inside)"""
    nblk = (W + 63) // 64
    t0, w0, p0 = regions(W, H)
    if name == "mid_payload":
        return p0 + 1 + int(rs.randint(size - p0 - 1)) if size > p0 + 1 else None
    return {"empty": 0, "magic": 4, "header": 31, "table": t0, "widths": w0, "widths_end": w0 + H * nblk, "payload": p0}[name]


def damage(data, W, H, rs, kind, cut=None):
    """One fault put into an intact file: -> (kind, or "cut:<place>"; bytes; the status a decoder must give).  cut: at the
    place `cut` names (CUTS); trailing: one byte more; width9: a width of 9; rowoff: a row offset shifted; check: a row
    check flipped; magic; w4: W + 4 in the header.  Which width, row, bit and shift is hit comes from rs."""
    data = bytearray(data)
    nblk = (W + 63) // 64
    t0, w0, p0 = regions(W, H)
    if kind == "cut":
        at = cut_position(cut, W, H, len(data), rs)
        assert at is not None and at < len(data), (cut, W, H)
        return "cut:" + cut, bytes(data[:at]), (E_HEADER if at < 32 else E_SIZE)
    if kind == "trailing":
        return kind, bytes(data) + b"\0", E_SIZE
    if kind == "width9":
        data[w0 + rs.randint(H * nblk)] = 9
        return kind, bytes(data), E_WIDTH
    if kind == "rowoff":
        y = rs.randint(H)
        o = t0 + 8 * y
        v = struct.unpack("<I", data[o:o + 4])[0]
        data[o:o + 4] = struct.pack("<I", (v + [1, 2, 64, 0x10000, 0xFFFFFFFF][rs.randint(5)]) & 0xFFFFFFFF)
        return kind, bytes(data), E_ROWS
    if kind == "check":
        o = t0 + 8 * rs.randint(H) + 4
        data[o + rs.randint(4)] ^= 1 << rs.randint(8)
        return kind, bytes(data), E_CHECK
    if kind == "magic":
        data[rs.randint(4)] ^= 0x20
        return kind, bytes(data), E_HEADER
    if kind == "w4":
        data[4:8] = struct.pack("<I", W + 4)
        return kind, bytes(data), E_HEADER
    raise ValueError(kind)


def contents(W, H, seed=0):
    """name -> image u8 [H, W]: the content classes of the tests (all zero, constant, uniform random, a ramp that wraps
    255 -> 0, sigma 1.6 noise)"""
    rs = np.random.RandomState(1000 + seed)
    out = {
        "zero": np.zeros((H, W), np.uint8),
        "constant": np.full((H, W), 173, np.uint8),
        "random": rs.randint(0, 256, (H, W)).astype(np.uint8),
        "ramp": ((np.arange(W)[None, :] * 3 + np.arange(H)[:, None] * 7 + 250) & 0xFF).astype(np.uint8),
        "noise": np.clip(np.rint(120 + rs.randn(H, W) * 1.6), 0, 255).astype(np.uint8),
    }
    return out
