"""Raw deflate streams (RFC 1951, what a zip entry of method 8 holds) for the tests of abub_unzip_dev: streams zlib wrote at
every level and strategy, hand-written ones (deflatecraft), and the refusals, each with the verdict zlib's Z_FINISH gives it;
and the layout of a batch: streams and outputs at multiples of 16 with canaries around them."""
import os
import re
import zlib

import numpy as np

import deflatecraft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the edges of the 16-byte flush, the 512-byte pass and the 32768 + 512 ring
LENGTHS = (0, 1, 15, 16, 17, 511, 512, 513, 32767, 32768, 32769, 33279, 33280, 33281, 100000)
LEVELS = (0, 1, 6, 9, "fixed")
CANARY_IN, CANARY_OUT, GAP = 0xFF, 0xC3, 32


def align16(n):
    return (n + 15) & ~15


def status_codes():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ABUB_(?:PNG|ZIP)_E_(\w+) (\d+)", hdr)
            if m.group(0).startswith("#define ABUB_ZIP") or m.group(1) != "DESC"}


def deflate_raw(data, level):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED) if level == "fixed" else zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(bytes(data)) + c.flush()


class Case:
    """one entry: the stream, what the descriptor states, and the status the kernel must give (None: accepted)"""

    def __init__(self, name, z, raw, code=None, ulen=None, crc=None, desc=None):
        self.name, self.z, self.raw, self.code, self.desc = name, bytes(z), bytes(raw), code, desc
        self.ulen = len(self.raw) if ulen is None else ulen
        self.crc = (zlib.crc32(self.raw) & 0xFFFFFFFF) if crc is None else crc


def zlib_verdict(c):
    """what ZipParser::readEntry does: inflate with Z_FINISH into ulen bytes, accept iff the stream ended and filled them,
    then the CRC-32"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(c.z)
    except zlib.error:
        return False
    return d.eof and len(out) == c.ulen and (zlib.crc32(out) & 0xFFFFFFFF) == c.crc


def contents(n, rs):
    yield "zeros", bytes(n)                                              # distance-1 matches, overlapping copies
    yield "period", (b"abcdefg" * (n // 7 + 1))[:n]                      # a short period
    yield "random", bytes(rs.randint(0, 256, n).astype(np.uint8))        # literals only


def png_file(W=320, H=200):
    """a PNG file whose zip layer is nearly incompressible"""
    rs = np.random.RandomState(5)
    img = (np.add.outer(np.arange(H), np.arange(W)) // 3 + rs.randint(0, 4, (H, W))).astype(np.uint8)
    rows = b"".join(b"\x00" + img[y].tobytes() for y in range(H))
    return dc.png_of(zlib.compress(rows, 1), W, H)


def bmp_file(W=1280, H=1024):
    import bmpfiles
    rs = np.random.RandomState(6)
    img = (np.add.outer(np.arange(H), np.arange(W)) // 9 + rs.randint(0, 3, (H, W))).astype(np.uint8)
    return bmpfiles.make_bmp(img, 8)


def good_cases():
    rs = np.random.RandomState(1)
    out = []
    for n in LENGTHS:
        for kind, data in contents(n, rs):
            for level in LEVELS:
                out.append(Case(f"{kind}-{n}-L{level}", deflate_raw(data, level), data))
    png = png_file()
    for level in LEVELS:
        out.append(Case(f"png-L{level}", deflate_raw(png, level), png))
    bmp = bmp_file()
    out.append(Case("bmp-1280x1024-L1", deflate_raw(bmp, 1), bmp))
    return out + crafted_good()


def lits(b, rs, n):
    for v in rs.randint(0, 5, n):
        b.lit(int(v))


def crafted_good():
    rs = np.random.RandomState(2)
    out = []
    s = dc.Stream()  # distances 32768 and 1
    s.stored(bytes(rs.randint(0, 5, 32768).astype(np.uint8)), False)
    b = s.fixed(True)
    b.match(258, 32768)
    b.match(3, 32768)
    lits(b, rs, 7)
    b.match(258, 1)
    b.match(3, 1)
    b.match(9, 32768)
    b.eob()
    out.append(Case("dist-32768-and-1", s.body(), s.raw))
    s = dc.Stream()  # 15-bit codes: lengths 1, 2, ..., 14, 15, 15 in both alphabets; the tokens use the 15-bit ones
    s.stored(bytes(rs.randint(0, 5, 32768).astype(np.uint8)), False)
    litlens, distlens = [0] * 286, [0] * 30
    for sym, l in zip([0, 1, 2, 4, 256] + list(range(257, 266)) + [3, 285], list(range(1, 16)) + [15]):
        litlens[sym] = l
    for sym, l in zip(list(range(14)) + [28, 29], list(range(1, 16)) + [15]):
        distlens[sym] = l
    b = s.dynamic(True, litlens, distlens)
    for dist in (32768, 16385, 24576, 24577):
        b.match(258, dist)
        b.lit(3)
    b.eob()
    out.append(Case("15-bit-codes", s.body(), s.raw))
    s = dc.Stream()  # a block that holds nothing but its end-of-block code, between two that hold data
    b = s.fixed(False)
    lits(b, rs, 20)
    b.eob()
    b = s.fixed(False)
    b.eob()
    b = s.dynamic(False, [0] * 256 + [1], [0])
    b.eob()
    b = s.fixed(True)
    lits(b, rs, 20)
    b.eob()
    out.append(Case("eob-only-blocks", s.body(), s.raw))
    s = dc.Stream()  # a stored block behind a block that ended inside a byte
    b = s.fixed(False)
    lits(b, rs, 3)
    b.eob()
    assert s.w.n != 0
    s.stored(b"stored behind a block that ended inside a byte", False)
    b = s.fixed(True)
    b.match(20, 30)
    b.eob()
    out.append(Case("stored-after-partial-byte", s.body(), s.raw))
    s = dc.Stream()  # ulen == 0: an empty final block of each kind
    s.fixed(True).eob()
    out.append(Case("empty-fixed", s.body(), b""))
    s = dc.Stream()
    s.stored(b"", True)
    out.append(Case("empty-stored", s.body(), b""))
    data = bytes(rs.randint(0, 7, 3000).astype(np.uint8))  # bytes behind the final block are not the stream's
    out.append(Case("trailing-bytes", deflate_raw(data, 6) + b"\x07\xff\x00behind the end" * 3, data))
    return out


def refused_cases():
    """(the three descriptor cases are made by the batch's layout: Batch(..., desc=...))"""
    rs = np.random.RandomState(3)
    data = bytes(rs.randint(0, 9, 5000).astype(np.uint8))
    z = deflate_raw(data, 6)
    out = []
    for cut in (len(z) // 2, len(z) - 1, 1, 7, len(z) // 3):  # inside the data, before the last byte, inside the header
        out.append(Case(f"truncated-at-{cut}", z[:cut], data, "TRUNCATED"))
    z0 = deflate_raw(data, 0)
    out.append(Case("truncated-stored", z0[:len(z0) // 2], data, "TRUNCATED"))
    out.append(Case("truncated-stored-header", z0[:3], data, "TRUNCATED"))
    out.append(Case("block-type-3", b"\x07\x00\x00\x00", b"", "BLOCKTYPE"))
    out.append(Case("len-nlen", b"\x01\x05\x00\xfa\xfehello", b"hello", "STORED"))
    s = dc.Stream()
    s.dynamic(True, [1, 1, 1] + [0] * 253 + [2], [1, 1])
    out.append(Case("over-subscribed", s.body() + bytes(8), b"", "CODES"))
    s = dc.Stream()
    b = s.fixed(True)
    b.lit(1)
    b.match(3, 2)
    b.eob()
    out.append(Case("distance-before-start", s.body(), s.raw, "DISTANCE"))
    out.append(Case("one-byte-more", z, data[:-1], "TOOMUCH", crc=0))
    out.append(Case("one-byte-fewer", z, data + b"\x00", "TOOLITTLE", crc=0))
    for n in (1, 513, 5000):
        out.append(Case(f"crc-one-bit-{n}", deflate_raw(data[:n], 6), data[:n], "CRC", crc=(zlib.crc32(data[:n]) ^ (1 << (n % 32))) & 0xFFFFFFFF))
    out.append(Case("off-misaligned", z, data, "DESC", desc="off"))
    out.append(Case("dst-past-out", z, data, "DESC", desc="dst"))
    out.append(Case("clen-past-comp", z, data, "DESC", desc="clen"))
    return out


class Batch:
    """comp: every stream at a multiple of 16, CANARY_IN behind it (the kernel must read those bytes as zeros), align16(clen)
    + 16 readable; out: every entry at a multiple of 16, GAP canary bytes between entries and behind the last."""

    def __init__(self, cases):
        self.cases = list(cases)
        comp, rows, pos = bytearray(), [], 0
        for c in self.cases:
            off = len(comp)
            comp += c.z + bytes([CANARY_IN]) * (align16(len(c.z)) - len(c.z) + 16)
            rows.append([off, len(c.z), c.ulen, c.crc, pos])
            pos += align16(c.ulen) + GAP
        self.comp, self.out_bytes = bytes(comp), pos
        for c, r in zip(self.cases, rows):
            if c.desc == "off":       # (the stream is there: only the alignment is wrong)
                r[0] += 4
                r[1] -= 4
            elif c.desc == "dst":     # room for ulen, but not for ulen rounded up to 16 plus the entry's place
                r[4] = align16(self.out_bytes - c.ulen + 1)
            elif c.desc == "clen":    # off + clen lies past comp_bytes
                r[0], r[1] = len(self.comp) - 32, 100
        self.rows = rows

    def expected(self):
        """the bytes of `out` after the call where they are known: canaries everywhere but inside the entries; inside an
        accepted entry its data; a descriptor refusal leaves its place untouched.  -> (bytes, mask of the known ones)"""
        want = np.full(self.out_bytes, CANARY_OUT, dtype=np.uint8)
        known = np.ones(self.out_bytes, dtype=bool)
        pos = 0
        for c in self.cases:
            if c.code is None:
                want[pos:pos + c.ulen] = np.frombuffer(c.raw, dtype=np.uint8)
            elif c.code != "DESC":
                known[pos:pos + align16(c.ulen)] = False  # (a refused entry may be partly written inside its own range)
            pos += align16(c.ulen) + GAP
        return want, known

    def want_status(self, codes):
        return [0 if c.code is None else codes[c.code] for c in self.cases]


def write_zip(path, entries):
    """A zip archive written by hand, for what zipfile does not write: entries = [(name, data, method, stream, crc)], stream
    None: `data` stored or deflated at level 6, else the bytes to put there (a stream cut short); crc None: that of `data`,
    else the value both headers state (a wrong one).  A name that ends in "/" is a directory."""
    import struct
    out, cd = bytearray(), bytearray()
    for name, data, method, stream, crc in entries:
        if stream is None:
            stream = data if method == 0 else deflate_raw(data, 6)
        if crc is None:
            crc = zlib.crc32(data) & 0xFFFFFFFF
        nm = name.encode()
        off = len(out)
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, method, 0, 0x21, crc, len(stream), len(data), len(nm), 0) + nm + stream
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, 0, method, 0, 0x21, crc, len(stream), len(data), len(nm), 0, 0, 0, 0,
                          0x10 if name.endswith("/") else 0, off) + nm
    eocd = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(entries), len(entries), len(cd), len(out), 0)
    open(path, "wb").write(bytes(out + cd) + eocd)
