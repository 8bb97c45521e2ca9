"""A deflate WRITER for tests (RFC 1950 / 1951), in plain Python with no compressor in it: a test spells out the blocks,
the code lengths and every token of a stream, so it can use the parts of the format a compressor never chooses (far
distances, 15-bit codes, repeats that run from the literal/length lengths into the distance lengths, degenerate
alphabets, reserved symbols, empty blocks).  The writer is the specification of those tests: keep it small and obvious.

    s = Stream()
    s.stored(data, final)                      # a stored block
    b = s.fixed(final)                         # a block of the fixed code ...
    b = s.dynamic(final, litlens, distlens)    # ... or of the code with these lengths; then tokens, then b.eob()
    b.lit(3); b.match(258, 32768); b.lensym(286); b.distsym(30); b.bits(1, 1); b.eob()
    z = zwrap(s.body(), s.raw)           # the zlib stream; s.raw = the bytes the blocks inflate to
    png = png_of(z, W, H, idat=100)      # an 8-bit grey PNG whose IDAT chunks carry z
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """bits go out LSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: its most significant bit first"""
        for k in range(n - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def data(self, data):
        assert self.n == 0
        self.out += data


def canonical_codes(lens):
    """code lengths -> [(code, length)] per symbol (RFC 1951 3.2.2); no check that the code is complete"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append((nxt[l], l))
        if l:
            nxt[l] += 1
    return out


def flat_lengths(n, used=None, size=None):
    """lengths of a complete code for n symbols (two neighbouring lengths); `used` places them in an alphabet of `size`"""
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lens = [k - 1] * short + [k] * (n - short)
    if used is None:
        return lens
    full = [0] * size
    for s, l in zip(sorted(used), lens):
        full[s] = l
    return full


def symbol_of(value, base, extra):
    for s in range(len(base) - 1, -1, -1):
        if value >= base[s] and value - base[s] < (1 << extra[s]):
            return s, value - base[s]
    raise ValueError(value)


class Block:
    """the tokens of one Huffman block; the stream's `raw` follows what an inflater would write"""

    def __init__(self, stream, litlens, distlens):
        self.s, self.w = stream, stream.w
        self.lc, self.dc = canonical_codes(litlens), canonical_codes(distlens)

    def _sym(self, codes, sym):
        code, n = codes[sym]
        assert n, f"symbol {sym} has no code in this block"
        self.w.code(code, n)

    def bits(self, value, n):
        """raw bits, for what no symbol spells (an unassigned code)"""
        self.w.bits(value, n)

    def lit(self, b):
        self._sym(self.lc, b)
        self.s.raw.append(b)

    def lensym(self, sym, extra=0, nextra=None):
        self._sym(self.lc, sym)
        self.w.bits(extra, LEN_EXTRA[sym - 257] if nextra is None else nextra)

    def distsym(self, sym, extra=0, nextra=None):
        self._sym(self.dc, sym)
        self.w.bits(extra, DIST_EXTRA[sym] if nextra is None else nextra)

    def match(self, length, dist, lsym=None):
        """lsym: the length symbol to use where two spell the length (258 = symbol 285, or 284 with extra 31)"""
        if lsym is None:
            ls, le = symbol_of(length, LEN_BASE, LEN_EXTRA)
        else:
            ls, le = lsym - 257, length - LEN_BASE[lsym - 257]
        ds, de = symbol_of(dist, DIST_BASE, DIST_EXTRA)
        self.lensym(257 + ls, le)
        self.distsym(ds, de)
        raw = self.s.raw
        for _ in range(length):  # (a distance before the first byte: the stream is invalid, what follows does not matter)
            raw.append(raw[-dist] if dist <= len(raw) else 0)

    def eob(self):
        self._sym(self.lc, 256)


class Stream:
    def __init__(self):
        self.w = BitWriter()
        self.raw = bytearray()

    def _head(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data=b"", final=False):
        assert len(data) < 65536
        self._head(final, 0)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits(len(data) ^ 0xFFFF, 16)
        self.w.data(data)
        self.raw += data

    def fixed(self, final=False):
        self._head(final, 1)
        return Block(self, FIXED_LIT, FIXED_DIST)

    def dynamic(self, final, litlens, distlens, clseq=None, hclen=19):
        """clseq: the code-length symbols as the stream carries them, [(symbol 0..18, extra bits' value)]: a repeat (16, 17,
        18) may run from the literal/length lengths into the distance lengths.  Default: one symbol per length."""
        assert 257 <= len(litlens) <= 286 and 1 <= len(distlens) <= 30
        if clseq is None:
            clseq = [(l, 0) for l in list(litlens) + list(distlens)]
        spelled = []
        for sym, extra in clseq:
            spelled += [sym] if sym < 16 else [spelled[-1]] * (3 + extra) if sym == 16 else [0] * ((3 if sym == 17 else 11) + extra)
        assert spelled == list(litlens) + list(distlens), "clseq does not spell the two length lists"
        used = sorted({sym for sym, _ in clseq})
        if len(used) == 1:  # the code-length code itself must be complete: a second, unused code
            used.append(1 if used[0] == 0 else 0)
        cllens = flat_lengths(len(used), used, 19)
        assert all(cllens[CL_ORDER[i]] == 0 for i in range(hclen, 19))
        self._head(final, 2)
        self.w.bits(len(litlens) - 257, 5)
        self.w.bits(len(distlens) - 1, 5)
        self.w.bits(hclen - 4, 4)
        for i in range(hclen):
            self.w.bits(cllens[CL_ORDER[i]], 3)
        clcodes = canonical_codes(cllens)
        for sym, extra in clseq:
            self.w.code(*clcodes[sym])
            if sym >= 16:
                self.w.bits(extra, CL_EXTRA[sym])
        return Block(self, litlens, distlens)

    def body(self):
        """the deflate stream so far, padded to a byte"""
        w = BitWriter()
        w.out, w.acc, w.n = bytearray(self.w.out), self.w.acc, self.w.n
        w.align()
        return bytes(w.out)


def zwrap(body, raw, cmf=0x78, flevel=2, fdict=False, adler=None):
    """RFC 1950: CMF, FLG (FCHECK makes the pair a multiple of 31), the deflate stream, the Adler-32 of `raw`"""
    flg = (flevel << 6) | (0x20 if fdict else 0)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31
    if adler is None:
        adler = zlib.adler32(bytes(raw)) & 0xFFFFFFFF
    return bytes([cmf, flg]) + bytes(body) + struct.pack(">I", adler)


def png_of(z, W, H, idat=1 << 30):
    """an 8-bit grey, non-interlaced PNG of W x H whose IDAT chunks carry z: chunks of `idat` bytes; idat = 0: an empty
    chunk in front, then one-byte chunks, then the rest (the pattern of test_gpu_png.make_png)"""
    from test_gpu_png import chunk
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0))
    if idat == 0:
        png += chunk(b"IDAT", b"")
        for k in range(min(5, len(z))):
            png += chunk(b"IDAT", z[k:k + 1])
        png += chunk(b"IDAT", z[5:])
    else:
        for k in range(0, len(z), idat):
            png += chunk(b"IDAT", z[k:k + idat])
    return png + chunk(b"IEND", b"")
