"""PNG files whose deflate streams no compressor emits (written token by token with tests/deflatecraft.py): the cases,
and what can be said about them without a GPU -- zlib's verdict is the stated one, the host decoder (cv::imdecode, the one a
frame the GPU refuses falls back to) agrees with zlib and with Pillow.  tests/test_png_model.py runs the same cases through
the lane-level model of the GPU inflate, tests/test_gpu_png_crafted.py through the kernels.

Every raw byte of every stream is in 0 .. 4 (literals, stored data, match sources), so whatever lands on the first byte of
a scanline is a filter type and no stream has to be laid out around the rows."""
import collections
import functools
import io
import struct
import zlib

import numpy as np

import deflatecraft as dc

Case = collections.namedtuple("Case", "name W H png accepts code")  # code: the documented status the cause maps to, or None
SMALL, WIDE = (64, 600), (2048, 18)   # 39,000 and 36,882 raw bytes: a 32,768-byte history, a wrapped ring, room for the tokens
IDATS = (1 << 30, 100, 0)            # one chunk; 100-byte chunks; an empty chunk, five one-byte chunks, the rest


def rnd(rs, n):
    return bytes(rs.randint(0, 5, n).astype(np.uint8))


def lits(b, rs, n):
    for v in rs.randint(0, 5, n):
        b.lit(int(v))


def fill(b, s, rs, upto):
    lits(b, rs, upto - len(s.raw))


def eobonly(distlens):
    return [0] * 256 + [1], distlens


def case_A(rs, size):
    s = dc.Stream()
    s.stored(rnd(rs, 32768), False)
    b = s.fixed(True)
    b.match(258, 32768)  # two long matches back to back: one record carries more than the ring's spare 512 bytes
    b.match(258, 32768)
    pre = [0, 1, 3, 7, 15, 16, 17, 33, 64, 127]
    k = 0
    for dist in (32768, 32767, 32507, 1, 2):
        for length in (3, 8, 9, 64, 258):
            lits(b, rs, pre[k % len(pre)])  # the match lands first in a record, late in one, at varied offsets of a pass
            k += 1
            b.match(length, dist)
    while size - len(s.raw) >= 3:  # far matches until the frame is full: the ring wraps under them
        b.match(min(258, size - len(s.raw)), 32768 - (len(s.raw) & 1))
    fill(b, s, rs, size)
    b.eob()
    return s


def case_A_margin(rs, size):
    """The writing side copies a short match by its own lane when its source ends before the pass's first byte, and a pass
    writes at most 512 bytes into a ring of 32768 + 512: a source at distance 32768 at pass offset 0 is the first byte a
    full pass does not overwrite.  A pass is what one record (128 bits of the block, counted from its first token) holds,
    so each construct opens a block of its own: a short match at distance 32768 (32767, 32507), then two long ones that
    fill the pass to exactly 512 bytes, then the end of the block."""
    s = dc.Stream()
    s.stored(rnd(rs, 32768), False)
    b = s.fixed(False)
    lits(b, rs, 516)    # past the ring's end (33280): the passes from here on take the straight-line path
    b.eob()
    b = s.fixed(False)
    b.match(8, 9)       # at ring offset 4, its source the ring's last 5 bytes and first 3 (read from their copy behind the end)
    b.eob()
    for dist in (32768, 32767, 32507):
        for short in (3, 5, 6, 8) if dist == 32768 else (3, 8):
            b = s.fixed(False)
            b.match(short, dist)
            b.match(258, 32768)
            b.match(512 - 258 - short, 32768)
            b.eob()
    b = s.fixed(True)
    fill(b, s, rs, size)
    b.eob()
    return s


def long_code_block(s, rs, size, five_extra):
    """16 used literal/length and 16 used distance symbols with code lengths 1, 2, ..., 14, 15, 15; the symbols the tokens use
    have the 15-bit codes"""
    litlens, distlens = [0] * 286, [0] * 30
    if five_extra:  # length symbols 283 and 284 (5 extra bits) at 15 bits: 15 + 5 + 15 + 13 = 48 bits per token
        order = [0, 1, 2, 4, 256, 3] + list(range(257, 265)) + [283, 284]
    else:           # length symbol 285 and literal 3 at 15 bits: 15 + 0 + 15 + 13 = 43 bits per token
        order = [0, 1, 2, 4, 256] + list(range(257, 266)) + [3, 285]
    for sym, l in zip(order, list(range(1, 16)) + [15]):
        litlens[sym] = l
    for sym, l in zip(list(range(14)) + [28, 29], list(range(1, 16)) + [15]):
        distlens[sym] = l
    b = s.dynamic(True, litlens, distlens)
    for edge in (32768, 16385, 24576, 24577):  # the ends of the two distance symbols' ranges
        b.match(226 if five_extra else 258, edge)
    while size - len(s.raw) >= 258:
        dist = int(rs.randint(16385, 32769))
        if five_extra:
            b.match(int(rs.randint(195, 258)), dist)
        else:
            b.match(258, dist)
            if rs.randint(0, 3) == 0:
                b.lit(3)
    while len(s.raw) < size:
        b.lit(3)
    b.eob()


def case_B(rs, size, five_extra):
    s = dc.Stream()
    s.stored(rnd(rs, 32768), False)
    long_code_block(s, rs, size, five_extra)
    return s


def case_C(rs, size):
    litlens = [10] * 56 + [9] * 228 + [2, 2]
    distlens = [2, 2, 3, 3, 3, 3]
    # ..., 2, 16 (repeat 3), 3, 16 (repeat 3): the first repeat covers literal/length 285 and distances 0 and 1
    clseq = [(10, 0)] * 56 + [(9, 0)] * 228 + [(2, 0), (16, 0), (3, 0), (16, 0)]
    s = dc.Stream()
    b = s.dynamic(True, litlens, distlens, clseq=clseq)
    lits(b, rs, 40)
    while size - len(s.raw) >= 300:
        lits(b, rs, int(rs.randint(0, 20)))
        if rs.randint(0, 2):
            b.match(258, int(rs.randint(1, 9)))
        else:
            b.match(int(rs.randint(227, 258)), int(rs.randint(1, 9)))  # symbol 284
    fill(b, s, rs, size)
    b.eob()
    return s


def case_D(rs, size, with_length_code):
    if with_length_code:  # D': length symbol 257 has a code and is used once, and there is no distance code to follow it
        litlens = [8] * 254 + [9] * 4
    else:
        litlens = [8] * 255 + [9] * 2
    s = dc.Stream()
    b = s.dynamic(True, litlens, [0])
    lits(b, rs, 5000)
    if with_length_code:
        b.lensym(257)
        b.bits(0, 1)
    fill(b, s, rs, size)
    b.eob()
    return s


def case_E(rs, size, unassigned):
    s = dc.Stream()
    b = s.dynamic(True, dc.flat_lengths(286), [1])  # a lone 1-bit distance code: distance 1 is code 0, code 1 is nobody's
    lits(b, rs, 100)
    n = 0
    while size - len(s.raw) >= 300:
        lits(b, rs, int(rs.randint(0, 30)))
        if unassigned and n == 20:
            b.lensym(260)
            b.bits(1, 1)
        else:
            b.match(int(rs.randint(3, 259)), 1)
        n += 1
    fill(b, s, rs, size)
    b.eob()
    return s


def case_F(rs, size):
    s = dc.Stream()
    for _ in range(5):
        s.stored(b"", False)
    b = s.fixed(False)
    lits(b, rs, 3001)
    b.match(100, 7)
    b.eob()
    probe = dc.Stream()
    probe.dynamic(False, *eobonly([0])).eob()
    if (s.w.n + probe.w.n) % 8 == 0:             # (the next block has to end inside a byte: shift it by 10 bits)
        s.fixed(False).eob()
    s.dynamic(False, *eobonly([0])).eob()        # a block of nothing but a 1-bit end-of-block
    assert s.w.n != 0
    s.stored(rnd(rs, 20000), False)              # ... and a stored block straight after it
    s.dynamic(False, *eobonly([1])).eob()        # the same with a lone 1-bit distance code
    s.fixed(False).eob()                         # an empty fixed block
    b = s.fixed(False)
    b.match(258, 20001)
    fill(b, s, rs, size)
    b.eob()
    s.stored(b"", True)                          # an empty final stored block
    return s


def case_H(rs, size, which):
    s = dc.Stream()
    b = s.fixed(True)
    lits(b, rs, 700)
    if which in (286, 287):   # reserved length symbols of the fixed code
        b.lensym(which, 0, 0)
    else:                     # reserved distance symbols 30, 31
        b.lensym(260)
        b.distsym(which, 0, 0)
    fill(b, s, rs, size)
    b.eob()
    return s


def case_I(rs, size, dist):
    s = dc.Stream()
    b = s.fixed(True)
    lits(b, rs, 10)
    b.match(20, dist)  # 10: the first byte of the output, legal; 11: one before it
    while size - len(s.raw) >= 300:
        lits(b, rs, int(rs.randint(0, 40)))
        b.match(int(rs.randint(3, 259)), int(rs.randint(1, 31)))
    fill(b, s, rs, size)
    b.eob()
    return s


def case_J(rs, size, over):
    s = dc.Stream()
    b = s.fixed(True)
    lits(b, rs, 500)
    end = size + over  # the last token is a 258-byte match that ends here
    while end - len(s.raw) - 258 >= 300:
        lits(b, rs, int(rs.randint(0, 40)))
        b.match(int(rs.randint(3, 259)), int(rs.randint(1, 400)))
    fill(b, s, rs, end - 258)
    b.match(258, 300)
    b.eob()
    return s


def cases_K(rs, size):
    """one zlib-made raw deflate body (a 512-byte window: no distance above 250) behind every zlib header"""
    raw = bytes(np.repeat(rs.randint(0, 5, size // 3 + 1).astype(np.uint8), 3)[:size])
    co = zlib.compressobj(6, zlib.DEFLATED, -9)
    body = co.compress(raw) + co.flush()
    for cmf in (0x08, 0x48, 0x78):
        for flevel in range(4):
            yield f"K cmf {cmf:#04x} flevel {flevel}", dc.zwrap(body, raw, cmf, flevel), True, None
    yield "K cmf 0x88", dc.zwrap(body, raw, 0x88), False, "HEADER"    # a 64 KiB window
    yield "K cmf 0x79", dc.zwrap(body, raw, 0x79), False, "HEADER"    # compression method 9
    yield "K fdict", dc.zwrap(body, raw, fdict=True), False, "HEADER"
    yield "K trailing bytes", dc.zwrap(body, raw) + bytes(range(16)), True, None


@functools.lru_cache(maxsize=None)
def crafted_cases():
    rs = np.random.RandomState(1951)
    out = []

    def add(name, geom, z, accepts, code=None):
        W, H = geom
        out.append(Case(name, W, H, dc.png_of(z, W, H, IDATS[len(out) % 3]), accepts, code))

    def add_stream(name, geom, build, accepts, code=None):
        s = build(geom[1] * (geom[0] + 1))
        add(name, geom, dc.zwrap(s.body(), s.raw), accepts, code)

    for geom, tag in ((SMALL, ""), (WIDE, " wide")):
        add_stream("A" + tag, geom, lambda n: case_A(rs, n), True)
    add_stream("A margin", SMALL, lambda n: case_A_margin(rs, n), True)
    add_stream("B", SMALL, lambda n: case_B(rs, n, False), True)
    for geom, tag in ((SMALL, ""), (WIDE, " wide")):
        add_stream("B2" + tag, geom, lambda n: case_B(rs, n, True), True)
    add_stream("C", SMALL, lambda n: case_C(rs, n), True)
    add_stream("D", SMALL, lambda n: case_D(rs, n, False), True)
    add_stream("D'", SMALL, lambda n: case_D(rs, n, True), False, "CODE")
    add_stream("E", SMALL, lambda n: case_E(rs, n, False), True)
    add_stream("E'", SMALL, lambda n: case_E(rs, n, True), False, "CODE")
    add_stream("F", SMALL, lambda n: case_F(rs, n), True)
    for which in (286, 287, 30, 31):
        add_stream(f"H {which}", SMALL, lambda n: case_H(rs, n, which), False, "CODE")
    add_stream("I", SMALL, lambda n: case_I(rs, n, 10), True)
    add_stream("I'", SMALL, lambda n: case_I(rs, n, 11), False, "DISTANCE")
    # zlib inflates J+ and J- to the end and their checksums are right: only the size is wrong
    add_stream("J+", SMALL, lambda n: case_J(rs, n, +1), False, "TOOMUCH")
    add_stream("J-", SMALL, lambda n: case_J(rs, n, -1), False, "TOOLITTLE")
    for name, z, accepts, code in cases_K(rs, SMALL[1] * (SMALL[0] + 1)):
        add(name, SMALL, z, accepts, code)
    return tuple(out)


def zlib_verdict(z, W, H):
    """eof reached, H * (W + 1) bytes, a filter type in front of every row -> (accepted, the raw bytes)"""
    try:
        d = zlib.decompressobj()
        raw = d.decompress(z)
    except zlib.error:
        return False, b""
    return d.eof and len(raw) == H * (W + 1) and all(raw[y * (W + 1)] <= 4 for y in range(H)), raw


def stream_of(png):
    """the concatenated IDAT data"""
    o, z = 8, b""
    while o + 12 <= len(png):
        ln, = struct.unpack(">I", png[o:o + 4])
        if png[o + 4:o + 8] == b"IDAT":
            z += png[o + 8:o + 8 + ln]
        o += 12 + ln
    return z


def pillow_pixels(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)))


def test_zlib_gives_the_stated_verdict_on_every_case():
    """no project code: the cases are what they claim to be"""
    names = [c.name for c in crafted_cases()]
    assert len(set(names)) == len(names)
    for c in crafted_cases():
        ok, raw = zlib_verdict(stream_of(c.png), c.W, c.H)
        assert ok == c.accepts, c.name
        assert all(v <= 4 for v in raw), c.name
    # J+ and J-: zlib inflates them to the end, checksum included; their size alone is wrong
    for c in crafted_cases():
        if c.name in ("J+", "J-"):
            d = zlib.decompressobj()
            raw = d.decompress(stream_of(c.png))
            assert d.eof and len(raw) == c.H * (c.W + 1) + (1 if c.name == "J+" else -1)


def test_host_decoder_agrees_with_zlib_and_pillow():
    from autobub3hs_amd import host
    for c in crafted_cases():
        got = host.imdecode(c.png)
        if c.accepts:
            assert got is not None, c.name
            assert np.array_equal(got, pillow_pixels(c.png)), c.name
        else:
            assert got is None, c.name
