"""The canonical Huffman-only PNG ("Unpacking a run") restated in numpy, from the format's rules and
not from the C++: the tests compare cv::pngHuffEncode and abub_png_encode_dev with it byte for byte."""
import struct
import zlib

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS_MAX = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 7
CONTAINER_BYTES = 8 + 25 + 12 + 2 + 4 + 12


def file_bound(W, H):
    """15 bits per symbol for H * (W + 1) + 1 symbols, the longest header, the container; 0 from 2^32 on or for a size
    outside [1, 65535]"""
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        return 0
    v = CONTAINER_BYTES + (HEADER_BITS_MAX + 15 * (H * (W + 1) + 1) + 7) // 8
    return 0 if v >= 1 << 32 else v


def tree_depths(counts):
    """Rules 1 and 2: the used symbols ascending by (count, symbol) and the depth of each one's leaf in the two-queue tree"""
    used = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(used)
    assert n >= 2
    weight = [c for c, _ in used]
    parent = [0] * (2 * n - 1)
    li, ii = 0, n  # heads of the leaf queue and of the queue of internal nodes
    for new in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= new or weight[li] <= weight[ii]):  # (on equal weight the leaf goes first)
                parent[li] = new
                w += weight[li]
                li += 1
            else:
                parent[ii] = new
                w += weight[ii]
                ii += 1
        weight.append(w)
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    return used, depth[:n]


def unlimited_depth(counts):
    return max(tree_depths(counts)[1])


def code_lengths(counts, limit):
    """Rules 1 to 6 -> one length per symbol"""
    used, depth = tree_depths(counts)
    per = [0] * (limit + 1)
    for d in depth:
        per[min(d, limit)] += 1
    while sum(per[d] << (limit - d) for d in range(1, limit + 1)) > 1 << limit:
        per[limit] -= 1
        d = max(k for k in range(1, limit) if per[k])
        per[d] -= 1
        per[d + 1] += 2
    lengths = [0] * len(counts)
    order = sorted(used, key=lambda cs: (-cs[0], cs[1]))
    at = 0
    for d in range(1, limit + 1):
        for _ in range(per[d]):
            lengths[order[at][1]] = d
            at += 1
    assert at == len(order)
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2"""
    count = [0] * 17
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, v in enumerate(lengths):
        if v:
            codes[s] = nxt[v]
            nxt[v] += 1
    return codes


def filtered(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    f = np.empty((H, W + 1), np.uint8)
    f[:, 0] = 1
    f[:, 1] = img[:, 0]
    f[:, 2:] = img[:, 1:] - img[:, :-1]
    return f


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):  # the n low bits of v, least significant first
        self.acc |= int(v) << self.n
        self.n += n

    def code(self, c, n):  # a Huffman code, most significant bit first
        self.put(int(format(c, "0%db" % n)[::-1], 2), n)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def lit_counts(img):
    counts = np.bincount(filtered(img).ravel(), minlength=257).astype(np.int64)
    counts[256] = 1
    return counts


def encode(img):
    f = filtered(img)
    H, W = np.asarray(img).shape
    counts = lit_counts(img)
    ll = code_lengths(counts, 15)
    seq = ll + [0]  # the 257 literal/length lengths, then the one distance length
    cl = code_lengths(np.bincount(seq, minlength=19), 7)
    assert not any(cl[16:])
    clc = canonical_codes(cl)
    b = _Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(15, 4)
    for s in CL_ORDER:
        b.put(cl[s], 3)
    for v in seq:
        b.code(clc[v], cl[v])
    codes = canonical_codes(ll)
    rev = np.array([int(format(c, "0%db" % n)[::-1], 2) if n else 0 for c, n in zip(codes, ll)], dtype=object)
    lens = np.array(ll)
    syms = f.ravel()
    # (vectorised: bit positions by a cumulative sum, then one big integer)
    n = lens[syms].astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(n)])
    nbits = int(pos[-1])
    bits = np.zeros(nbits + 16, np.uint8)
    vals = np.array([int(v) for v in rev], np.int64)[syms]
    for k in range(15):
        m = n > k
        bits[pos[:-1][m] + k] = (vals[m] >> k) & 1
    body = np.packbits(bits, bitorder="little")
    b.put(int.from_bytes(body.tobytes(), "little"), nbits)
    b.code(codes[256], ll[256])
    z = b"\x78\x01" + b.acc.to_bytes((b.n + 7) // 8, "little") + struct.pack(">I", zlib.adler32(f.tobytes()) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", z)
            + _chunk(b"IEND", b""))


def chunks(png):
    """[(type, data, stored crc)] of a PNG file"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        out.append((png[at + 4:at + 8], png[at + 8:at + 8 + n], struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(png)
    return out


def header_lengths(z):
    """The code lengths a file's deflate header states: (the 19 of the code-length code, the 258 it sends)"""
    v = int.from_bytes(z[2:2 + 260], "little")
    assert v & 7 == 5 and (v >> 3) & 0x3FFF == 15 << 10
    at = 17
    cl = [0] * 19
    for s in CL_ORDER:
        cl[s] = (v >> at) & 7
        at += 3
    codes = canonical_codes(cl)
    table = {(format(c, "0%db" % n)): s for s, (c, n) in enumerate(zip(codes, cl)) if n}
    sent = []
    while len(sent) < 258:
        key = ""
        while key not in table:
            key += str((v >> at) & 1)
            at += 1
            assert len(key) <= 7
        assert table[key] < 16
        sent.append(table[key])
    return cl, sent


def unfilter(raw, W, H):
    f = np.frombuffer(raw, np.uint8).reshape(H, W + 1)
    assert (f[:, 0] == 1).all()
    return np.cumsum(f[:, 1:], axis=1, dtype=np.uint64).astype(np.uint8)


# ---- the shapes the tests share: the smallest at which each mechanism of an encoder can fail ---------------------------------
def from_residuals(res, W, H):
    """the image whose Sub residuals (first pixel included) are `res`"""
    return np.cumsum(np.asarray(res, np.uint8).reshape(H, W), axis=1, dtype=np.uint64).astype(np.uint8)


def limit15_case():
    """128 x 2048: residual values 2 .. 19 with counts 2^0 .. 2^17, padded with 19, shuffled: the unlimited tree is 18 deep"""
    vals = np.concatenate([np.full(1 << k, 2 + k, np.uint8) for k in range(18)])
    res = np.full(128 * 2048, 19, np.uint8)
    res[:len(vals)] = vals
    np.random.RandomState(15).shuffle(res)
    return from_residuals(res, 128, 2048)


def limit7_case():
    """88 x 23: 2048 symbols whose counts are powers of two, chosen so that the code has 1, 1, 3, 5, 8, 13, 21 and 2 codes
    of the lengths 1, 2, 5, 6, 8, 9, 10 and 11 (Kraft sum 1).  The histogram of the 258 lengths is then (204, 1, 1, 3, 5,
    8, 13, 21, 2): Fibonacci-like, and its unlimited tree is 8 deep, one more than the code-length code may be."""
    W, H = 88, 23
    groups = [(1024, 1), (512, 1), (64, 3), (32, 5), (8, 8), (4, 13), (2, 21), (1, 1)]  # (count, symbols); EOB is the other 1
    values = [0, 2, 3, 4, 5, 1] + list(range(6, 60))  # symbol 1 (the filter byte, H of its 32 are not residuals) has count 32
    res, at = [], 0
    for count, n in groups:
        for v in values[at:at + n]:
            res += [v] * (count - H if v == 1 else count)
        at += n
    res = np.array(res, np.uint8)
    assert len(res) == W * H
    np.random.RandomState(7).shuffle(res)
    return from_residuals(res, W, H)


def small_cases(sample, synth_frame):
    """name -> image, without the two limit cases and the full sample frame"""
    def crop(img, W, H, x0=0, y0=0):
        img = img[y0:, x0:]
        reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
        return np.ascontiguousarray(np.tile(img, reps)[:H, :W])

    rs = np.random.RandomState(2024)
    out = {
        "w1_ones": np.full((40, 1), 1, np.uint8),  # lengths {1, 1}: rows of 2 bits, four to a byte
        "w1_sevens": np.full((40, 1), 7, np.uint8),  # lengths {1, 2, 2}: rows of 3 or 4 bits
        "w2_ones": np.full((33, 2), 1, np.uint8),  # lengths {1, 2, 2}
        "3x5": rs.randint(0, 256, (5, 3)).astype(np.uint8),
        "7x65": rs.randint(0, 256, (65, 7)).astype(np.uint8),
        "1280x8": crop(synth_frame, 1280, 8, 0, 40),
        "1680x6": crop(synth_frame, 1680, 6, 5, 77),
        "160x96": crop(sample, 160, 96, 700, 400),
    }
    for W in (63, 64, 65, 127, 128, 129):
        out[f"{W}x3"] = crop(synth_frame if W & 1 else sample, W, 3, 11, 50) if W != 64 else rs.randint(0, 256, (3, 64)).astype(np.uint8)
    return out
