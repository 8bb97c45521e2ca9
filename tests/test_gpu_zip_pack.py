"""abub_zip_pack_dev on the GPU against the restatement of the archive (tests/zipref.py): every byte of every item's range --
local header with the CRC, name, padding field, data -- is the reference's, every byte outside stays as it was, the CRCs are
zlib's; tile boundaries, every residue of the header's place, one to 300 items; and each descriptor error between intact
neighbours."""
import zlib

import numpy as np
import pytest
import torch

import zipref
from autobub3hs_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 65536  # ABUB_ZIP_PACK_TILE
FILL = 0xC3
SMALL = (0, 1, 15, 16, 17)
LENGTHS = SMALL + (T - 1, T, T + 1, 2 * T + 5, 300001)
NAME_LENGTHS = (1, 2, 3, 4, 17, 255)
E_DESC = 1


def test_the_tile_size_is_the_headers():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abub_hip.h")).read()
    assert f"#define ABUB_ZIP_PACK_TILE {T}\n" in hdr


def build(lengths, seed=0, same_src=()):
    """Files of the given lengths at multiples of 16 of a buffer, names, and items laid out in a segment so that the place of
    item k's header is k modulo 16 (gaps in between belong to nobody).  same_src: pairs (k, j): item k reads item j's file.
    -> (buf, names, items rows, [(dst, name, data)], seg_bytes)"""
    rs = np.random.RandomState(seed)
    files, srcs, at = [], [], 0
    for n in lengths:
        files.append(rs.randint(0, 256, n).astype(np.uint8))
        srcs.append(at)
        at += (n + 15) & ~15
    for k, j in same_src:
        files[k], srcs[k] = files[j], srcs[j]
    buf = rs.randint(0, 256, at + 16).astype(np.uint8)
    for s, f in zip(srcs, files):
        buf[s:s + len(f)] = f
    names, rows, placed, off = bytearray(), [], [], 7
    for k, f in enumerate(files):
        m = NAME_LENGTHS[(k + k // len(NAME_LENGTHS)) % len(NAME_LENGTHS)]
        name = bytes(rs.randint(97, 123, m).astype(np.uint8))
        off += (k - off) % 16 + 16 * int(rs.randint(0, 3))  # the header's place: residue k mod 16, behind a gap
        xl = zipref.extra_len(off, m, len(f))
        rows.append((srcs[k], off, len(f), len(names), m, xl))
        placed.append((off, name, f.tobytes()))
        names += name
        off += 30 + m + xl + len(f)
    return buf, np.frombuffer(bytes(names) + b"\0", np.uint8).copy(), rows, placed, off + 9


def expected(placed, seg_bytes, skip=()):
    want = np.full(seg_bytes, FILL, np.uint8)
    for k, (dst, name, data) in enumerate(placed):
        if k not in skip:
            e = zipref.local_entry(dst, name, data)
            want[dst:dst + len(e)] = np.frombuffer(e, np.uint8)
    return want


def run(buf, names, rows, seg_bytes, seg=None, names_bytes=None, buf_bytes=None):
    d_buf, d_names = torch.from_numpy(buf).to(DEV), torch.from_numpy(names).to(DEV)
    if seg is None:
        seg = torch.full((seg_bytes + 64,), FILL, dtype=torch.uint8, device=DEV)
    crc, status = hip.zip_pack(d_buf, rows, d_names, seg, seg_bytes=seg_bytes, names_bytes=names_bytes, buf_bytes=buf_bytes)
    torch.cuda.synchronize()
    return crc.numpy(), status.numpy(), seg


def check(placed, crc, status, seg, seg_bytes, skip=()):
    got = seg.cpu().numpy()
    assert (got[seg_bytes:] == FILL).all(), "written behind seg_bytes"
    want = expected(placed, seg_bytes, skip)
    bad = np.flatnonzero(got[:seg_bytes] != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}"
    for k, (_, _, data) in enumerate(placed):
        if k in skip:
            assert status[k] == E_DESC and crc[k] == 0, k
        else:
            assert status[k] == 0 and crc[k] == zlib.crc32(data), (k, len(data))


def test_every_length_name_length_and_residue():
    lengths = LENGTHS * 4  # 40 items: every length meets several residues of the header's place and several name lengths
    buf, names, rows, placed, seg_bytes = build(lengths, seed=1)
    assert {r[1] % 16 for r in rows} == set(range(16)) and {r[4] for r in rows} == set(NAME_LENGTHS)
    assert {-(r[1] + 30 + r[4]) % 16 for r in rows if r[2]} == set(range(16))  # every padding case
    assert {r[5] for r in rows} == {0, 17, 18, 19} | set(range(4, 16))
    crc, status, seg = run(buf, names, rows, seg_bytes)
    check(placed, crc, status, seg, seg_bytes)
    # once more on the buffers as they are: the same bytes, the same CRCs
    before = seg.clone()
    crc2, status2, seg = run(buf, names, rows, seg_bytes, seg=seg)
    assert torch.equal(seg, before) and np.array_equal(crc, crc2) and np.array_equal(status, status2)


@pytest.mark.parametrize("nitems", [1, 2, 255, 256, 257, 300])
def test_item_counts(nitems):
    big = {1: (300001,), 2: (2 * T + 5, T)}.get(nitems, (T + 1, 300001, T - 1))
    lengths = [big[k // 97 % len(big)] if k % 97 == 0 else SMALL[k % len(SMALL)] + 16 * (k % 7) for k in range(nitems)]
    buf, names, rows, placed, seg_bytes = build(lengths, seed=nitems)
    crc, status, seg = run(buf, names, rows, seg_bytes)
    check(placed, crc, status, seg, seg_bytes)


def test_two_items_may_share_a_source():
    buf, names, rows, placed, seg_bytes = build((T + 1, 17, 40, 0, T + 1), seed=5, same_src=((4, 0), (2, 1)))
    assert rows[4][0] == rows[0][0]
    crc, status, seg = run(buf, names, rows, seg_bytes)
    check(placed, crc, status, seg, seg_bytes)
    assert crc[4] == crc[0]


def test_a_file_of_many_tiles_and_a_short_grid():
    """one file of 70 tiles (a workgroup takes more than one tile: at most 64 are in flight per item)"""
    buf, names, rows, placed, seg_bytes = build((70 * T - 3, 16), seed=6)
    crc, status, seg = run(buf, names, rows, seg_bytes)
    check(placed, crc, status, seg, seg_bytes)


def refusals(rows, buf_bytes, names_bytes, seg_bytes):
    """(what, item, its row with one descriptor error)"""
    def change(k, **kw):
        cols = ("src", "dst", "len", "name", "name_len", "extra_len")
        r = dict(zip(cols, rows[k]), **kw)
        return tuple(r[c] for c in cols)
    src, dst, ln, name, nl, xl = rows[3]
    return [("src not a multiple of 16", 3, change(3, src=src + 8)),
            ("src behind the buffer", 3, change(3, src=(buf_bytes + 32) & ~15)),
            ("the file leaves the buffer", 3, change(3, src=(buf_bytes - ln + 16) & ~15)),
            ("a length of 2^32 - 1", 3, change(3, len=0xFFFFFFFF)),
            ("name behind the names", 3, change(3, name=names_bytes + 1)),
            ("the name leaves the names", 3, change(3, name=names_bytes - nl + 1)),
            ("a padding field of 1 byte", 5, change(5, extra_len=1)),
            ("a padding field of 3 bytes", 5, change(5, extra_len=3)),
            ("data not at a multiple of 16", 3, change(3, dst=dst + 1)),
            ("data not at a multiple of 16, by the padding", 3, change(3, extra_len=xl + 4)),
            ("dst behind the segment", 3, change(3, dst=seg_bytes + 16)),
            ("the entry leaves the segment", 3, change(3, dst=((seg_bytes - ln - 30 - nl - xl) & ~15) + 16 + dst % 16))]


def test_descriptor_errors_between_intact_neighbours():
    lengths = (40, 17, 300, 5000, 16, 0, 33, T + 1)
    buf, names, rows, placed, seg_bytes = build(lengths, seed=9)
    names_bytes, buf_bytes = len(names) - 1, len(buf) - 16
    cases = refusals(rows, buf_bytes, names_bytes, seg_bytes)
    assert len(cases) == 12
    for what, k, row in cases:
        bad = list(rows)
        bad[k] = row
        crc, status, seg = run(buf, names, bad, seg_bytes, names_bytes=names_bytes, buf_bytes=buf_bytes)
        assert status[k] == E_DESC, what
        check(placed, crc, status, seg, seg_bytes, skip=(k,))
    # several at once, first and last item among them
    bad = list(rows)
    for _, k, row in (cases[0], cases[6]):
        bad[k] = row
    bad[0] = (rows[0][0] + 4,) + rows[0][1:]
    bad[7] = rows[7][:2] + (0xFFFFFFFF,) + rows[7][3:]
    crc, status, seg = run(buf, names, bad, seg_bytes, names_bytes=names_bytes, buf_bytes=buf_bytes)
    check(placed, crc, status, seg, seg_bytes, skip=(0, 3, 5, 7))
