"""abub_unzip_dev on the GPU: raw deflate streams of zip entries -> their files, bit for bit what zlib.decompress(..., -15)
gives, with the status include/abub_hip.h documents for every refusal.  One batch holds every accepted case (output lengths
at the edges of the 16-byte flush, the 512-byte pass and the ring; zeros, a short period, random bytes, a PNG and a BMP file;
levels 0, 1, 6, 9 and Z_FIXED; hand-written streams); a second one every refusal between two good entries.  Canaries lie
behind every entry and between entries; the bytes behind a stream in `comp` are 0xFF.  The good batch once more through the
one-wave route (ABUB_PNG_WAVES=1) in a fresh process; the CRC kernel on its own against zlib.crc32."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import zipcraft as zc  # noqa: E402

pytestmark = pytest.mark.gpu


def run_batch(batch):
    import torch

    from autobub3hs_amd import hip
    comp = torch.frombuffer(bytearray(batch.comp), dtype=torch.uint8).cuda()
    out = torch.full((batch.out_bytes,), zc.CANARY_OUT, dtype=torch.uint8, device="cuda")
    st = hip.unzip(comp, batch.rows, out)
    torch.cuda.synchronize()
    return st.cpu().numpy().tolist(), out.cpu().numpy()


def refusal_batch():
    rs = np.random.RandomState(4)
    good = [zc.Case(f"good-{k}", zc.deflate_raw(d, 6), d) for k, d in
            enumerate(bytes(rs.randint(0, 6, 700 + 37 * k).astype(np.uint8)) for k in range(len(zc.refused_cases()) + 1))]
    cases = [good[0]]
    for k, c in enumerate(zc.refused_cases()):
        cases += [c, good[k + 1]]
    return zc.Batch(cases)


def summary(st, out):
    return {"status": st, "out": hashlib.sha256(out.tobytes()).hexdigest()}


@pytest.fixture(scope="module")
def good():
    b = zc.Batch(zc.good_cases())
    return (b,) + run_batch(b)


@pytest.fixture(scope="module")
def refused():
    b = refusal_batch()
    return (b,) + run_batch(b)


def check(batch, st, out):
    codes = zc.status_codes()
    want_st = batch.want_status(codes)
    for c, got, want in zip(batch.cases, st, want_st):
        assert got == want, (c.name, got, want)
    want, known = batch.expected()
    pos = 0
    for c in batch.cases:  # (per entry first: a failure names the case)
        if c.code is None:
            assert out[pos:pos + c.ulen].tobytes() == zlib.decompress(c.z, -15) == c.raw, c.name
        n = zc.align16(c.ulen)
        assert (out[pos + (c.ulen if c.code is None else n):pos + n + zc.GAP] == zc.CANARY_OUT).all(), c.name
        pos += n + zc.GAP
    assert np.array_equal(out[known], want[known])


def test_every_accepted_stream_bit_for_bit(good):
    batch, st, out = good
    assert len(batch.cases) > 200 and {c.ulen for c in batch.cases} >= set(zc.LENGTHS)
    assert all(c.code is None for c in batch.cases)
    check(batch, st, out)


def test_refusals_between_good_entries(refused):
    """every refusal has the documented status, its neighbours are intact, a descriptor refusal writes nothing"""
    batch, st, out = refused
    assert {c.code for c in batch.cases} >= {None, "TRUNCATED", "BLOCKTYPE", "STORED", "CODES", "DISTANCE", "TOOMUCH", "TOOLITTLE",
                                             "CRC", "DESC"}
    assert {c.desc for c in batch.cases} == {None, "off", "dst", "clen"}
    check(batch, st, out)


def test_one_wave_route_gives_the_same(good, refused):
    """ABUB_PNG_WAVES=1 (k_zip_inflate<false>: one wave parses and writes) is read once per process: one fresh child runs the
    same batches and reports statuses and a digest of the output"""
    env = dict(os.environ, ABUB_PNG_WAVES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["good"] == summary(*good[1:])
    # (inside a refused entry's own range the two routes may have got differently far)
    assert got["refused"]["status"] == refused[1]


def test_crc_kernel_alone():
    """abub_crc32_dev == zlib.crc32 at every length of the list, at the lengths around the 256 pieces of 64 bytes and more, and
    on a real-size file; a descriptor outside the buffer is refused and its word left alone"""
    import torch

    from autobub3hs_amd import hip
    rs = np.random.RandomState(9)
    lens = list(zc.LENGTHS) + [63, 64, 65, 16383, 16384, 16385, 16400, 1280 * 1024 + 1078]
    buf, rows = bytearray(), []
    for n in lens:
        rows.append([0, 0, n, 0, len(buf)])
        buf += bytes(rs.randint(0, 256, n).astype(np.uint8)) + bytes(zc.align16(n) - n)
    want = [zlib.crc32(bytes(buf[r[4]:r[4] + r[2]])) & 0xFFFFFFFF for r in rows]
    rows += [[0, 0, 100, 0, 8], [0, 0, 100, 0, len(buf)], [0, 0, 17, 0, len(buf) - 16], [0, 0, 1 << 28, 0, 0]]
    crc, st = hip.crc32(torch.frombuffer(buf, dtype=torch.uint8).cuda(), rows)
    assert st.tolist() == [0] * len(lens) + [zc.status_codes()["DESC"]] * 4
    assert crc.tolist()[:len(lens)] == want
    assert crc.tolist()[len(lens):] == [0] * 4


if __name__ == "__main__":
    g = run_batch(zc.Batch(zc.good_cases()))
    r = run_batch(refusal_batch())
    print(json.dumps({"good": summary(*g), "refused": summary(*r)}))
