"""Resident frames compared on the GPU: abub_frames_compare_dev against numpy (count of a != b, argmax, abs().max() on
int16) at every size and pair of alignments at which it takes another path, with differences on every tile, wave and lane
seam; what a launch is made of (many pairs, repeated frames, one buffer on both sides, a reused results buffer); its range
status; one launch at the workload's size; and the device route of abub3hs --verify-repack / Run.verify(device=0) against
the host route, on every tampering of tests/test_verify_repack.py."""
import os
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

from autobub3hs_amd import hip, host, synth
from test_abf_format import make_run_dir
from test_verify_repack import (CASES, ENV, EXE, NCAMS, RUN_ID, TOTAL, VERDICTS, World, base, check, fresh, rewrite,  # noqa: F401
                                summary_and_findings, tamper_25)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GARBAGE = 0x5A5A5A5A
SIZES = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 4096, 4099, 16385, 65536 + 48, 3 * 65536 + 7, 96 * 64, 1280 * 9]
MODS = (0, 1, 4, 15)
E_RANGE = 1
NEUTRAL = [0, 0xFFFFFFFF, 0]


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def reference(a, b):
    """rows of (status, ndiff, first, max_abs) for frames a[i], b[i]"""
    ne = a != b
    n = ne.sum(axis=1)
    first = np.where(n > 0, ne.argmax(axis=1), 0xFFFFFFFF)
    mx = np.abs(a.astype(np.int16) - b.astype(np.int16)).max(axis=1)
    return np.stack([np.zeros_like(n), n, first, mx], axis=1).astype(np.int64)


def contents(n, rs):
    """the pairs of one shape -> (a [m, n], b [m, n]); pair 0 is identical, the last two differ everywhere"""
    a0 = rs.randint(0, 256, n).astype(np.uint8)
    seams = {0, n - 1}
    k = 1
    while k - 1 < n:
        seams.update(p for p in (k - 1, k, k + 1) if p < n)
        k *= 2
    changes = [lambda b: None]  # identical
    for p in sorted(seams):  # one differing byte, on every plausible tile, wave and lane seam
        changes.append(lambda b, p=p: b.__setitem__(p, b[p] ^ 0x10))
    if n >= 2:  # two differing bytes: `first` is the lower one
        lo, hi = sorted(int(v) for v in rs.choice(n, 2, replace=False))
        changes.append(lambda b: (b.__setitem__(lo, (int(b[lo]) + 7) & 0xFF), b.__setitem__(hi, (int(b[hi]) + 99) & 0xFF)))
    hit = np.nonzero(rs.rand(n) < 0.01)[0]  # a random 1 %
    new = rs.randint(0, 256, hit.size).astype(np.uint8)
    changes.append(lambda b: b.__setitem__(hit, new))
    a = np.stack([np.roll(a0, 3 * i) for i in range(len(changes))])  # (each pair has a source of its own)
    b = a.copy()
    for row, change in zip(b, changes):
        change(row)
    a_all = np.zeros(n, np.uint8)  # all bytes differ, by 255
    b_all = np.full(n, 255, np.uint8)
    b_one = np.where(a0 == 255, 254, a0.astype(np.int16) + 1).astype(np.uint8)  # |a - b| = 1 everywhere
    return np.concatenate([a, a_all[None], a0[None]]), np.concatenate([b, b_all[None], b_one[None]])


def scatter(frames, mod, rs):
    """the frames at scattered offsets congruent to `mod` mod 16, not in order, in a buffer of other bytes -> (buffer, offsets)"""
    m, n = frames.shape
    offs = np.zeros(m, np.int64)
    at = 16
    for slot in rs.permutation(m):
        at = ((at + int(rs.randint(0, 70)) + 15) & ~15) + mod
        offs[slot] = at
        at += n
    buf = (np.arange(at + 21, dtype=np.uint32) * 37 >> 3).astype(np.uint8)
    for o, f in zip(offs, frames):
        buf[o:o + n] = f
    return buf, offs


def launch(A, B, pairs, n, **kw):
    """one call with the results between canaries and full of garbage -> the records; the canaries must be whole"""
    m = len(pairs)
    full = torch.full((8 + 4 * m + 8,), GARBAGE, dtype=torch.int32, device=DEV)
    got = hip.frames_compare(A, B, pairs, n, results=full[8:8 + 4 * m], **kw)
    whole = full.cpu().numpy()
    assert (whole[:8] == GARBAGE).all() and (whole[8 + 4 * m:] == GARBAGE).all(), "a canary was written"
    assert np.array_equal(whole[8:8 + 4 * m].view(np.uint32).astype(np.int64).reshape(m, 4), got)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_numpy(n):
    rs = np.random.RandomState(n % 9973)
    a, b = contents(n, rs)
    want = reference(a, b)
    assert want[0, 1] == 0 and list(want[-2]) == [0, n, 0, 255] and list(want[-1]) == [0, n, 0, 1]
    assert (want[1:len(want) - 3, 1] >= 1).all() and (want[1:len(want) - 3, 1] <= 2).all()  # (the seams, and the two bytes)
    for ma in MODS:
        bufa, offa = scatter(a, ma, rs)
        A = torch.from_numpy(bufa).to(DEV)
        for mb in MODS:
            bufb, offb = scatter(b, mb, rs)
            B = torch.from_numpy(bufb).to(DEV)
            assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
            got = launch(A, B, np.stack([offa, offb], axis=1), n)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (n, ma, mb, bad[:5], got[bad[:5]], want[bad[:5]])


def test_a_launch_is_the_sum_of_its_pairs():
    n, nf = 4099, 40
    rs = np.random.RandomState(5)
    frames = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    frames[1::2] = frames[0::2]  # neighbours are equal, or differ in a few bytes only
    for i in range(1, nf, 4):
        frames[i, rs.choice(n, 1 + i, replace=False)] ^= 0x81
    # one buffer for both sides, every frame in it four times: once at each alignment
    pieces, offs, at = [], [], 0
    for mod in MODS:
        buf, o = scatter(frames, mod, rs)
        pieces.append(buf)
        offs.append(o + at)
        at += len(buf) + (-len(buf)) % 16
        pieces.append(np.zeros((-len(buf)) % 16, np.uint8))
    offs = np.concatenate(offs)
    T = torch.from_numpy(np.concatenate(pieces)).to(DEV)
    assert T.data_ptr() % 16 == 0
    ia, ib = rs.randint(0, len(offs), 300), rs.randint(0, len(offs), 300)
    ib[:20] = ia[:20]  # a frame against itself
    ib[20:40] = ia[20:40] ^ 1  # ... and against its neighbour
    pairs = np.stack([offs[ia], offs[ib]], axis=1)
    want = reference(frames[ia % nf], frames[ib % nf])
    assert (want[:20, 1] == 0).all() and (want[:, 1] > 0).sum() > 200 and (want[20:40, 1] < 50).all()
    assert len({(int(p[0]) % 16, int(p[1]) % 16) for p in pairs}) == 16
    got = launch(T, T, pairs, n)
    assert np.array_equal(got, want)
    one_by_one = np.concatenate([launch(T, T, pairs[i:i + 1], n) for i in range(len(pairs))])
    assert np.array_equal(one_by_one, got)
    # a reused results buffer: what the launch before left there does not show
    res = torch.full((4 * 300,), GARBAGE, dtype=torch.int32, device=DEV)
    first = hip.frames_compare(T, T, pairs, n, results=res)
    again = hip.frames_compare(T, T, pairs[::-1].copy(), n, results=res)
    assert np.array_equal(first, want) and np.array_equal(again, want[::-1])
    assert np.array_equal(hip.frames_compare(T, T, pairs, n, results=res), want)


def test_range_status():
    """the offsets stay inside the real tensors: only the sizes the kernel is told are small"""
    n, nf = 1000, 10
    rs = np.random.RandomState(11)
    a = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    b = a.copy()
    for i in range(nf):
        b[i, rs.choice(n, i + 1, replace=False)] ^= 0xFF
    A, B = torch.from_numpy(a.reshape(-1)).to(DEV), torch.from_numpy(b.reshape(-1)).to(DEV)
    pairs = np.stack([np.arange(nf) * n, np.arange(nf) * n], axis=1).astype(np.int64)
    want = reference(a, b)
    assert np.array_equal(launch(A, B, pairs, n), want)
    for kw, out in ((dict(a_bytes=7 * n - 1), [6, 7, 8, 9]), (dict(b_bytes=3 * n + 999), [3, 4, 5, 6, 7, 8, 9]),
                    (dict(a_bytes=9 * n, b_bytes=10 * n - 1), [9]), (dict(a_bytes=n - 1), list(range(nf))),
                    (dict(a_bytes=10 * n, b_bytes=10 * n), [])):
        got = launch(A, B, pairs[::-1].copy(), n, **kw)[::-1]
        for i in range(nf):
            if i in out:
                assert list(got[i]) == [E_RANGE] + NEUTRAL, (kw, i, got[i])
            else:
                assert np.array_equal(got[i], want[i]), (kw, i, got[i], want[i])


def test_one_launch_at_the_workload_size():
    W, H = 1280, 1024
    spec = synth.random_spec(W, H, 12, 3, 0)
    fr = np.ascontiguousarray(np.asarray(synth.render_event(W, H, spec, 3, 0))[4:12]).reshape(8, -1)
    other = fr.copy()
    rs = np.random.RandomState(3)
    for i in range(0, 8, 2):  # half of them with one pixel changed
        p = int(rs.randint(W * H)) if i else W * H - 1
        other[i, p] = (int(other[i, p]) + 1 + i) & 0xFF
    A, B = torch.from_numpy(fr.reshape(-1)).to(DEV), torch.from_numpy(other.reshape(-1)).to(DEV)
    pairs = np.stack([np.arange(8) * W * H] * 2, axis=1).astype(np.int64)
    assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0 and (W * H) % 16 == 0
    want = reference(fr, other)
    assert list(want[:, 1]) == [1, 0] * 4 and want[0, 2] == W * H - 1
    assert np.array_equal(launch(A, B, pairs, W * H), want)


# ---- the device route against the host route ----------------------------------------------------------------------------------
SHARED = VERDICTS + ("rc", "events", "frames", "event_file", "findings")


def both_routes(w, kind="raw", kernel_frames=None):
    """Run.verify() and Run.verify(device=0) of a world -> the host route's answer, after checking the device route's is it"""
    cpu, gpu = w.verify(kind), w.verify(kind, device=0)
    for k in SHARED:
        assert cpu[k] == gpu[k], (kind, k, cpu[k], gpu[k])
    assert cpu["device"] == -1 and cpu["frames_kernel"] == 0
    assert gpu["frames_kernel"] + gpu["frames_host_route"] == gpu["frames"]
    if kernel_frames is not None:
        assert gpu["device"] == 0 and gpu["frames_kernel"] == kernel_frames, gpu
    return cpu, gpu


def test_clean_run_on_the_device_route(base):
    for kind in ("raw", "stored", "deflated"):
        cpu, gpu = both_routes(base, kind, kernel_frames=TOTAL)
        check(gpu, [], event_file="same" if kind == "raw" else "not compared")
        assert gpu["src_gpu_png_decoded"] == TOTAL and gpu["other_gpu_unpacked"] == TOTAL and gpu["batches"] == 1
    a, b = host.Run("raw", base.src + "/", "Images"), host.Run("raw", base.src + "/", "Images")
    try:  # the source against itself: PNG on both sides
        res = a.verify(b, nthreads=4, ncams=NCAMS, device=0)
    finally:
        a.close()
        b.close()
    assert res["rc"] == 0 and res["same_not_packed"] == TOTAL == res["frames_kernel"] == res["other_gpu_png_decoded"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_agree_on_every_tampering(base, tmp_path, name):
    w = fresh(base, tmp_path)
    expected = CASES[name](w)
    for kind in ("raw", "stored", "deflated"):
        cpu, gpu = both_routes(w, kind)
        assert gpu["device"] == 0 and gpu["frames_kernel"] >= TOTAL - 1
        if kind == "raw":
            check(gpu, expected, copied=1 if name == "source_does_not_decode" else 0)
            continue
        # an archive has no event file of its own to compare the copy's with: that finding goes, the others stay
        rest = [f for f in expected if not f["verdict"].startswith("event_file_")]
        check(gpu, rest, copied=1 if name == "source_does_not_decode" else 0, event_file="not compared")


def test_routes_agree_on_25_tamperings_in_several_batches(base, tmp_path, monkeypatch):
    w = fresh(base, tmp_path)
    expected = tamper_25(w)
    monkeypatch.setenv("ABUB_VERIFY_BATCH", "7")
    cpu, gpu = both_routes(w)
    check(gpu, expected)
    assert gpu["batches"] == (TOTAL + 6) // 7
    monkeypatch.delenv("ABUB_VERIFY_BATCH")
    cpu, gpu = both_routes(w, "deflated")
    assert gpu["batches"] == 1 and gpu["findings"] == expected


def test_routes_agree_on_frames_the_decoders_do_not_take(base, tmp_path):
    w = fresh(base, tmp_path)
    k16, kodd, kempty = (0, 0, "cam0_image31.png"), (1, 0, "cam0_image35.png"), (2, 1, "cam1_image40.png")
    Image.fromarray(w.frames[k16].astype(np.uint16) * 257).save(w.path(w.src, k16[0], k16[2]))  # a 16-bit PNG
    Image.fromarray(np.ascontiguousarray(w.frames[kodd][:31, :51])).save(w.path(w.src, kodd[0], kodd[2]))  # an odd size
    rewrite(w.path(w.src, kempty[0], kempty[2]), lambda d: b"")
    st = w.repack()
    assert st["copied"] == 1 and st["packed"] == TOTAL - 1
    for kind in ("raw", "deflated"):
        cpu, gpu = both_routes(w, kind)
        check(gpu, [], copied=1, event_file="same" if kind == "raw" else "not compared")
        # the 16-bit frame is decoded by a host thread and compared by the kernel; the other two take the host route
        assert gpu["frames_kernel"] == TOTAL - 2 and gpu["frames_host_route"] == 2 and gpu["src_host_decoded"] == 1, gpu
    # ... and with the copy of each of them spoilt
    rewrite(w.path(w.out, k16[0], k16[2]), lambda d: host.abf_encode(255 - w.frames[k16]))
    rewrite(w.path(w.out, kodd[0], kodd[2]), lambda d: d[:-3])
    rewrite(w.path(w.out, kempty[0], kempty[2]), lambda d: b"\0")
    cpu, gpu = both_routes(w)
    assert [f["verdict"] for f in gpu["findings"]] == ["differ", "undecodable", "undecodable"] and gpu["rc"] == 1
    assert gpu["findings"][0]["ndiff"] == int((w.frames[k16] != 255 - w.frames[k16]).sum())


def test_a_width_outside_the_gate_takes_the_host_route_whole(tmp_path):
    rd, frames = make_run_dir(str(tmp_path / "data"), W=98, H=24, F=3, nev=2, ncams=NCAMS)
    w = World(str(tmp_path), rd, str(tmp_path / "packed" / RUN_ID), frames)
    w.repack()
    rewrite(w.path(w.out, 1, "cam0_image31.png"), lambda d: d[:-1])
    cpu, gpu = both_routes(w)
    assert gpu["device"] == -1 and gpu["frames_kernel"] == 0 and gpu["frames_host_route"] == 12 and gpu["batches"] == 0
    assert gpu["undecodable"] == 1 and gpu["same"] == 11 and gpu["rc"] == 1


def cli(*args):
    return subprocess.run([EXE] + list(args), env=ENV, capture_output=True, text=True)


def test_cli_on_the_device_route(base, tmp_path):
    data, x = os.path.dirname(base.src), str(tmp_path / "X")
    r = cli("-d", data, "-r", RUN_ID, "--repack", x, "--repack-gpu", "--verify-repack", x, "--verify-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines] == ["repack", "repack-gpu", "verify", "verify-gpu"], r.stdout
    assert f"{TOTAL} frames: {TOTAL} same, " in lines[2] and f"verify-gpu: {TOTAL} frames compared on GPU 0 " in lines[3]
    w = fresh(base, tmp_path / "t")
    tamper_25(w)
    args = ("-d", os.path.dirname(w.src), "-r", RUN_ID, "--verify-repack", os.path.dirname(w.out))
    a, b = cli(*args), cli(*args, "--verify-gpu")
    assert a.returncode == b.returncode == 1, a.stderr + b.stderr
    la, lb = a.stdout.splitlines(), b.stdout.splitlines()
    assert len(la) == 22 and len(lb) == 23 and lb[22].startswith("verify-gpu: ") and la[20] == lb[20] == "... and 5 more"
    assert la[:21] == lb[:21]
    assert la[21].rsplit("; ", 1)[0] == lb[21].rsplit("; ", 1)[0] and la[21].startswith("verify: 4 events, ")
