"""Canonical Huffman-only PNG files written on the GPU: abub_png_encode_dev against the host encoder (cv::pngHuffEncode) and
the numpy restatement of the format (tests/pnghuffref.py), byte for byte, at the shapes where each mechanism can fail (rows
that share a byte, block ends, both length limits); its capacity and source errors; the scan across many files; the round
trip through abub_png_decode_dev on the device; and abub3hs --unpack --unpack-gpu / Run.unpack(device=0) against the host
unpack, file by file."""
import functools
import os
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import enclayout
import pnghuffref as ref
from autobub3hs_amd import _lib, hip, host, synth
from enclayout import CANARY, DEV, E_CAP, E_SRC, align16, check_layout, expected_layout, scatter, tree
from test_abf_format import make_packed_run, zip_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
RUN_ID = "20200925_1"
encode = functools.partial(enclayout.encode, hip.png_encode)
NAMES = ["w1_ones", "w1_sevens", "w2_ones", "3x5", "7x65", "63x3", "64x3", "65x3", "127x3", "128x3", "129x3", "1280x8", "1680x6",
         "160x96", "limit15", "limit7"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def cases():
    """name -> image: made once, shared, never changed"""
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = np.ascontiguousarray(synth.render_event(320, 128, spec, 300, 0)[spec.F - 1])
    imgs = ref.small_cases(sample, frame)
    imgs["limit15"] = ref.limit15_case()
    imgs["limit7"] = ref.limit7_case()
    assert sorted(imgs) == sorted(NAMES)
    return imgs


@pytest.mark.parametrize("name", NAMES)
def test_kernel_writes_the_host_encoders_bytes(cases, name):
    img = cases[name]
    H, W = img.shape
    rs = np.random.RandomState(W * 16 + H)
    imgs = [img, np.ascontiguousarray(img[::-1]), rs.randint(0, 256, (H, W)).astype(np.uint8), np.full((H, W), 200, np.uint8)]
    buf, offs = scatter(imgs, rs)
    want = [host.png_huff_encode(im) for im in imgs]
    assert want[0] == ref.encode(img)
    bound = _lib.lib().abub_png_file_bound(W, H)
    files, total, out = encode(buf, offs, W, H, len(imgs) * align16(bound) + 64)
    assert (files[:, 2] == 0).all(), files
    check_layout(files, total, out, want, [True] * len(imgs))


def test_capacity_errors_leave_the_file_unwritten_and_total_true():
    W, H, n = 65, 3, 3
    rs = np.random.RandomState(5)
    imgs = [rs.randint(0, 256, (H, W)).astype(np.uint8) for _ in range(n)]
    buf, offs = scatter(imgs, rs)
    want = [host.png_huff_encode(im) for im in imgs]
    room = n * align16(_lib.lib().abub_png_file_bound(W, H))
    _, end = expected_layout([len(w) for w in want])
    files, total, out = encode(buf, offs, W, H, room, out_cap=end)
    assert list(files[:, 2]) == [0, 0, 0] and total == end
    check_layout(files, total, out, want, [True] * n)
    files, total, out = encode(buf, offs, W, H, room, out_cap=end - 1)
    assert list(files[:, 2]) == [0, 0, E_CAP] and total == end
    check_layout(files, total, out, want, [True, True, False])
    files, total, out = encode(buf, offs, W, H, room, out_cap=0)
    assert list(files[:, 2]) == [E_CAP] * n and total == end
    check_layout(files, total, out, want, [False] * n)


def test_a_source_outside_the_pixels_takes_no_room():
    W, H = 127, 2
    rs = np.random.RandomState(9)
    imgs = [rs.randint(0, 256, (H, W)).astype(np.uint8) for _ in range(4)]
    buf, offs = scatter(imgs, rs)
    offs[2] = len(buf) - W * H + 1  # one byte past the end
    want = [host.png_huff_encode(im) for im in imgs]
    want[2] = b""
    room = 4 * align16(_lib.lib().abub_png_file_bound(W, H))
    files, total, out = encode(buf, offs, W, H, room)
    assert list(files[:, 2]) == [0, 0, E_SRC, 0]
    check_layout(files, total, out, want, [True, True, False, True])
    offs[2] = len(buf) - W * H  # the last place a frame fits
    files, total, out = encode(buf, offs, W, H, room)
    assert list(files[:, 2]) == [0, 0, 0, 0] and files[2, 1] > 0


def test_many_files_and_a_reused_scratch(cases):
    """300 frames: the scan across files takes two rounds; then other content on the same scratch and `out`"""
    W, H, n = 64, 3, 300
    L = _lib.lib()
    scratch = torch.full((L.abub_png_encode_scratch_bytes(n, W, H),), 0xEE, dtype=torch.uint8, device=DEV)
    room = n * align16(L.abub_png_file_bound(W, H))
    whole = torch.full((room + 512,), CANARY, dtype=torch.uint8, device=DEV)
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        kinds = [cases["64x3"], np.full((H, W), seed, np.uint8), cases["160x96"][seed:seed + H, :W], cases["1280x8"][:H, 100:100 + W]]
        imgs = [kinds[(i * 5 + seed) % 4] if i % 3 else rs.randint(0, 1 << (1 + i % 8), (H, W)).astype(np.uint8) for i in range(n)]
        buf, offs = scatter(imgs, rs)
        want = [host.png_huff_encode(im) for im in imgs]
        whole.fill_(CANARY)
        files, total, out = encode(buf, offs, W, H, room, out=whole, scratch=scratch)
        assert (files[:, 2] == 0).all()
        check_layout(files, total, out, want, [True] * n)


def test_round_trip_through_the_gpu_decoder(cases):
    """the encoder's files fed to abub_png_decode_dev: it takes every one (status 0, no host fall-back), the pixels are the source's"""
    W, H, n = 1280, 8, 6
    rs = np.random.RandomState(4)
    base = cases["1280x8"]
    imgs = [base, np.ascontiguousarray(base[::-1]), rs.randint(0, 256, (H, W)).astype(np.uint8), np.full((H, W), 9, np.uint8),
            rs.randint(0, 4, (H, W)).astype(np.uint8), np.ascontiguousarray(base[:, ::-1])]
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    files, total, out = hip.png_encode(frames, np.arange(n) * W * H, W, H)
    assert (files[:, 2] == 0).all() and total <= out.numel()
    got = out.cpu().numpy()
    pngs = [got[int(o):int(o + l)].tobytes() for o, l, _ in files]
    assert pngs == [host.png_huff_encode(im) for im in imgs]
    back, st = hip.png_decode(pngs, W, H, DEV)
    torch.cuda.synchronize()
    assert list(st) == [0] * n, st
    assert torch.equal(back, frames)


@pytest.mark.parametrize("name", ["limit15", "limit7"])
def test_round_trip_of_the_length_limited_codes(cases, name):
    """files whose literal code was repaired to 15 bits, and whose code-length code was repaired to 7, through the GPU inflate"""
    img = cases[name]
    H, W = img.shape
    assert W % 4 == 0 and 4 <= W <= 2048  # (the decoder's width gate)
    lengths = ref.code_lengths(ref.lit_counts(img), 15)
    if name == "limit15":
        assert max(lengths) == 15 and ref.unlimited_depth(ref.lit_counts(img)) > 15
    else:
        h = np.bincount(lengths + [0], minlength=19)
        assert max(ref.code_lengths(h, 7)) == 7 and ref.unlimited_depth(h) > 7
    imgs = [img, np.ascontiguousarray(img[::-1])]
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    files, total, out = hip.png_encode(frames, np.arange(2) * W * H, W, H)
    assert (files[:, 2] == 0).all()
    got = out.cpu().numpy()
    pngs = [got[int(o):int(o + l)].tobytes() for o, l, _ in files]
    assert pngs == [host.png_huff_encode(im) for im in imgs]
    back, st = hip.png_decode(pngs, W, H, DEV)
    torch.cuda.synchronize()
    assert list(st) == [0, 0], st
    assert torch.equal(back, frames)


def test_unpack_gpu_writes_the_trees_of_the_host_unpack(tmp_path):
    W, H, F = 96, 64, 6
    rd, frames = make_packed_run(str(tmp_path / "data"), W, H, F, nev=2, ncams=2)
    total = len(frames)
    d1 = os.path.join(rd, "1", "Images")
    Image.fromarray(frames[(1, 0, "cam0_image31.png")]).save(os.path.join(d1, "cam0_image31.png"))  # a PNG among the packed frames
    victim = os.path.join(d1, "cam1_image33.png")
    open(victim, "wb").write(open(victim, "rb").read()[:100])  # a truncated packed file: copied as it is
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4", ABUB_REPACK_BATCH="7")
    env.pop("ABUB_GPU_DECODE", None)
    data = os.path.dirname(rd)

    def cli(*args, timeout=120):
        r = subprocess.run([EXE] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    line_a = cli("-d", data, "-r", RUN_ID, "--unpack", a)
    lines_b = cli("-d", data, "-r", RUN_ID, "--unpack", b, "--unpack-gpu", "--verify-repack", b, "--verify-gpu")
    first = [l for l in line_a.splitlines() if l.startswith("unpack: ")]
    # (verify names every frame that is the same but not packed -- the first 20 -- in front of its summary)
    both = [l for l in lines_b.splitlines() if not l.endswith(": same but not packed") and not l.startswith("... and ")]
    assert [l.split(":")[0] for l in both] == ["unpack", "unpack-gpu", "verify", "verify-gpu"], lines_b
    assert f"unpack: 2 events, {total - 1} frames written as PNG" in both[0] and "1 copied as they are, 0 not written" in both[0]
    assert first[0].split(" not written")[0] == both[0].split(" not written")[0]
    assert f"{total - 1} frames encoded on GPU 0 (1 decoded by the PNG kernel, {total - 2} by the packed kernel, 0 by a host thread), " \
           f"1 took the host route, {(total + 6) // 7} batches" in both[1], both[1]
    assert f"{total} frames: 0 same, {total - 1} same but not packed, 1 copied, 0 differ, 0 missing, 0 undecodable, 0 extra" in both[2]
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb) and len(ta) == total + 1
    for name in ta:
        assert ta[name] == tb[name], name
    assert tb[os.path.join(RUN_ID, "0", "Images", "cam0_image30.png")] == host.png_huff_encode(frames[(0, 0, "cam0_image30.png")])

    # from a stored archive, through the Python entry, in one batch
    zpath = str(tmp_path / "data" / (RUN_ID + ".zip"))
    zip_run(rd, zpath, zipfile.ZIP_STORED)
    run = host.Run("zip", zpath, "Images")
    try:
        sc = run.unpack(str(tmp_path / "C" / RUN_ID), nthreads=3, ncams=2)
        sd = run.unpack(str(tmp_path / "D" / RUN_ID), nthreads=3, ncams=2, device=0)
    finally:
        run.close()
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sc[k] == sd[k], k
    assert sd["packed"] == total - 1 and sd["copied"] == 1 and sd["failed"] == 0 and sd["device"] == 0
    assert sd["frames_gpu_encoded"] == total - 1 and sd["frames_host_route"] == 1 and sd["batches"] == 1
    tc, td = tree(str(tmp_path / "C")), tree(str(tmp_path / "D"))
    assert sorted(tc) == sorted(td) and all(tc[n] == td[n] for n in tc)
    assert all(tc[n] == ta[n] for n in tc if not n.endswith(".txt"))

    # the analysis of the unpacked run gives the result file of the source, decoded by host threads
    env["ABUB_GPU_DECODE"] = "0"
    for tag, src in (("os", data), ("oa", a), ("ob", b)):
        os.makedirs(str(tmp_path / tag))
        cli("-d", src, "-r", RUN_ID, "-o", str(tmp_path / tag))
    rs_, ra, rb = (open(str(tmp_path / tag / f"abub3hs_{RUN_ID}.txt"), "rb").read() for tag in ("os", "oa", "ob"))
    assert rs_ == ra == rb and len(rs_.splitlines()) >= 2
