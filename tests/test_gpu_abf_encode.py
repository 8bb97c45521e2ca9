"""Packed frames ("ABF1") encoded on the GPU: abub_abf_encode_dev against the host encoder (cv::abfEncode) and the numpy
restatement of the format (tests/abfref.py), bit for bit; its capacity and source errors; the scan across many files; the
round trip through abub_abf_decode_dev on the device; and abub3hs --repack --repack-gpu / Run.repack(device=0) against the
host repack, file by file."""
import functools
import os
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import abfref
import enclayout
from autobub3hs_amd import _lib, hip, host, synth
from enclayout import CANARY, DEV, E_CAP, E_SRC, align16, check_layout, expected_layout, scatter, tree
from test_abf_format import all_contents, make_run_dir, zip_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1), (2, 1), (63, 2), (64, 3), (65, 3), (127, 2), (128, 9), (129, 9), (257, 9), (1280, 9), (2050, 2), (4100, 1)]  # W x H
RUN_ID = "20200925_1"
encode = functools.partial(enclayout.encode, hip.abf_encode)


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def sources():
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = synth.render_event(320, 128, spec, 300, 0)[spec.F - 1]
    return {"sample": sample, "synth": np.ascontiguousarray(frame)}


def worst(W, H):
    """every difference is +-128, which zigzags to 255: every block 8 bits wide, the file as long as abub_abf_file_bound"""
    return np.ascontiguousarray(np.broadcast_to((128 * (np.arange(W) & 1)).astype(np.uint8), (H, W)))


def ladder(W, H):
    """block (y, k) needs exactly (y + k) mod 9 bits: constant for 0, a falling ramp of step -1 for 1, and for b >= 2 pixels
    alternating between 100 and 100 + 2^(b - 2) (the step up zigzags to 2^(b - 1))"""
    img = np.zeros((H, W), np.uint8)
    j = np.arange(64)
    for y in range(H):
        for k in range((W + 63) // 64):
            b = (y + k) % 9
            blk = np.full(64, 77) if b == 0 else 200 - j if b == 1 else 100 + (j & 1) * (1 << (b - 2))
            n = min(64, W - 64 * k)
            img[y, 64 * k:64 * k + n] = blk[:n]
    return img


@pytest.mark.parametrize("W,H", SHAPES)
def test_kernel_writes_the_host_encoders_bytes(sources, W, H):
    rs = np.random.RandomState(W * 16 + H)
    named = dict(all_contents(sources, W, H, seed=W), worst=worst(W, H), ladder=ladder(W, H))
    imgs = list(named.values())
    buf, offs = scatter(imgs, rs)
    want = [abfref.encode(im) for im in imgs]
    assert want == [host.abf_encode(im) for im in imgs]
    bound = _lib.lib().abub_abf_file_bound(W, H)
    assert len(want[list(named).index("worst")]) == bound
    files, total, out = encode(buf, offs, W, H, len(imgs) * align16(bound) + 64)
    assert (files[:, 2] == 0).all(), files
    check_layout(files, total, out, want, [True] * len(imgs))
    # the ladder really has every width, where the shape has nine (y + k) classes of whole blocks
    nblk = (W + 63) // 64
    if H + (W // 64) - 1 >= 9:
        f = want[list(named).index("ladder")]
        t0, w0, p0 = abfref.regions(W, H)
        assert set(f[w0:w0 + H * nblk]) == set(range(9))


def test_capacity_errors_leave_the_file_unwritten_and_total_true():
    W, H, n = 65, 3, 3
    imgs = [worst(W, H)] * n
    buf, offs = scatter(imgs, np.random.RandomState(5))
    want = [abfref.encode(im) for im in imgs]
    bound = _lib.lib().abub_abf_file_bound(W, H)
    assert all(len(w) == bound for w in want)
    room = n * align16(bound)
    _, end = expected_layout([bound] * n)
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
    want = [abfref.encode(im) for im in imgs]
    want[2] = b""
    files, total, out = encode(buf, offs, W, H, 4 * align16(len(want[0]) + 64))
    assert list(files[:, 2]) == [0, 0, E_SRC, 0]
    check_layout(files, total, out, want, [True, True, False, True])
    offs[2] = len(buf) - W * H  # the last place a frame fits
    files, total, out = encode(buf, offs, W, H, 4 * align16(len(want[0]) + 64))
    assert list(files[:, 2]) == [0, 0, 0, 0] and files[2, 1] > 0


def test_many_files_and_a_reused_scratch(sources):
    """300 frames: the scan across files takes two rounds; then other content on the same scratch and `out`"""
    W, H, n = 64, 3, 300
    L = _lib.lib()
    scratch = torch.full((L.abub_abf_encode_scratch_bytes(n, W, H),), 0xEE, dtype=torch.uint8, device=DEV)
    room = n * align16(L.abub_abf_file_bound(W, H))
    whole = torch.full((room + 512,), CANARY, dtype=torch.uint8, device=DEV)
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        kinds = [list(all_contents(sources, W, H, seed=seed * 1000 + i).values()) for i in range(8)]
        imgs = [kinds[i % 8][(i * 5 + seed) % 7] for i in range(n)]
        buf, offs = scatter(imgs, rs)
        want = [host.abf_encode(im) for im in imgs]
        whole.fill_(CANARY)
        files, total, out = encode(buf, offs, W, H, room, out=whole, scratch=scratch)
        assert (files[:, 2] == 0).all()
        check_layout(files, total, out, want, [True] * n)


def test_round_trip_on_the_device(sources):
    """the encoder's output fed to abub_abf_decode_dev as it lies in `out`, the descriptors taken from `files`"""
    W, H, n = 1280, 64, 16
    kinds = [list(all_contents(sources, W, H, seed=i).values()) for i in range(3)]
    imgs = [kinds[i % 3][i % 7] for i in range(n)]
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    files, total, out = hip.abf_encode(frames, np.arange(n) * W * H, W, H)
    assert (files[:, 2] == 0).all() and total <= out.numel()
    back = torch.full((n, H, W), CANARY, dtype=torch.uint8, device=DEV)
    descs = [(int(o), int(l), i * W * H) for i, (o, l, _) in enumerate(files)]
    st = hip.abf_decode(out, descs, W, H, back)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    assert torch.equal(back, frames)
    assert out[int(files[3, 0]):int(files[3, 0] + files[3, 1])].cpu().numpy().tobytes() == host.abf_encode(imgs[3])


def test_repack_gpu_writes_the_trees_of_the_host_repack(tmp_path):
    W, H, F = 96, 64, 12
    rd, frames = make_run_dir(str(tmp_path / "data"), W, H, F, nev=3, ncams=2)
    d1 = os.path.join(rd, "1", "Images")
    victim = os.path.join(d1, "cam1_image33.png")
    open(victim, "wb").write(open(victim, "rb").read()[:200])  # a truncated PNG
    Image.fromarray(frames[(1, 0, "cam0_image37.png")].astype(np.uint16) << 8).save(os.path.join(d1, "cam0_image37.png"))  # 16 bit
    open(os.path.join(d1, "cam0_image31.png"), "wb").write(host.abf_encode(frames[(1, 0, "cam0_image31.png")]))  # packed already
    Image.fromarray(np.full((H + 2, W + 4), 9, np.uint8)).save(os.path.join(d1, "cam1_image40.png"))  # another size
    total = 3 * 2 * F
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
    env.pop("ABUB_GPU_DECODE", None)
    data = os.path.dirname(rd)

    def cli(*args):
        r = subprocess.run([exe] + list(args), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    line_a = cli("-d", data, "-r", RUN_ID, "--repack", a)
    lines_b = cli("-d", data, "-r", RUN_ID, "--repack", b, "--repack-gpu")
    first = [l for l in line_a.splitlines() if l.startswith("repack: ")]
    both = [l for l in lines_b.splitlines() if l.startswith("repack")]
    assert len(first) == 1 and len(both) == 2 and both[1].startswith("repack-gpu: ")
    assert f"repack: 4 events, {total - 1} frames packed" in both[0] and "1 copied as they are, 0 not written" in both[0]
    assert first[0].split(" not written")[0] == both[0].split(" not written")[0]
    # total - 4 frames on the GPU (one of them through the packed decoder); the 16-bit PNG, the other size and the truncated
    # file on host threads.  (A PNG cut behind its header may be planned for the GPU first: it ends on the host route.)
    assert f"{total - 3} frames encoded on GPU 0 ({total - 4} decoded by the PNG kernel, 1 by the packed kernel, 0 by a host thread), " \
           "3 took the host route" in both[1], both[1]
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb) and len(ta) == total + 1
    for name in ta:
        assert ta[name] == tb[name], name
    assert tb[os.path.join(RUN_ID, "1", "Images", "cam0_image31.png")] == open(os.path.join(d1, "cam0_image31.png"), "rb").read()

    # from a deflated archive, through the Python entry
    zpath = str(tmp_path / "data" / (RUN_ID + ".zip"))
    zip_run(rd, zpath, zipfile.ZIP_DEFLATED)
    run = host.Run("zip", zpath, "Images")
    try:
        sc = run.repack(str(tmp_path / "C" / RUN_ID), nthreads=3, ncams=2)
        sd = run.repack(str(tmp_path / "D" / RUN_ID), nthreads=3, ncams=2, device=0)
    finally:
        run.close()
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sc[k] == sd[k], k
    assert sd["packed"] == total - 1 and sd["copied"] == 1 and sd["failed"] == 0 and sd["device"] == 0
    assert sd["frames_gpu_encoded"] + sd["frames_host_route"] == total
    assert sd["frames_gpu_png_decoded"] + sd["frames_gpu_unpacked"] + sd["frames_host_decoded"] == sd["frames_gpu_encoded"] == total - 3
    assert sd["frames_gpu_unpacked"] == 1 and sd["batches"] == 1
    tc, td = tree(str(tmp_path / "C")), tree(str(tmp_path / "D"))
    assert sorted(tc) == sorted(td) and all(tc[n] == td[n] for n in tc)
    assert all(tc[n] == ta[n] for n in tc if not n.endswith(".txt"))

    # the analysis of tree B gives the result file of tree A
    for tag, src in (("oa", a), ("ob", b)):
        os.makedirs(str(tmp_path / tag))
        cli("-d", src, "-r", RUN_ID, "-o", str(tmp_path / tag))
    ra = open(str(tmp_path / "oa" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    rb = open(str(tmp_path / "ob" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    assert ra == rb and len(ra.splitlines()) >= 3
