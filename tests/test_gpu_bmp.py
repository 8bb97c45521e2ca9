"""BMP frames decoded on the GPU (abub_bmp_decode_dev, csrc/abub_bmp.hip) against the host decoder (host.imdecode, which
test_ingest.test_bmp_decode_matches_pillow pins to Pillow): the kernel on every pixel format, row order and alignment,
between canaries; descriptors that lie; and the five device reading routes on runs whose frames are BMP files."""
import os
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import bmpfiles
from autobub3hs_amd import hip, host, synth
from test_ingest import make_run_dir, png_bytes, zip_run
from test_train_device import write_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
DEV = "cuda:0"
CANARY = 0xC7
NONE = 0xFFFFFFFF
RUN_ID = "20200925_1"
BMP_FORMAT = "cam%d_image%u.bmp"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- the kernel ---------------------------------------------------------------------------------------------------
def place(files, rs, odd_base=False):
    """the files at multiples of 16 in one buffer, other bytes in front, between and (except behind the last) behind
    them -> (device tensor, offsets); odd_base: the buffer itself starts at an odd address"""
    blob = bytearray(rs.randint(0, 256, 16 * rs.randint(1, 4)).astype(np.uint8).tobytes())
    offs = []
    for i, d in enumerate(files):
        offs.append(len(blob))
        blob += d
        if i + 1 < len(files):
            blob += rs.randint(0, 256, (-len(blob)) % 16 + 16 * rs.randint(0, 3)).astype(np.uint8).tobytes()
    t = torch.frombuffer(bytearray(bytes(odd_base) + bytes(blob)), dtype=torch.uint8).to(DEV)
    if odd_base:
        t = t[1:]
        assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    return t, offs


def descriptors(files, offs, W, H):
    """-> (rows for hip.bmp_decode without dst, luts tensor or None): what buildFileDescs makes of bmpWalk's answer"""
    rows, luts = [], []
    for d, o in zip(files, offs):
        info = host.bmp_walk(d, W, H)
        assert info is not None and info == hip.bmp_parse(d, W, H)
        li = NONE
        if info["bpp"] <= 8 and not info["identity"]:
            if info["lut"] not in luts:
                luts.append(info["lut"])
            li = luts.index(info["lut"])
        rows.append([o, len(d), info["data_off"], info["stride"], info["bpp"], int(info["top_down"]), li])
    lt = torch.frombuffer(bytearray(b"".join(luts)), dtype=torch.uint8).to(DEV) if luts else None
    return rows, lt


def scatter(n, P, rs):
    """n frames of P bytes at scattered, unaligned offsets -> (offsets, bytes of the whole output)"""
    offs, cur = [], 0
    for _ in range(n):
        cur += int(rs.randint(1, 40))
        offs.append(cur)
        cur += P
    return offs, cur + int(rs.randint(1, 40))


def decode_group(files, W, H, seed, odd_base=False):
    """one launch over `files` (all W x H): every status 0, the pixels the host decoder's, the canaries intact"""
    rs = np.random.RandomState(seed)
    want = [host.imdecode(d, cap=1 << 23) for d in files]
    assert all(w is not None and w.shape == (H, W) for w in want)
    d_files, offs = place(files, rs, odd_base)
    rows, luts = descriptors(files, offs, W, H)
    dst, total = scatter(len(files), W * H, rs)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
    st = hip.bmp_decode(d_files, [r + [o] for r, o in zip(rows, dst)], luts, W, H, out)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all(), st
    got = out.cpu().numpy()
    mask = np.ones(total, bool)
    for i, o in enumerate(dst):
        assert np.array_equal(got[o:o + W * H].reshape(H, W), want[i]), (W, H, i)
        mask[o:o + W * H] = False
    assert (got[mask] == CANARY).all()


def eight_bit_files(W, H, rs):
    idx = rs.randint(0, 256, (H, W))
    colours = rs.randint(0, 256, (256, 4))
    files = [bmpfiles.make_bmp(idx, 8),                                  # bottom-up, the grey ramp: no table
             bmpfiles.make_bmp(idx, 8, top_down=True, palette=colours),  # top-down, with a table
             bmpfiles.make_bmp(idx, 8, ncol=16, palette=colours[:16]),   # a short palette
             bmpfiles.pillow_bmp(idx.astype(np.uint8), "L")]
    for gap in range(4):  # data_off = 0, 1, 2, 3 mod 4, with and without a table
        files.append(bmpfiles.make_bmp(idx, 8, gap=gap + 2, palette=colours if gap & 1 else None, top_down=gap >= 2))
        files.append(bmpfiles.make_bmp(idx, 8, gap=gap + 2, palette=None if gap & 1 else colours))
    assert {host.bmp_walk(f, W, H)["data_off"] % 4 for f in files} == {0, 1, 2, 3}
    return files


@pytest.mark.parametrize("H", [1, 2, 9, 33])
def test_eight_bit_shapes(H):
    """one row, more rows than a wave owns (8), more than a workgroup owns (32); widths around the 16-byte pieces, the
    wave's 64 lanes and 256"""
    for W in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257):
        decode_group(eight_bit_files(W, H, np.random.RandomState(W * 100 + H)), W, H, seed=W + H)
    decode_group(eight_bit_files(65, H, np.random.RandomState(H)), 65, H, seed=H, odd_base=True)


@pytest.mark.parametrize("W,H", [(1280, 8), (1680, 6)])
def test_eight_bit_crops_of_the_camera_sizes(W, H):
    rs = np.random.RandomState(W)
    spec = synth.random_spec(W, 64, 12, 300, 0, margin=10)
    frame = synth.render_event(W, 64, spec, 300, 0)[spec.F - 1][20:20 + H]
    files = eight_bit_files(W, H, rs) + [bmpfiles.pillow_bmp(np.ascontiguousarray(frame), "L"),
                                         bmpfiles.pillow_bmp(np.ascontiguousarray(frame), "P", palette_seed=2)]
    decode_group(files, W, H, seed=W)


def test_other_pixel_formats():
    rs = np.random.RandomState(21)
    colours = rs.randint(0, 256, (16, 4))
    for H in (1, 9, 33):
        for W in (1, 7, 8, 9, 33):
            i1 = rs.randint(0, 2, (H, W))
            decode_group([bmpfiles.make_bmp(i1, 1), bmpfiles.make_bmp(i1, 1, top_down=True, palette=colours[:2]),
                          bmpfiles.pillow_bmp((i1 * 255).astype(np.uint8), "1")], W, H, seed=W)
        for W in (1, 2, 3, 9):
            i4 = rs.randint(0, 16, (H, W))
            decode_group([bmpfiles.make_bmp(i4, 4), bmpfiles.make_bmp(i4, 4, top_down=True, palette=colours, gap=1)], W, H, seed=W)
        for W in (1, 2, 3, 5):  # row padding 1, 2, 3, 1
            c3 = rs.randint(0, 256, (H, W, 3))
            decode_group([bmpfiles.make_bmp(c3, 24), bmpfiles.make_bmp(c3, 24, top_down=True, gap=3),
                          bmpfiles.pillow_bmp(rs.randint(0, 256, (H, W)).astype(np.uint8), "RGB")], W, H, seed=W)
        for W in (1, 3, 66):
            c4 = rs.randint(0, 256, (H, W, 4))
            decode_group([bmpfiles.make_bmp(c4, 32), bmpfiles.make_bmp(c4, 32, comp=3, top_down=True, hdr=108)], W, H, seed=W)


@pytest.mark.parametrize("name", ["sample_40l19_cam1_bellows_mask.bmp", "sample_40l19_cam1_mask.bmp"])
def test_reference_sample_masks(name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    img = host.imdecode(data, cap=1 << 23)
    H, W = img.shape
    decode_group([data, data], W, H, seed=3)


def test_lying_descriptors_between_intact_neighbours():
    W, H = 65, 9
    rs = np.random.RandomState(4)
    P = W * H
    files = eight_bit_files(W, H, rs)[:8] + eight_bit_files(W, H, rs)[:5]
    n = len(files)
    want = [host.imdecode(d) for d in files]
    d_files, offs = place(files, rs)
    rows, luts = descriptors(files, offs, W, H)
    nluts = luts.numel() // 256
    dst, total = scatter(n, P, rs)
    total = dst[-1] + P  # (the last frame ends the output)
    desc = [r + [o] for r, o in zip(rows, dst)]
    liars = {1: "off + len", 3: "data_off + stride * H", 5: "stride", 7: "bpp", 9: "lut", 12: "dst"}
    desc[1][1] = d_files.numel() - desc[1][0] + 1   # off + len one past files_bytes
    desc[3][2] = desc[3][1] - desc[3][3] * H + 1     # data_off + stride * H one past len
    desc[5][3] = W - 1                               # stride one below ceil(W * bpp / 8)
    desc[7][4] = 7                                   # bpp 7
    desc[9][6] = nluts                               # lut == nluts
    desc[12][7] = total - P + 1                      # dst + W * H one past out_bytes
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
    st = hip.bmp_decode(d_files, desc, luts, W, H, out).cpu().numpy()
    got = out.cpu().numpy()
    for i in range(n):
        o = dst[i]
        if i in liars:
            assert st[i] == 1, (liars[i], st)
            if i != 12:
                assert (got[o:o + P] == CANARY).all(), liars[i]
        else:
            assert st[i] == 0, (i, st)
            assert np.array_equal(got[o:o + P].reshape(H, W), want[i]), i
    keep = np.ones(total, bool)
    for i in range(n):
        if i not in liars:
            keep[dst[i]:dst[i] + P] = False
    assert (got[keep] == CANARY).all()  # (frame 12's own place included: it lies one byte back)
    # the limits themselves are taken: the same descriptors one step back decode
    desc[1][1] = d_files.numel() - desc[1][0]
    desc[3][2] -= 1
    desc[12][7] = total - P
    desc[5][3], desc[7][4], desc[9][6] = rows[5][3], 8, NONE
    st = hip.bmp_decode(d_files, desc, luts, W, H, out).cpu().numpy()
    assert (st == 0).all(), st
    # a descriptor is all the kernel believes: data_off 0 in a buffer at an odd address gives the file's own first bytes
    d_odd, offs = place(files[:2], rs, odd_base=True)
    out = torch.full((2 * P + 7,), CANARY, dtype=torch.uint8, device=DEV)
    st = hip.bmp_decode(d_odd, [[offs[0], len(files[0]), 0, W, 8, 1, NONE, 3], [0, d_odd.numel(), 0, W, 8, 0, NONE, P + 5]], None, W, H, out)
    assert (st.cpu().numpy() == 0).all()
    got, raw = out.cpu().numpy(), d_odd.cpu().numpy()
    assert np.array_equal(got[3:3 + P], raw[offs[0]:offs[0] + P])
    assert np.array_equal(got[P + 5:2 * P + 5].reshape(H, W), raw[:P].reshape(H, W)[::-1])
    assert (got[:3] == CANARY).all() and (got[3 + P:5 + P] == CANARY).all() and (got[2 * P + 5:] == CANARY).all()


def test_many_files_on_reused_buffers():
    W, H, n = 64, 3, 300
    P = W * H
    out = torch.empty((n * (P + 40) + 40,), dtype=torch.uint8, device=DEV)
    status = torch.empty((n,), dtype=torch.int32, device=DEV)
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        kinds = eight_bit_files(W, H, rs)
        files = [kinds[(i * 5 + seed) % len(kinds)] for i in range(n)]
        want = [host.imdecode(d) for d in kinds]
        d_files, offs = place(files, rs)
        rows, luts = descriptors(files, offs, W, H)
        dst, total = scatter(n, P, rs)
        out.fill_(CANARY)
        status.fill_(99)
        st = hip.bmp_decode(d_files, [r + [o] for r, o in zip(rows, dst)], luts, W, H, out, status=status)
        assert (st.cpu().numpy() == 0).all()
        got = out.cpu().numpy()
        keep = np.ones(len(got), bool)
        for i, o in enumerate(dst):
            assert np.array_equal(got[o:o + P].reshape(H, W), want[(i * 5 + seed) % len(kinds)]), i
            keep[o:o + P] = False
        assert (got[keep] == CANARY).all()


# ---- runs ---------------------------------------------------------------------------------------------------------
W_RUN, H_RUN, F_RUN = 320, 128, 20


@pytest.fixture(scope="module")
def bmp_run(tmp_path_factory):
    """a BMP run of five events and two cameras; among the frames a truncated BMP, an empty file, a BMP of another size,
    a file named .bmp that holds PNG bytes and one that holds packed bytes -> (run dir, stored zip, deflated zip, frames)"""
    root = str(tmp_path_factory.mktemp("bmprun"))
    rd, frames = make_run_dir(root, W=W_RUN, H=H_RUN, F=F_RUN, nev=5, ncams=2, fmt="bmp")
    d3, d4 = os.path.join(rd, "3", "Images"), os.path.join(rd, "4", "Images")
    data = open(os.path.join(d3, "cam1_image40.bmp"), "rb").read()
    open(os.path.join(d3, "cam1_image40.bmp"), "wb").write(data[:len(data) // 2])  # truncated
    open(os.path.join(d4, "cam0_image33.bmp"), "wb").close()  # empty
    Image.fromarray(np.zeros((H_RUN, W_RUN + 4), np.uint8)).save(os.path.join(d4, "cam1_image35.bmp"))  # another size
    open(os.path.join(d3, "cam0_image37.bmp"), "wb").write(png_bytes(frames[(3, 0, "cam0_image37.bmp")]))  # PNG bytes
    open(os.path.join(d4, "cam0_image41.bmp"), "wb").write(host.abf_encode(frames[(4, 0, "cam0_image41.bmp")]))  # packed bytes
    zs, zd = os.path.join(root, "stored.zip"), os.path.join(root, "deflated.zip")
    zip_run(rd, zs, zipfile.ZIP_STORED)
    zip_run(rd, zd, zipfile.ZIP_DEFLATED)
    return rd, zs, zd, frames


TOTAL = 5 * 2 * F_RUN


def batched(kind, src, outdir, env, monkeypatch, image_format=BMP_FORMAT, batch_mb=2):
    """one RunBatched with the BMP decoder on (ABUB_GPU_BMP=1; it is off by default) unless `env` says otherwise; an
    ABUB_GPU_BMP of None leaves the variable unset"""
    for k in ("ABUB_GPU_DECODE", "ABUB_GPU_BMP", "ABUB_GPU_DECODE_EVENTS", "ABUB_HOST_DECODE_EVENTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict({"ABUB_GPU_BMP": "1"}, **env).items():
        if v is not None:
            monkeypatch.setenv(k, v)
    os.makedirs(outdir, exist_ok=True)
    run = host.Run(kind, src, "Images", image_format)
    try:
        for c in range(2):
            assert run.train(c, shape=(H_RUN, W_RUN))[0] == 0
        st = run.run_batched(2, outdir + "/", "r", 30, nthreads=4, decode_threads=4, batch_mb=batch_mb)
    finally:
        run.close()
    return st, open(os.path.join(outdir, "abub3hs_r.txt")).read()


@pytest.fixture(scope="module")
def bmp_reference(bmp_run, tmp_path_factory):
    """the text of the run with every frame decoded by host threads"""
    mp = pytest.MonkeyPatch()
    try:
        st, text = batched("raw", bmp_run[0] + "/", str(tmp_path_factory.mktemp("ref")), {"ABUB_GPU_DECODE": "0"}, mp)
    finally:
        mp.undo()
    assert st["frames_gpu_decoded"] == 0 and st["frames_gpu_bmp"] == 0 and st["frames_failed"] == 3
    assert st["frames"] == TOTAL - 3 and len(text.splitlines()) >= 12
    return text


@pytest.mark.parametrize("source", ["raw", "stored", "deflated"])
def test_batched_bmp_run(bmp_run, bmp_reference, tmp_path, monkeypatch, source):
    rd, zs, zd, _ = bmp_run
    kind, src = {"raw": ("raw", rd + "/"), "stored": ("zip", zs), "deflated": ("zip", zd)}[source]
    st, text = batched(kind, src, str(tmp_path / "gpu"), {}, monkeypatch)
    assert text == bmp_reference
    # every intact BMP by the BMP kernel, the PNG and the packed file by their own kernels: one batch runs all three
    assert st["frames_gpu_bmp"] == TOTAL - 5 and st["frames_gpu_unpacked"] == 1 and st["frames_gpu_decoded"] == TOTAL - 3, st
    assert st["frames_failed"] == 3 and st["frames_host_decoded"] == 0, st


def test_batched_bmp_run_with_the_decoder_off(bmp_run, bmp_reference, tmp_path, monkeypatch):
    st, text = batched("raw", bmp_run[0] + "/", str(tmp_path / "off"), {"ABUB_GPU_BMP": "0"}, monkeypatch)
    assert text == bmp_reference
    assert st["frames_gpu_bmp"] == 0 and st["frames_gpu_decoded"] == 0 and st["frames_failed"] == 3, st
    st, text = batched("raw", bmp_run[0] + "/", str(tmp_path / "unset"), {"ABUB_GPU_BMP": None}, monkeypatch)  # the default
    assert text == bmp_reference
    assert st["frames_gpu_bmp"] == 0 and st["frames_gpu_decoded"] == 0 and st["frames_failed"] == 3, st


def test_batched_bmp_run_in_one_event_batches(bmp_run, bmp_reference, tmp_path, monkeypatch):
    st, text = batched("zip", bmp_run[1], str(tmp_path / "one"), {"ABUB_GPU_DECODE_EVENTS": "1"}, monkeypatch, batch_mb=64)
    assert text == bmp_reference
    assert st["events_per_batch"] == 1 and st["batches"] == 6, st  # (six event directories: 0..4 and the frame-less 9)
    assert st["frames_gpu_bmp"] == TOTAL - 5 and st["frames_gpu_decoded"] == TOTAL - 3 and st["frames_failed"] == 3, st


def test_png_run_with_one_bmp_frame(tmp_path, monkeypatch):
    rd, frames = make_run_dir(str(tmp_path / "data"), W=W_RUN, H=H_RUN, F=F_RUN, nev=4, ncams=2)
    victim = os.path.join(rd, "2", "Images", "cam1_image36.png")
    open(victim, "wb").write(bmpfiles.pillow_bmp(frames[(2, 1, "cam1_image36.png")], "L"))
    ref_st, ref = batched("raw", rd + "/", str(tmp_path / "host"), {"ABUB_GPU_DECODE": "0"}, monkeypatch, "cam%d_image%u.png")
    st, text = batched("raw", rd + "/", str(tmp_path / "gpu"), {}, monkeypatch, "cam%d_image%u.png")
    assert text == ref and ref_st["frames_gpu_bmp"] == 0
    assert st["frames_gpu_bmp"] == 1 and st["frames_gpu_decoded"] == 4 * 2 * F_RUN and st["frames_host_decoded"] == 0, st
    st, text = batched("raw", rd + "/", str(tmp_path / "off"), {"ABUB_GPU_BMP": "0"}, monkeypatch, "cam%d_image%u.png")
    assert text == ref
    assert st["frames_gpu_bmp"] == 0 and st["frames_gpu_decoded"] == 4 * 2 * F_RUN - 1 and st["frames_host_decoded"] == 1, st


def test_train_on_gpu_from_a_bmp_run(tmp_path, monkeypatch):
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    E, C = 5, 2
    rd = write_run(str(tmp_path), ext="bmp", nev=E, ncams=C)
    dev_run = host.Run("raw", rd + "/", "Images", BMP_FORMAT)
    got = dev_run.train_on_gpu(C, shape=(128, 320))
    assert dev_run.train_path == "device"
    assert dev_run.train_stats["frames_gpu_bmp"] == 2 * E * C == dev_run.train_stats["frames_gpu_decoded"], dev_run.train_stats
    assert dev_run.train_stats["frames_host_decoded"] == 0
    dev_run.close()
    host_run = host.Run("raw", rd + "/", "Images", BMP_FORMAT)
    for c in range(C):
        st, tss, mu, sg = host_run.train(c, shape=(128, 320))
        assert (got[c][0], got[c][1]) == (st, tss) == (0, 2 * E)
        assert np.array_equal(got[c][2], mu) and np.array_equal(got[c][3], sg)
    host_run.close()


def tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def cli(*args):
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4", ABUB_GPU_BMP="1")
    env.pop("ABUB_GPU_DECODE", None)
    r = subprocess.run([EXE] + list(args), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_repack_unpack_and_verify_from_a_bmp_run(bmp_run, tmp_path, monkeypatch):
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    rd = bmp_run[0]
    encoded = TOTAL - 3  # the truncated and the empty file are copied, the other size takes the host route
    for op in ("repack", "unpack"):
        run = host.Run("raw", rd + "/", "Images", BMP_FORMAT)
        try:
            a, b = str(tmp_path / (op + "_host") / RUN_ID), str(tmp_path / (op + "_dev") / RUN_ID)
            sh = getattr(run, op)(a, nthreads=4, ncams=2)
            sd = getattr(run, op)(b, nthreads=4, ncams=2, device=0)
        finally:
            run.close()
        for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
            assert sh[k] == sd[k], (op, k)
        ta, tb = tree(a), tree(b)
        assert sorted(ta) == sorted(tb) and len(ta) == TOTAL + 1
        for name in ta:
            assert ta[name] == tb[name], (op, name)
        assert sd["frames_gpu_bmp_decoded"] == TOTAL - 5 and sd["frames_gpu_unpacked"] == 1 and sd["frames_gpu_png_decoded"] == 1, sd
        assert sd["frames_gpu_png_decoded"] + sd["frames_gpu_unpacked"] + sd["frames_gpu_bmp_decoded"] + sd["frames_host_decoded"] == \
            sd["frames_gpu_encoded"] == encoded, sd
        assert "frames_gpu_bmp_decoded" not in sh
    src, other = host.Run("raw", rd + "/", "Images", BMP_FORMAT), host.Run("raw", str(tmp_path / "repack_dev" / RUN_ID) + "/", "Images", BMP_FORMAT)
    try:
        vh = src.verify(other, nthreads=4, ncams=2)
        vd = src.verify(other, nthreads=4, ncams=2, device=0)
    finally:
        src.close()
        other.close()
    for k in ("rc", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra", "findings"):
        assert vh[k] == vd[k], k
    # every frame that decodes is `same` (the frame that was packed already among them); the two that do not are copies
    assert vd["rc"] == 0 and vd["frames"] == TOTAL and vd["same"] == TOTAL - 2 and vd["copied"] == 2, vd
    assert vd["src_gpu_bmp_decoded"] == TOTAL - 5 and vd["other_gpu_bmp_decoded"] == 0 and vd["other_gpu_unpacked"] == TOTAL - 3, vd
    assert vh["src_gpu_bmp_decoded"] == 0 and vh["device"] == -1


def test_cli_lines(bmp_run, tmp_path):
    """a BMP run adds one line behind each device route's line; a PNG run prints exactly the lines it prints today"""
    data = os.path.dirname(bmp_run[0])
    b, u = str(tmp_path / "B"), str(tmp_path / "U")
    so = cli("-d", data, "-r", RUN_ID, "--repack", b, "--repack-gpu", "--verify-repack", b, "--verify-gpu")
    lines = so.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("repack-gpu: ")]
    assert len(at) == 2 and at[1] == at[0] + 1 and lines[at[1]] == f"repack-gpu: {TOTAL - 5} frames decoded by the BMP kernel", so
    assert f"{TOTAL - 3} frames encoded on GPU 0 (1 decoded by the PNG kernel, 1 by the packed kernel, 0 by a host thread), " in lines[at[0]]
    at = [i for i, l in enumerate(lines) if l.startswith("verify-gpu: ")]
    assert len(at) == 2 and at[1] == at[0] + 1, so
    assert lines[at[1]] == f"verify-gpu: {TOTAL - 5} frames decoded by the BMP kernel (the source's {TOTAL - 5}, the copy's 0)", so
    so = cli("-d", data, "-r", RUN_ID, "--unpack", u, "--unpack-gpu")
    assert f"unpack-gpu: {TOTAL - 5} frames decoded by the BMP kernel" in so.splitlines(), so
    assert "ABUB_GPU_BMP=1" in subprocess.run([EXE, "-h"], capture_output=True, text=True).stdout
    # a PNG run
    rd, _ = make_run_dir(str(tmp_path / "png"), W=96, H=64, F=4, nev=2, ncams=2)
    p = str(tmp_path / "P")
    so = cli("-d", os.path.dirname(rd), "-r", RUN_ID, "--repack", p, "--repack-gpu", "--verify-repack", p, "--verify-gpu")
    assert "BMP" not in so
    assert [l.split(":")[0] for l in so.splitlines() if l.startswith(("repack", "verify"))] == ["repack", "repack-gpu", "verify", "verify-gpu"], so
    so = cli("-d", os.path.dirname(rd), "-r", RUN_ID, "--unpack", str(tmp_path / "PU"), "--unpack-gpu")
    assert "BMP" not in so and [l.split(":")[0] for l in so.splitlines() if l.startswith("unpack")] == ["unpack", "unpack-gpu"], so


def test_cli_on_the_layout_of_a_bmp_series(tmp_path):
    """-D 2l-16: frames "cam<c>image <n>.bmp" in the event folder itself, two cameras -- the batched text is --per-event's"""
    W, H, F, nev = 320, 128, 20, 4
    rd = os.path.join(str(tmp_path), "data", RUN_ID)
    for e in range(nev):
        for c in range(2):
            spec = synth.random_spec(W, H, F, 700 + e, c, margin=10)
            st = synth.render_event(W, H, spec, 700 + e, c)
            os.makedirs(os.path.join(rd, str(e)), exist_ok=True)
            for k in range(F):
                Image.fromarray(st[k]).save(os.path.join(rd, str(e), f"cam{c}image {10 + k}.bmp"))
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(nev):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    texts = {}
    for tag, extra in (("batched", []), ("per_event", ["--per-event"])):
        out = str(tmp_path / tag)
        os.makedirs(out)
        so = cli("-d", os.path.dirname(rd), "-r", RUN_ID, "-o", out, "-D", "2l-16", *extra)
        assert ("batched detect:" in so) == (tag == "batched"), so
        texts[tag] = open(os.path.join(out, f"abub3hs_{RUN_ID}.txt")).read()
    assert texts["batched"] == texts["per_event"] and len(texts["batched"].splitlines()) >= 6 + nev
