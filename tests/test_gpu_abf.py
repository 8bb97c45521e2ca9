"""Packed frames ("ABF1") on the GPU: abub_abf_decode_dev against the pixels that were packed and against the numpy
restatement of the format (tests/abfref.py) on damaged files; then the reading path: batched runs, device training and the
command line on a repacked run give what the PNG run gives."""
import os
import shutil
import struct
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import abfref
from autobub3hs_amd import hip, host, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CANARY = 0xA5
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def sources():
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = synth.render_event(320, 128, spec, 300, 0)[spec.F - 1]
    return {"sample": sample, "synth": np.ascontiguousarray(frame)}


def crop(img, W, H, x0=0, y0=0):
    img = img[y0:, x0:]
    reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
    return np.ascontiguousarray(np.tile(img, reps)[:H, :W])


def mixed_frames(sources, W, H, n, seed):
    """n frames cycling through every content class: zero, constant, random, wrapping ramp, noise, sample crop, synth"""
    out = []
    for i in range(n):
        c = abfref.contents(W, H, seed + i)
        c["sample"] = crop(sources["sample"], W, H, 600 + 13 * i, 300 + 7 * i)
        c["synth"] = crop(sources["synth"], W, H, 5 * i, i)
        names = sorted(c)
        out.append(c[names[i % len(names)]])
    return out


def lay_out(files, tail=0):
    """the files one after the other at 16-byte-rounded offsets, as planFileTask lays them out -> (blob, offsets)"""
    blob, offs = bytearray(), []
    for f in files:
        offs.append(len(blob))
        blob += f
        blob += b"\0" * (-len(blob) % 16)
    blob += b"\0" * tail
    return blob, offs


def scattered(n, P, rs, odd):
    """destinations of n frames of P bytes: unordered, with gaps, at odd addresses where asked -> (offsets, total bytes)"""
    order = rs.permutation(n)
    offs = np.zeros(n, np.int64)
    at = 37
    for slot in order:
        at += int(rs.randint(1, 40))
        if odd and at % 2 == 0:
            at += 1
        offs[slot] = at
        at += P
    return offs, at + 29


def run_decode(blob, descs, W, H, out_bytes, files_bytes=None):
    d_files = torch.frombuffer(bytearray(blob) or bytearray(1), dtype=torch.uint8).to(DEV)
    if files_bytes is not None:
        d_files = d_files[:files_bytes].contiguous()
    # canaries in front of and behind `out`: the launcher is handed the middle
    whole = torch.full((out_bytes + 512,), CANARY, dtype=torch.uint8, device=DEV)
    out = whole[256:256 + out_bytes]
    st = hip.abf_decode(d_files, descs, W, H, out)
    torch.cuda.synchronize()
    whole = whole.cpu().numpy()
    assert (whole[:256] == CANARY).all() and (whole[256 + out_bytes:] == CANARY).all(), "written outside out"
    return st.cpu().numpy(), whole[256:256 + out_bytes]


def check_frames(out, offs, imgs, W, H, expect_ok):
    """frames with expect_ok decoded bit for bit; every byte that belongs to no frame still the canary"""
    P = W * H
    free = np.ones(len(out), bool)
    for o, img, ok in zip(offs, imgs, expect_ok):
        free[o:o + P] = False
        if ok:
            assert np.array_equal(out[o:o + P].reshape(H, W), img)
    assert (out[free] == CANARY).all(), "written into a gap"


@pytest.mark.parametrize("W", [1, 4, 63, 64, 65, 127, 130, 1280, 1680, 2050])
def test_kernel_decodes_batches_bit_for_bit(sources, W):
    for H in (1, 2, 7):
        rs = np.random.RandomState(W * 8 + H)
        imgs = mixed_frames(sources, W, H, 40, seed=W + H)
        blob, foffs = lay_out([host.abf_encode(im) for im in imgs])
        doffs, total = scattered(40, W * H, rs, odd=W % 2 == 1)
        descs = [(fo, len(host.abf_encode(im)), int(do)) for fo, im, do in zip(foffs, imgs, doffs)]
        st, out = run_decode(blob, descs, W, H, total)
        assert (st == 0).all(), (W, H, st)
        check_frames(out, doffs, imgs, W, H, [True] * 40)


def test_rows_of_more_than_64_blocks(sources):
    """W > 4096: the kernel places a row's blocks 64 at a time and carries the offset over; 65 blocks, the last of 4 pixels"""
    W, H = 4100, 1
    rs = np.random.RandomState(4100)
    imgs = mixed_frames(sources, W, H, 8, seed=41)
    files = [host.abf_encode(im) for im in imgs]
    assert all(f == abfref.encode(im) for f, im in zip(files[:3], imgs[:3]))
    blob, foffs = lay_out(files)
    doffs, total = scattered(8, W * H, rs, odd=True)
    st, out = run_decode(blob, [(fo, len(f), int(do)) for fo, f, do in zip(foffs, files, doffs)], W, H, total)
    assert (st == 0).all(), st
    check_frames(out, doffs, imgs, W, H, [True] * 8)


FAULTS = [("cut", c) for c in abfref.CUTS] + [(k, None) for k in abfref.KINDS if k != "cut"]


@pytest.mark.parametrize("W,H", [(130, 5), (65, 3), (320, 4)])
def test_damaged_files_are_refused_and_neighbours_stay_intact(sources, W, H):
    rs = np.random.RandomState(W)
    good = mixed_frames(sources, W, H, 41, seed=3 * W)
    files, imgs, want, kinds = [], [], [], []
    for i in range(40):
        files.append(abfref.encode(good[i]))
        imgs.append(good[i])
        want.append(0)
        kinds.append("intact")
        src = good[(7 * i + 3) % 41]
        # 40 files per shape: every place of a cut (8), then the six other faults five times each, then two more cuts
        fault = FAULTS[i] if i < len(FAULTS) else FAULTS[8 + (i - len(FAULTS)) % 6] if i < 38 else FAULTS[i - 38 + 6]
        kind, bad, code = abfref.damage(abfref.encode(src, extra_bits=i % 2), W, H, rs, *fault)
        files.append(bad)
        imgs.append(src)
        want.append(code)
        kinds.append(kind)
    files.append(abfref.encode(good[40], extra_bits=1))  # (non-minimal widths: accepted)
    imgs.append(good[40])
    want.append(0)
    kinds.append("intact")
    blob, foffs = lay_out(files)
    doffs, total = scattered(len(files), W * H, rs, odd=True)
    st, out = run_decode(blob, [(fo, len(f), int(do)) for fo, f, do in zip(foffs, files, doffs)], W, H, total)
    ref = [abfref.decode(f, W, H)[0] for f in files]
    for i, (s, r, w, k) in enumerate(zip(st, ref, want, kinds)):
        assert (s != 0) == (r != 0), (i, k, s, r)
        assert s == r == w, (i, k, s, r, w)  # single faults: the documented code
    assert sum(s != 0 for s in st) == 40
    assert set(kinds) == {"intact"} | {"cut:" + c for c in abfref.CUTS} | {k for k in abfref.KINDS if k != "cut"}
    check_frames(out, doffs, imgs, W, H, [s == 0 for s in st])


def test_descriptors_and_a_lying_last_file(sources):
    W, H = 130, 5
    P = W * H
    imgs = mixed_frames(sources, W, H, 6, seed=9)
    files = [host.abf_encode(im) for im in imgs]
    t0, w0, p0 = abfref.regions(W, H)
    # the last file of the buffer states a larger payload and row offsets beyond its end (its length says the truth)
    liar = bytearray(files[5])
    liar[16:20] = struct.pack("<I", len(liar) - p0 + 4096)
    for y in range(1, H):
        liar[t0 + 8 * y:t0 + 8 * y + 4] = struct.pack("<I", len(liar) + 1000 * y)
    # the same with a descriptor that repeats the lie: its length then runs beyond files_bytes
    # and one whose size is right and whose row offsets alone point past the end
    rows = bytearray(files[4])
    for y in range(1, H):
        rows[t0 + 8 * y:t0 + 8 * y + 4] = struct.pack("<I", 0x7FFFFF00 + y)
    files[4], files[5] = bytes(rows), bytes(liar)
    blob, foffs = lay_out(files)
    files_bytes = foffs[5] + len(files[5])  # the buffer ends with the last file's last byte
    out_bytes = 6 * P + 10
    descs = [(foffs[i], len(files[i]), i * P + (3 if i else 0)) for i in range(6)]
    descs[1] = (foffs[1], files_bytes - foffs[1] + 1, descs[1][2])      # off + len beyond files_bytes
    descs[2] = (foffs[2], len(files[2]), out_bytes - P + 1)             # dst + W * H beyond out_bytes
    st, out = run_decode(blob, descs, W, H, out_bytes, files_bytes=files_bytes)
    assert list(st) == [0, abfref.E_DESC, abfref.E_DESC, 0, abfref.E_ROWS, abfref.E_SIZE], st
    assert np.array_equal(out[:P].reshape(H, W), imgs[0]) and np.array_equal(out[3 * P + 3:4 * P + 3].reshape(H, W), imgs[3])
    assert (out[P:3 * P + 3] == CANARY).all() and (out[5 * P + 3:] == CANARY).all()  # frames 1, 2, 5: nothing written
    descs[5] = (foffs[5], len(files[5]) + 4096, descs[5][2])
    st, out = run_decode(blob, descs, W, H, out_bytes, files_bytes=files_bytes)
    assert st[5] == abfref.E_DESC and (out[5 * P + 3:] == CANARY).all()
    far = [(0xFFFFFFF0, 0xFFFFFFF0, 0), (0, len(files[0]), 1 << 40)]     # sums that do not fit 32 bits
    st, out = run_decode(blob, far, W, H, out_bytes, files_bytes=files_bytes)
    assert list(st) == [abfref.E_DESC] * 2 and (out == CANARY).all()


# ---- the reading path -------------------------------------------------------------------------------------------------
RUN_ID = "20200925_1"


def make_run_dir(root, W, H, F, nev, ncams=2):
    """the run of test_ingest.make_run_dir"""
    frames = {}
    rd = os.path.join(root, RUN_ID)
    for e in range(nev):
        for c in range(ncams):
            spec = synth.random_spec(W, H, F, 300 + e, c, margin=10)
            st = synth.render_event(W, H, spec, 300 + e, c)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                name = f"cam{c}_image{30 + k}.png"
                Image.fromarray(st[k]).save(os.path.join(d, name))
                frames[(e, c, name)] = st[k]
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(nev):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    os.makedirs(os.path.join(rd, "9", "Images"))
    return rd, frames


def zip_run(rd, path, compress):
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", compression=compress, allowZip64=True) as z:
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))


W4, H4, F4 = 320, 128, 20


def batched(kind, src, outdir, gpu, batch_mb=2, env=()):
    old = {k: os.environ.get(k) for k in ("ABUB_GPU_DECODE", "ABUB_GPU_DECODE_EVENTS", "ABUB_HOST_DECODE_EVENTS")}
    os.environ["ABUB_GPU_DECODE"] = "1" if gpu else "0"
    os.environ.pop("ABUB_GPU_DECODE_EVENTS", None)
    os.environ.pop("ABUB_HOST_DECODE_EVENTS", None)
    os.environ.update(dict(env))
    os.makedirs(outdir, exist_ok=True)
    run = host.Run(kind, src, "Images")
    try:
        for c in range(2):
            assert run.train(c, shape=(H4, W4))[0] == 0
        st = run.run_batched(2, outdir + "/", "r", 30, nthreads=4, decode_threads=4, batch_mb=batch_mb)
    finally:
        run.close()
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return st, open(os.path.join(outdir, "abub3hs_r.txt")).read()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A PNG run with a 16-bit PNG, a truncated file, an empty file and a frame of W + 4 among its frames, its text under
    host decode, and the repacked run with the same four faults: the 16-bit PNG as it is, the others in the packed format."""
    root = str(tmp_path_factory.mktemp("abf_runs"))
    rd, frames = make_run_dir(os.path.join(root, "png"), W4, H4, F4, nev=7)
    packed = os.path.join(root, "packed", RUN_ID)
    run = host.Run("raw", rd + "/", "Images")
    st = run.repack(packed, nthreads=4, ncams=2)
    run.close()
    assert st["packed"] == 7 * 2 * F4 and st["copied"] == 0 and st["failed"] == 0
    wide = np.zeros((H4, W4 + 4), np.uint8)
    for d, pack in ((rd, False), (packed, True)):
        d3, d4 = os.path.join(d, "3", "Images"), os.path.join(d, "4", "Images")
        Image.fromarray(frames[(3, 0, "cam0_image37.png")].astype(np.uint16) << 8).save(os.path.join(d3, "cam0_image37.png"))
        data = open(os.path.join(d3, "cam1_image40.png"), "rb").read()
        open(os.path.join(d3, "cam1_image40.png"), "wb").write(data[:len(data) // 2])
        open(os.path.join(d4, "cam0_image33.png"), "wb").close()
        if pack:
            open(os.path.join(d4, "cam1_image35.png"), "wb").write(host.abf_encode(wide))
        else:
            Image.fromarray(wide).save(os.path.join(d4, "cam1_image35.png"))
    st0, ref = batched("raw", rd + "/", os.path.join(root, "out_ref"), gpu=False)
    assert st0["frames_gpu_decoded"] == 0 and st0["frames_failed"] == 3 and len(ref.splitlines()) >= 12
    return {"root": root, "png": rd, "packed": packed, "ref": ref, "total": 7 * 2 * F4}


def test_batched_run_from_packed_directory_and_archives(runs):
    root, packed = runs["root"], runs["packed"]
    zs, zd = os.path.join(root, "stored.zip"), os.path.join(root, "deflated.zip")
    zip_run(packed, zs, zipfile.ZIP_STORED)
    zip_run(packed, zd, zipfile.ZIP_DEFLATED)
    for kind, src, tag in (("raw", packed + "/", "p_raw"), ("zip", zs, "p_stored"), ("zip", zd, "p_deflated")):
        st, text = batched(kind, src, os.path.join(root, tag), gpu=True)
        assert text == runs["ref"], tag
        assert st["frames_failed"] == 3 and st["frames_host_decoded"] == 1, (tag, st)  # the 16-bit PNG
        assert st["frames_gpu_unpacked"] == runs["total"] - 4 == st["frames_gpu_decoded"], (tag, st)
    st, text = batched("raw", packed + "/", os.path.join(root, "p_host"), gpu=False)
    assert text == runs["ref"]
    assert st["frames_gpu_decoded"] == 0 == st["frames_gpu_unpacked"] and st["frames_failed"] == 3, st


def test_batched_run_mixing_png_and_packed_frames(runs):
    root = runs["root"]
    mixed = os.path.join(root, "mixed", RUN_ID)
    shutil.copytree(runs["packed"], mixed)
    shutil.rmtree(os.path.join(mixed, "2"))
    shutil.copytree(os.path.join(runs["png"], "2"), os.path.join(mixed, "2"))  # one event left as PNG
    st, text = batched("raw", mixed + "/", os.path.join(root, "m_raw"), gpu=True)
    assert text == runs["ref"]
    assert st["frames_gpu_decoded"] == runs["total"] - 4 and st["frames_gpu_unpacked"] == runs["total"] - 4 - 2 * F4, st
    # one event per batch: batches whose GPU share is only packed frames, one whose share is only PNG frames
    st, text = batched("raw", mixed + "/", os.path.join(root, "m_one"), gpu=True, batch_mb=64, env={"ABUB_GPU_DECODE_EVENTS": "1"}.items())
    assert text == runs["ref"]
    assert st["events_per_batch"] == 1 and st["batches"] == 8, st
    assert st["frames_failed"] == 3 and st["frames_host_decoded"] == 1, st
    assert st["frames_gpu_decoded"] == runs["total"] - 4 and st["frames_gpu_unpacked"] == runs["total"] - 4 - 2 * F4, st


def test_device_training_from_a_packed_run(tmp_path):
    W, H, F, nev = 320, 128, 4, 5
    rd, _ = make_run_dir(str(tmp_path / "png"), W, H, F, nev=nev)
    packed = str(tmp_path / "packed" / RUN_ID)
    run = host.Run("raw", rd + "/", "Images")
    run.repack(packed, nthreads=4, ncams=2)
    run.close()
    dev = host.Run("raw", packed + "/", "Images")
    got = dev.train_on_gpu(2, shape=(H, W))
    assert dev.train_path == "device"
    assert dev.train_stats["frames_gpu_unpacked"] == 2 * nev * 2 == dev.train_stats["frames_gpu_decoded"], dev.train_stats
    dev.close()
    for src in (rd, packed):  # the host Trainer on the PNG run and on the packed run
        ref = host.Run("raw", src + "/", "Images")
        for c in range(2):
            st, tss, mu, sg = ref.train(c, shape=(H, W))
            assert (got[c][0], got[c][1]) == (st, tss) and st == 0
            assert np.array_equal(got[c][2], mu) and np.array_equal(got[c][3], sg)
        ref.close()


def test_cli_repack_then_analyse_gives_the_same_result_file(tmp_path):
    rd, _ = make_run_dir(str(tmp_path / "data"), W4, H4, F4, nev=3)
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
    env.pop("ABUB_GPU_DECODE", None)

    def cli(*args):
        r = subprocess.run([exe] + list(args), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    data, out = os.path.dirname(rd), str(tmp_path / "packed")
    os.makedirs(str(tmp_path / "o1"))
    os.makedirs(str(tmp_path / "o2"))
    cli("-d", data, "-r", RUN_ID, "-o", str(tmp_path / "o1"))
    cli("-d", data, "-r", RUN_ID, "--repack", out)
    cli("-d", out, "-r", RUN_ID, "-o", str(tmp_path / "o2"))
    a = open(str(tmp_path / "o1" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    b = open(str(tmp_path / "o2" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    assert a == b and len(a.splitlines()) >= 9
