"""One small run that holds every frame format the GPU decoders take -- 8-bit grey PNG, packed ("ABF1") and BMP (with
ABUB_GPU_BMP=1) -- through every route that reads files for them: RunBatched, TrainOnDevice, --repack-gpu / --unpack-gpu and
--verify-gpu.  Each route must give what its host route gives, byte for byte, and count every frame once, under the
decoder that took it.  Among the frames: a 16-bit PNG (the walk refuses it, the reading thread decodes it), a frame of
another size, a PNG whose deflate stream has a flipped byte behind an intact header (the walk accepts it, the kernel and
the host decoder refuse it) and a packed frame cut off behind a valid header.  The batch knobs are set so that RunBatched,
repack, unpack and verify take three batches each, every one with frames for all three decoders.  TrainOnDevice has no
such knob: it decodes that run's sixteen training frames in one launch, so a second run of many two-frame events of a tiny
size gives it more GPU frames than one launch takes (4 per CU) and the irregular frames in the second launch."""
import os

import numpy as np
import pytest

import abfref
import bmpfiles
from autobub3hs_amd import host
from test_gpu_bmp import batched, tree
from test_ingest import make_run_dir, png_bytes
from test_verify_repack import bumped

pytestmark = pytest.mark.gpu
RUN_ID = "20200925_1"
W, H, F, NEV, NCAMS = 320, 128, 20, 4, 2
TOTAL = NEV * NCAMS * F
FORMAT = "cam%d_image%u.png"
# (event, camera, frame index): the 16-bit PNG and the damaged PNG are training frames (indices 0 and 1)
PNG16, BAD_PNG, BAD_ABF, OTHER_SIZE = (3, 0, 1), (3, 1, 0), (1, 0, 6), (2, 1, 7)


def name_of(c, k):
    return f"cam{c}_image{30 + k}.png"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """-> (run dir, frames, kinds): frame k of event e is a PNG, a packed or a BMP file by (k + e) % 3, whatever its name"""
    root = str(tmp_path_factory.mktemp("mixed"))
    rd, frames = make_run_dir(root, W=W, H=H, F=F, nev=NEV, ncams=NCAMS)
    kinds = {}
    for (e, c, name), img in frames.items():
        k = int(name.split("image")[1].split(".")[0]) - 30
        kind = ("png", "abf", "bmp")[(k + e) % 3]
        data = {"png": lambda: png_bytes(img), "abf": lambda: host.abf_encode(img), "bmp": lambda: bmpfiles.pillow_bmp(img, "L")}[kind]()
        if (e, c, k) == PNG16:
            kind, data = "png16", png_bytes(img, "I;16")
        elif (e, c, k) == OTHER_SIZE:
            kind, data = "size", png_bytes(np.zeros((H, W + 4), np.uint8))
        elif (e, c, k) == BAD_PNG:
            assert kind == "png"
            at = data.index(b"IDAT") + 4
            n = int.from_bytes(data[at - 8:at - 4], "big")
            data = bytearray(data)
            data[at + n // 2] ^= 0x10  # in the middle of the deflate stream
            kind, data = "badpng", bytes(data)
            assert host.png_walk(data, W, H) is not None and host.imdecode(data) is None
        elif (e, c, k) == BAD_ABF:
            assert kind == "abf"
            kind, data = "badabf", data[:len(data) // 2]
            assert len(data) > 32 + 8 * H and host.imdecode(data) is None and host.abf_decode(data, W, H)[0] != 0
        kinds[(e, c, k)] = kind
        open(os.path.join(rd, str(e), "Images", name), "wb").write(data)
    first = frames[(0, 0, name_of(0, 1))]
    assert host.abf_encode(first) == abfref.encode(first)  # (the packed files are the reference encoder's)
    assert sorted(set(kinds.values())) == ["abf", "badabf", "badpng", "bmp", "png", "png16", "size"]
    return rd, frames, kinds


def count(kinds, kind, keep=lambda key: True):
    return sum(1 for key, v in kinds.items() if v == kind and keep(key))


def test_run_batched(mixed, tmp_path, monkeypatch):
    rd, _, kinds = mixed
    ref_st, ref = batched("raw", rd + "/", str(tmp_path / "host"), {"ABUB_GPU_DECODE": "0"}, monkeypatch, FORMAT)
    assert ref_st["frames_gpu_decoded"] == 0 and ref_st["frames_failed"] == 3 and ref_st["frames"] == TOTAL - 3
    st, text = batched("raw", rd + "/", str(tmp_path / "gpu"), {"ABUB_GPU_DECODE_EVENTS": "2"}, monkeypatch, FORMAT, batch_mb=64)
    assert text == ref and len(ref.splitlines()) >= 6 + NEV
    assert st["events_per_batch"] == 2 and st["batches"] == 3, st  # (five event directories: 0..3 and the frame-less 9)
    # (these stats have no PNG field: the sum holds by construction, the comparison with the run's own counts is the pin)
    png = st["frames_gpu_decoded"] - st["frames_gpu_unpacked"] - st["frames_gpu_bmp"]
    assert (png, st["frames_gpu_unpacked"], st["frames_gpu_bmp"]) == (count(kinds, "png"), count(kinds, "abf"), count(kinds, "bmp")), st
    assert min(png, st["frames_gpu_unpacked"], st["frames_gpu_bmp"]) >= 1 and st["frames_gpu_decoded"] == TOTAL - 4, st
    assert st["frames_failed"] == 3 and st["frames_host_decoded"] == 1 and st["frames"] == TOTAL - 3, st


def train_both(rd, monkeypatch, shape):
    """TrainOnDevice against the host Trainer, camera by camera -> (the device route's stats, the training set sizes)"""
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    dev = host.Run("raw", rd + "/", "Images", FORMAT)
    got = dev.train_on_gpu(NCAMS, shape=shape)
    st = dev.train_stats
    dev.close()
    assert dev.train_path == "device"
    ref = host.Run("raw", rd + "/", "Images", FORMAT)
    for c in range(NCAMS):
        rst, tss, mu, sg = ref.train(c, shape=shape)
        assert (got[c][0], got[c][1]) == (rst, tss) and rst == 0 and tss >= 2, (c, got[c][:2], rst, tss)
        assert np.array_equal(got[c][2], mu) and np.array_equal(got[c][3], sg), c
    ref.close()
    return st, [g[1] for g in got]


def test_train_on_device(mixed, monkeypatch):
    rd, _, kinds = mixed
    st, _ = train_both(rd, monkeypatch, (H, W))
    trained = lambda key: key[2] < 2
    # (no PNG field here either: see test_run_batched)
    png = st["frames_gpu_decoded"] - st["frames_gpu_unpacked"] - st["frames_gpu_bmp"]
    assert (png, st["frames_gpu_unpacked"], st["frames_gpu_bmp"]) == \
        (count(kinds, "png", trained), count(kinds, "abf", trained), count(kinds, "bmp", trained)), st
    assert min(png, st["frames_gpu_unpacked"], st["frames_gpu_bmp"]) >= 1, st
    assert st["frames_gpu_decoded"] == 2 * NEV * NCAMS - 2 and st["frames_host_decoded"] == 1 and st["decode_launches"] == 1, st


def test_train_on_device_in_two_launches(tmp_path, monkeypatch):
    """A launch takes at most 4 frames per CU, 1024 on an MI355X: 540 events of two cameras give 2160 training frames in the
    three formats, tasks in camera, event and frame order, so the second launch starts inside camera 0 and the third inside
    camera 1.  The 16-bit PNG, the damaged PNG and the cut packed frame lie behind the first launch."""
    w, h, nev = 32, 16, 540
    png16, bad_png, bad_abf = (530, 1, 1), (531, 1, 0), (532, 1, 1)  # (camera 1: behind the first launch in any event order)
    rs = np.random.RandomState(7)
    rd = str(tmp_path / RUN_ID)
    n = {"png": 0, "abf": 0, "bmp": 0}
    for e in range(nev):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d)
        for c in range(NCAMS):
            img = rs.randint(0, 256, (h, w)).astype(np.uint8)  # (both frames of a pair alike: the veto keeps it)
            for k in range(2):
                kind = ("png", "abf", "bmp")[(k + e + c) % 3]
                if (e, c, k) == png16:
                    data = png_bytes(img, "I;16")
                elif (e, c, k) == bad_png:
                    data = bytearray(png_bytes(img))
                    at = data.index(b"IDAT") + 4
                    data[at + int.from_bytes(data[at - 8:at - 4], "big") // 2] ^= 0x10
                    assert host.png_walk(bytes(data), w, h) is not None and host.imdecode(bytes(data)) is None
                elif (e, c, k) == bad_abf:
                    data = host.abf_encode(img)[:32 + 8 * h + 4]
                    assert host.imdecode(data) is None
                else:
                    data = {"png": png_bytes, "abf": host.abf_encode, "bmp": lambda i: bmpfiles.pillow_bmp(i, "L")}[kind](img)
                    n[kind] += 1
                open(os.path.join(d, name_of(c, k)), "wb").write(data)
    st, tss = train_both(rd, monkeypatch, (h, w))
    assert tss == [2 * nev, 2 * (nev - 2)], tss  # (the two damaged frames drop their events of camera 1)
    png = st["frames_gpu_decoded"] - st["frames_gpu_unpacked"] - st["frames_gpu_bmp"]
    assert (png, st["frames_gpu_unpacked"], st["frames_gpu_bmp"]) == (n["png"], n["abf"], n["bmp"]) and min(n.values()) > 342, (st, n)
    assert st["frames_gpu_decoded"] == 2 * nev * NCAMS - 3 and st["frames_host_decoded"] == 1, st
    assert st["decode_launches"] >= 2, st


def both(run_dir, op, a, b):
    """Run.repack / Run.unpack of run_dir on the host into a, on the GPU into b -> the device route's stats"""
    run = host.Run("raw", run_dir + "/", "Images", FORMAT)
    try:
        sh = getattr(run, op)(a, nthreads=4, ncams=NCAMS)
        sd = getattr(run, op)(b, nthreads=4, ncams=NCAMS, device=0)
    finally:
        run.close()
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sh[k] == sd[k], (op, k, sh, sd)
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb) and len(ta) == TOTAL + 1
    for name in ta:
        assert ta[name] == tb[name], (op, name)
    return sd


def test_repack_then_unpack(mixed, tmp_path, monkeypatch):
    rd, _, kinds = mixed
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.setenv("ABUB_REPACK_BATCH", "64")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    for op in ("repack", "unpack"):  # of the mixed run: all three decoders in every batch
        sd = both(rd, op, str(tmp_path / (op + "_host") / RUN_ID), str(tmp_path / (op + "_dev") / RUN_ID))
        assert sd["batches"] == 3 and sd["packed"] == TOTAL - 2 and sd["copied"] == 2 and sd["failed"] == 0, sd
        got = (sd["frames_gpu_png_decoded"], sd["frames_gpu_unpacked"], sd["frames_gpu_bmp_decoded"])
        assert got == (count(kinds, "png"), count(kinds, "abf"), count(kinds, "bmp")) and min(got) >= 1, sd
        # the decoders were given every frame but the 16-bit PNG and the frame of another size; they refused two
        assert sum(got) + sd["frames_host_decoded"] == TOTAL - 2 - 2 == sd["frames_gpu_encoded"] and sd["frames_host_decoded"] == 0, sd
        assert sd["frames_host_route"] == 4, sd
    # ... and the way back from the repacked run
    sd = both(str(tmp_path / "repack_dev" / RUN_ID), "unpack", str(tmp_path / "back_host" / RUN_ID), str(tmp_path / "back_dev" / RUN_ID))
    # (the two damaged files were copied as they are, and the frame of another size is a packed frame of another size)
    assert sd["batches"] == 3 and sd["frames_gpu_unpacked"] == TOTAL - 3 == sd["frames_gpu_encoded"] and sd["copied"] == 2, sd
    assert sd["frames_host_route"] == 3, sd
    assert sd["frames_gpu_png_decoded"] == 0 == sd["frames_gpu_bmp_decoded"] and sd["frames_host_decoded"] == 0, sd


def test_verify(mixed, tmp_path, monkeypatch):
    rd, frames, kinds = mixed
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.setenv("ABUB_VERIFY_BATCH", "64")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    out = str(tmp_path / "packed" / RUN_ID)
    run = host.Run("raw", rd + "/", "Images", FORMAT)
    try:
        run.repack(out, nthreads=4, ncams=NCAMS)
    finally:
        run.close()
    # the copy tampered with: a PNG and a BMP among its packed files, one pixel moved, one file gone
    as_png, as_bmp, moved, gone = (0, 0, 3), (0, 1, 5), (1, 1, 4), (2, 0, 9)
    path = lambda key: os.path.join(out, str(key[0]), "Images", name_of(*key[1:]))
    img = lambda key: frames[(key[0], key[1], name_of(*key[1:]))]
    open(path(as_png), "wb").write(png_bytes(img(as_png)))
    open(path(as_bmp), "wb").write(bmpfiles.pillow_bmp(img(as_bmp), "L"))
    open(path(moved), "wb").write(host.abf_encode(bumped(img(moved), [(12, 3, 5)])))
    os.remove(path(gone))
    src, other = host.Run("raw", rd + "/", "Images", FORMAT), host.Run("raw", out + "/", "Images", FORMAT)
    try:
        vh = src.verify(other, nthreads=4, ncams=NCAMS)
        vd = src.verify(other, nthreads=4, ncams=NCAMS, device=0)
    finally:
        src.close()
        other.close()
    for k in ("rc", "events", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra", "event_file",
              "findings"):
        assert vh[k] == vd[k], (k, vh[k], vd[k])
    assert [(f["event"], f["name"], f["verdict"]) for f in vd["findings"]] == \
        [("0", name_of(0, 3), "same_not_packed"), ("0", name_of(1, 5), "same_not_packed"), ("1", name_of(1, 4), "differ"),
         ("2", name_of(0, 9), "missing")], vd["findings"]
    assert vd["findings"][2]["ndiff"] == 1 and (vd["findings"][2]["x"], vd["findings"][2]["y"]) == (12, 3)
    assert vd["rc"] == 1 and vd["frames"] == TOTAL and vd["copied"] == 2 and vd["same"] == TOTAL - 6, vd
    assert vh["device"] == -1 and vd["device"] == 0 and vd["batches"] == 3, vd
    # both sides were given every frame but the one of another size and the one the copy lacks; each side's kernels refused
    # the two damaged files, which the host route then found to be copies
    given = TOTAL - 2
    assert vd["frames_kernel"] == given - 2 and vd["frames_host_route"] == 4, vd
    there = lambda key: key != gone
    s = (vd["src_gpu_png_decoded"], vd["src_gpu_unpacked"], vd["src_gpu_bmp_decoded"])
    assert s == (count(kinds, "png", there), count(kinds, "abf", there), count(kinds, "bmp", there)) and min(s) >= 1, vd
    assert sum(s) + vd["src_host_decoded"] == given - 2 and vd["src_host_decoded"] == 1, vd
    o = (vd["other_gpu_png_decoded"], vd["other_gpu_unpacked"], vd["other_gpu_bmp_decoded"])
    assert o == (1, given - 4, 1) and sum(o) + vd["other_host_decoded"] == given - 2 and vd["other_host_decoded"] == 0, vd
