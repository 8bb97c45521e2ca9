"""ABUB_GPU_PNG_ADAM7=1 in the five device reading routes: a run whose frames are Adam7-interlaced 8-bit grey PNGs, with an
interlaced RGB 8, an interlaced 16-bit grey, an interlaced 2-bit grey, a non-interlaced frame and a truncated file among them,
read from a directory, a stored archive and a deflated archive.  With the knob on (and ABUB_GPU_PNG_TYPES=1 for the three
typed frames) every frame but the truncated one is decoded by the PNG kernels and no host thread decodes any; with it off
(the default) the interlaced frames are decoded by the host threads, whose decoder reads them.  Results never depend on the
knob: RunBatched's text, the trained model, the repacked files and the verdicts of verify are those of the host route, and the
text is that of the same run written without interlace.  The files come from tests/pngadam7.py (random filter types per pass
row)."""
import os
import zipfile

import numpy as np
import pytest

import pngadam7 as a7
import pngtypes as pt
from autobub3hs_amd import host, synth
from test_ingest import zip_run

pytestmark = pytest.mark.gpu

W, H, F, NEV, NCAMS = 320, 128, 20, 4, 2
TOTAL = NEV * NCAMS * F
RUN_ID = "20200925_1"
KNOBS = ("ABUB_GPU_DECODE", "ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE_EVENTS",
         "ABUB_HOST_DECODE_EVENTS", "ABUB_REPACK_BATCH", "ABUB_VERIFY_BATCH")
ON = {"ABUB_GPU_PNG_ADAM7": "1", "ABUB_GPU_PNG_TYPES": "1"}
# (event, camera, frame index).  The non-interlaced frame is the run's first (RunBatched's probe takes it knob or no knob);
# frames 0 and 1 of every event are training frames: the non-interlaced, the RGB and the 16-bit frame are among them, the
# 2-bit frame (a quarter of the grey levels) and the truncated file are not
PLAIN, RGB8, GREY16, GREY2, CUT = (0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 1, 5), (1, 1, 7)
INTERLACED = TOTAL - 2  # every frame but the non-interlaced one and the truncated one
TYPED = 3


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def frame_file(key, img, rs, interlaced=True):
    """the file of frame `key`; interlaced=False: the same samples written without interlace"""
    grey = img.astype(np.uint16)
    if key == RGB8:
        s, ctype, depth = np.repeat(grey[:, :, None], 3, axis=2), 2, 8
    elif key == GREY16:
        s, ctype, depth = (grey << 8)[:, :, None] | rs.randint(0, 256, (H, W, 1)).astype(np.uint16), 0, 16
    elif key == GREY2:
        s, ctype, depth = (grey >> 6)[:, :, None], 0, 2
    else:
        s, ctype, depth = grey[:, :, None], 0, 8
    fts = [rs.randint(0, 5, H) for _ in range(7)]
    data = a7.make_adam7(s, ctype, depth, fts) if interlaced and key != PLAIN else pt.make_png(s, ctype, depth, fts[6])
    return data[:len(data) // 2] if key == CUT else data


def write_run(root, interlaced=True, first_interlaced=False):
    rd = os.path.join(root, RUN_ID)
    rs = np.random.RandomState(6)
    for e in range(NEV):
        for c in range(NCAMS):
            spec = synth.random_spec(W, H, F, 300 + e, c, margin=10)
            st = synth.render_event(W, H, spec, 300 + e, c)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                key = (e, c, k) if not (first_interlaced and (e, c, k) == PLAIN) else None
                data = frame_file(key, st[k], rs, interlaced)
                if (e, c, k) not in (CUT, GREY2):  # (two bits keep a quarter of the grey levels)
                    assert np.array_equal(host.imdecode(data), st[k])
                open(os.path.join(d, f"cam{c}_image{30 + k}.png"), "wb").write(data)
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(NEV):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd


@pytest.fixture(scope="module")
def adam7_run(tmp_path_factory):
    """-> {"raw": (kind, source), "stored": ..., "deflated": ...}"""
    root = str(tmp_path_factory.mktemp("adam7"))
    rd = write_run(root)
    zs, zd = os.path.join(root, "stored.zip"), os.path.join(root, "deflated.zip")
    zip_run(rd, zs, zipfile.ZIP_STORED)
    zip_run(rd, zd, zipfile.ZIP_DEFLATED)
    return {"raw": ("raw", rd + "/"), "stored": ("zip", zs), "deflated": ("zip", zd)}


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def batched(source, outdir, env, monkeypatch):
    set_env(monkeypatch, env)
    os.makedirs(outdir, exist_ok=True)
    run = host.Run(source[0], source[1], "Images")
    try:
        for c in range(NCAMS):
            assert run.train(c, shape=(H, W))[0] == 0
        st = run.run_batched(NCAMS, outdir + "/", "r", 30, nthreads=4, decode_threads=4, batch_mb=2)
    finally:
        run.close()
    return st, open(os.path.join(outdir, "abub3hs_r.txt")).read()


@pytest.fixture(scope="module")
def reference(adam7_run, tmp_path_factory):
    """the text of the run with every frame decoded by host threads"""
    mp = pytest.MonkeyPatch()
    try:
        st, text = batched(adam7_run["raw"], str(tmp_path_factory.mktemp("ref")), {"ABUB_GPU_DECODE": "0"}, mp)
    finally:
        mp.undo()
    assert st["frames_gpu_decoded"] == 0 and st["frames_failed"] == 1 and st["frames"] == TOTAL - 1, st
    assert len(text.splitlines()) >= 6 + NEV
    return text


@pytest.mark.parametrize("source,unzip", [("raw", False), ("stored", False), ("deflated", False), ("deflated", True)])
def test_batched_run_with_the_knob_on(adam7_run, reference, tmp_path, monkeypatch, source, unzip):
    env = dict(ON, **({"ABUB_GPU_UNZIP": "1"} if unzip else {}))
    st, text = batched(adam7_run[source], str(tmp_path / "on"), env, monkeypatch)
    assert text == reference
    assert st["frames_host_decoded"] == 0 and st["frames_gpu_decoded"] == TOTAL - 1 and st["frames_failed"] == 1, st
    assert st["frames_gpu_unpacked"] == 0 and st["frames_gpu_bmp"] == 0, st
    assert (st["frames_gpu_unzipped"] > TOTAL // 2) == unzip, st


def test_batched_run_with_the_knob_on_without_the_typed_one(adam7_run, reference, tmp_path, monkeypatch):
    """the interlaced 8-bit frames on the GPU, the three interlaced frames of other types on host threads"""
    st, text = batched(adam7_run["raw"], str(tmp_path / "a7"), {"ABUB_GPU_PNG_ADAM7": "1"}, monkeypatch)
    assert text == reference
    assert st["frames_host_decoded"] == TYPED and st["frames_gpu_decoded"] == TOTAL - 1 - TYPED and st["frames_failed"] == 1, st


@pytest.mark.parametrize("value", [None, "0"])
def test_batched_run_with_the_knob_off(adam7_run, reference, tmp_path, monkeypatch, value):
    """the non-interlaced frame on the GPU, the interlaced frames on host threads"""
    env = {"ABUB_GPU_PNG_TYPES": "1"} if value is None else {"ABUB_GPU_PNG_ADAM7": value, "ABUB_GPU_PNG_TYPES": "1"}
    st, text = batched(adam7_run["raw"], str(tmp_path / "off"), env, monkeypatch)
    assert text == reference
    assert st["frames_gpu_decoded"] == 1 and st["frames_host_decoded"] == INTERLACED and st["frames_failed"] == 1, st


def test_the_probe_takes_an_interlaced_first_frame_with_the_knob(reference, tmp_path, monkeypatch):
    """the same run with its first frame interlaced too: RunBatched's probe decides by that frame"""
    rd = write_run(str(tmp_path / "src"), first_interlaced=True)
    st, text = batched(("raw", rd + "/"), str(tmp_path / "on"), ON, monkeypatch)
    assert text == reference
    assert st["frames_host_decoded"] == 0 and st["frames_gpu_decoded"] == TOTAL - 1 and st["frames_failed"] == 1, st
    st, text = batched(("raw", rd + "/"), str(tmp_path / "off"), {}, monkeypatch)
    assert text == reference
    assert st["frames_gpu_decoded"] == 0 and st["frames_failed"] == 1, st  # (no device decode: the probe refused)


def test_the_run_written_without_interlace_gives_the_same_text(reference, tmp_path, monkeypatch):
    rd = write_run(str(tmp_path / "src"), interlaced=False)
    st, text = batched(("raw", rd + "/"), str(tmp_path / "plain"), {"ABUB_GPU_DECODE": "0"}, monkeypatch)
    assert text == reference
    assert st["frames_failed"] == 1 and st["frames"] == TOTAL - 1, st


def test_train_on_device(adam7_run, monkeypatch):
    ntrain = 2 * NEV * NCAMS
    got = {}
    for knob in (None, "1"):
        set_env(monkeypatch, {} if knob is None else ON)
        dev = host.Run("zip", adam7_run["deflated"][1], "Images")
        try:
            got[knob] = (dev.train_on_gpu(NCAMS, shape=(H, W)), dev.train_stats)
            assert dev.train_path == "device"
        finally:
            dev.close()
    ref = host.Run("zip", adam7_run["deflated"][1], "Images")
    try:
        for c in range(NCAMS):
            rst, tss, mu, sg = ref.train(c, shape=(H, W))
            for knob in (None, "1"):
                g = got[knob][0][c]
                assert (g[0], g[1]) == (rst, tss) and rst == 0, (knob, c, g[:2], rst, tss)
                assert np.array_equal(g[2], mu) and np.array_equal(g[3], sg), (knob, c)
    finally:
        ref.close()
    off, on = got[None][1], got["1"][1]
    assert on["frames_gpu_decoded"] == ntrain and on["frames_host_decoded"] == 0, on
    assert off["frames_gpu_decoded"] == 1 and off["frames_host_decoded"] == ntrain - 1, off


def tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def test_repack_gpu_and_verify_gpu(adam7_run, tmp_path, monkeypatch):
    set_env(monkeypatch, {"ABUB_REPACK_BATCH": "64", "ABUB_VERIFY_BATCH": "64"})
    a, b, c = (str(tmp_path / t / RUN_ID) for t in ("host", "off", "on"))
    run = host.Run(*adam7_run["stored"], "Images")
    try:
        sh = run.repack(a, nthreads=4, ncams=NCAMS)
        soff = run.repack(b, nthreads=4, ncams=NCAMS, device=0)
        for k, v in ON.items():
            monkeypatch.setenv(k, v)
        son = run.repack(c, nthreads=4, ncams=NCAMS, device=0)
    finally:
        run.close()
    th, toff, ton = tree(a), tree(b), tree(c)
    assert sorted(th) == sorted(toff) == sorted(ton) and len(th) == TOTAL + 1
    for name in th:  # file by file against the host repack
        assert th[name] == ton[name] == toff[name], name
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sh[k] == son[k] == soff[k], (k, sh, son)
    assert son["packed"] == TOTAL - 1 and son["copied"] == 1, son
    # (a frame its reading thread decodes is packed by that thread too: it never reaches the device and counts in
    # frames_host_route, with the truncated file)
    assert son["frames_gpu_png_decoded"] == son["frames_gpu_encoded"] == TOTAL - 1 and son["frames_host_decoded"] == 0, son
    assert soff["frames_gpu_png_decoded"] == soff["frames_gpu_encoded"] == 1 and soff["frames_host_route"] == son["frames_host_route"] + INTERLACED, soff
    # verify: the source against its repacked copy, with one pixel of one frame changed
    victim = os.path.join(c, "2", "Images", "cam0_image34.png")
    data = bytearray(host.abf_decode(open(victim, "rb").read(), W, H)[1])
    data[3 * W + 12] ^= 0x40
    open(victim, "wb").write(host.abf_encode(np.frombuffer(bytes(data), np.uint8).reshape(H, W)))
    src, other = host.Run(*adam7_run["stored"], "Images"), host.Run("raw", c + "/", "Images")
    try:
        vh = src.verify(other, nthreads=4, ncams=NCAMS)
        von = src.verify(other, nthreads=4, ncams=NCAMS, device=0)
        for k in ON:
            monkeypatch.delenv(k)
        voff = src.verify(other, nthreads=4, ncams=NCAMS, device=0)
    finally:
        src.close()
        other.close()
    for k in ("rc", "events", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra", "event_file",
              "findings"):
        assert vh[k] == von[k] == voff[k], (k, vh[k], von[k], voff[k])
    assert von["rc"] == 1 and von["differ"] == 1 and von["frames"] == TOTAL and von["same"] == TOTAL - 2 and von["copied"] == 1, von
    assert von["src_gpu_png_decoded"] == TOTAL - 1 and von["src_host_decoded"] == 0, von
    assert voff["src_gpu_png_decoded"] == 1 and voff["src_host_decoded"] == INTERLACED, voff
