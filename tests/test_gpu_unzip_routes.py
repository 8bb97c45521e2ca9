"""ABUB_GPU_UNZIP=1 through every route that reads files for the GPU decoders: deflated archives of PNG, packed and BMP
frames and one that mixes stored and deflated entries of all three.  With the knob on, the text, the trained model, the
repacked files and the verdicts are byte for byte those of the knob unset and of the host route (ABUB_GPU_DECODE=0), and
frames_gpu_unzipped counts every deflated entry but the broken ones: an entry whose deflate stream is cut short (the host
fails too), one whose central-directory CRC-32 is wrong (the kernel refuses it, the host's inflate does not look at the CRC)
and an empty one.  A 16-bit PNG is inflated on the GPU and decoded by a host thread.  The archives are written by hand
(zipcraft.write_zip; test_unzip_abi checks that writer against zipfile)."""
import os
import re

import numpy as np
import pytest

import bmpfiles
import zipcraft as zc
from autobub3hs_amd import host
from autobub3hs_amd import synth
from test_gpu_bmp import batched, tree
from test_ingest import make_run_dir, png_bytes

pytestmark = pytest.mark.gpu
RUN_ID = "20200925_1"
W, H, F, NEV, NCAMS = 320, 128, 20, 4, 2
TOTAL = NEV * NCAMS * F
FORMAT = "cam%d_image%u.png"
# (event, camera, frame index); the 16-bit PNG and the entry with the wrong CRC are training frames (indices 0 and 1); the
# entry cut short is frame 2, the first one the trigger search may stop at (AnalyzerUnit::minEvalFrameNumber): the search
# of its stack meets a frame that is not there before anything can trigger, so that event and camera must report -9
# (AnalyzerUnit.cpp FindTriggerFrame, "corrupted/empty"), whatever the frames show
PNG16, BAD_CRC, CUT, EMPTY = (3, 0, 1), (2, 1, 1), (1, 0, 2), (1, 1, 9)
TIMES = ("total_s", "list_s", "decode_s", "gpu_s", "write_s", "gpudecode_s", "unzip_s")


def name_of(c, k):
    return f"cam{c}_image{30 + k}.png"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """-> {tag: (path, {(e, c, k): method})}: "png", "abf", "bmp" (every entry deflated), "mixed" (format by (k + e) % 3, every
    other entry stored), "stored" (the PNG archive, stored), "whole" (mixed formats, all deflated, no entry that cannot be read:
    for repack and verify, which refuse a run with one)"""
    root = str(tmp_path_factory.mktemp("unziproutes"))
    rd, frames = make_run_dir(root, W=W, H=H, F=F, nev=NEV, ncams=NCAMS)
    enc = {"png": png_bytes, "abf": host.abf_encode, "bmp": lambda img: bmpfiles.pillow_bmp(img, "L")}
    out = {}
    for tag in ("png", "abf", "bmp", "mixed", "stored", "whole"):
        entries, methods = [(RUN_ID + "/", b"", 0, None, None)], {}
        entries.append((f"{RUN_ID}/{RUN_ID}.txt", open(os.path.join(rd, RUN_ID + ".txt"), "rb").read(), 8, None, None))
        for e in list(range(NEV)) + [9]:
            entries += [(f"{RUN_ID}/{e}/", b"", 0, None, None), (f"{RUN_ID}/{e}/Images/", b"", 0, None, None)]
        for (e, c, name), img in sorted(frames.items()):
            k = int(name.split("image")[1].split(".")[0]) - 30
            kind = ("png", "abf", "bmp")[(k + e) % 3] if tag in ("mixed", "whole") else "png" if tag == "stored" else tag
            method = 0 if tag == "stored" or (tag == "mixed" and (k + c) % 2 == 0) else 8
            data, stream, crc = enc[kind](img), None, None
            odd = tag not in ("stored",)
            if odd and (e, c, k) == PNG16:
                data, method = png_bytes(img, "I;16"), 8
            elif odd and (e, c, k) == BAD_CRC:
                crc, method = (zc.zlib.crc32(data) ^ 0x400) & 0xFFFFFFFF, 8
            elif odd and tag != "whole" and (e, c, k) == CUT:
                z = zc.deflate_raw(data, 6)
                stream, method = z[:len(z) // 2], 8
            elif odd and tag != "whole" and (e, c, k) == EMPTY:
                data, method = b"", 8
            methods[(e, c, k)] = method
            entries.append((f"{RUN_ID}/{e}/Images/{name}", data, method, stream, crc))
        path = os.path.join(root, tag + ".zip")
        zc.write_zip(path, entries)
        out[tag] = (path, methods)
    return out


def unzippable(methods, tag, keep=lambda key: True):
    """the deflated entries minus exactly the broken ones"""
    broken = {BAD_CRC} if tag == "whole" else set() if tag == "stored" else {BAD_CRC, CUT, EMPTY}
    return sum(1 for key, m in methods.items() if m == 8 and key not in broken and keep(key))


def go(src, outdir, env, monkeypatch, batch_mb=2):
    monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
    return batched("zip", src, outdir, env, monkeypatch, FORMAT, batch_mb)


def same_counters(a, b):
    for k in a:
        if k not in TIMES and k != "frames_gpu_unzipped":
            assert a[k] == b[k], (k, a, b)


@pytest.mark.parametrize("tag", ["png", "abf", "bmp", "mixed"])
def test_run_batched(archives, tmp_path, monkeypatch, tag):
    path, methods = archives[tag]
    host_st, ref = go(path, str(tmp_path / "host"), {"ABUB_GPU_DECODE": "0"}, monkeypatch)
    off_st, off = go(path, str(tmp_path / "off"), {}, monkeypatch)
    on_st, on = go(path, str(tmp_path / "on"), {"ABUB_GPU_UNZIP": "1"}, monkeypatch)
    assert on == off == ref and len(ref.splitlines()) >= 6 + NEV
    assert host_st["frames_gpu_decoded"] == 0 and host_st["frames_failed"] == 2 and host_st["frames"] == TOTAL - 2, host_st
    assert off_st["frames_gpu_unzipped"] == 0 == host_st["frames_gpu_unzipped"]
    assert on_st["frames_gpu_unzipped"] == unzippable(methods, tag) >= TOTAL // 2 - 3, on_st
    same_counters(on_st, off_st)
    # every frame but the 16-bit PNG (a host thread decodes it, wherever its file was inflated) and the two that cannot be read
    assert on_st["frames_gpu_decoded"] == TOTAL - 3 and on_st["frames_host_decoded"] == 1 and on_st["frames_failed"] == 2, on_st
    # the entry cut short: -9 for its event and camera, in the batched text and in the block the per-event loop writes
    rows = [l for l in on.splitlines(True) if l.startswith(f"r  {CUT[0]}  ")]
    assert [l for l in rows if l.startswith(f"r  {CUT[0]}  0  0  {CUT[1]}  -9  ")] and len(rows) >= NCAMS, rows
    monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
    per_event = str(tmp_path / "per_event")
    os.makedirs(per_event)
    run = host.Run("zip", path, "Images", FORMAT)
    try:
        for c in range(NCAMS):
            assert run.train(c, shape=(H, W))[0] == 0
        host.event_to_file(run, str(CUT[0]), CUT[0], NCAMS, per_event + "/", "r", 30)
    finally:
        run.close()
    assert open(os.path.join(per_event, "abub3hs_r.txt")).read() == "".join(rows)
    if tag == "png":  # the knob has no effect where the GPU decoders are off
        st, text = go(path, str(tmp_path / "nodec"), {"ABUB_GPU_DECODE": "0", "ABUB_GPU_UNZIP": "1"}, monkeypatch)
        assert text == ref and st["frames_gpu_unzipped"] == 0 and st["frames_gpu_decoded"] == 0, st


def test_stored_archive_has_nothing_to_inflate(archives, tmp_path, monkeypatch):
    path, methods = archives["stored"]
    off_st, off = go(path, str(tmp_path / "off"), {}, monkeypatch)
    on_st, on = go(path, str(tmp_path / "on"), {"ABUB_GPU_UNZIP": "1"}, monkeypatch)
    assert on == off and on_st["frames_gpu_unzipped"] == 0 and on_st["frames_gpu_decoded"] == TOTAL, on_st
    same_counters(on_st, off_st)


def test_a_batch_with_a_host_share(archives, tmp_path, monkeypatch):
    path, methods = archives["mixed"]
    env = {"ABUB_GPU_DECODE_EVENTS": "1", "ABUB_HOST_DECODE_EVENTS": "1"}
    off_st, off = go(path, str(tmp_path / "off"), env, monkeypatch, batch_mb=64)
    on_st, on = go(path, str(tmp_path / "on"), dict(env, ABUB_GPU_UNZIP="1"), monkeypatch, batch_mb=64)
    assert on == off and on_st["events_per_batch"] == 2 and on_st["batches"] == 3, on_st
    # (events 0 .. 3 and the frame-less 9 in batches of a GPU event and a host event: the GPU's are 0, 2 and 9)
    assert on_st["frames_gpu_unzipped"] == unzippable(methods, "mixed", lambda key: key[0] in (0, 2)) >= 20, on_st
    assert off_st["frames_gpu_unzipped"] == 0
    same_counters(on_st, off_st)


def test_two_batches(archives, tmp_path, monkeypatch):
    path, methods = archives["mixed"]
    env = {"ABUB_GPU_DECODE_EVENTS": "3"}
    off_st, off = go(path, str(tmp_path / "off"), env, monkeypatch, batch_mb=64)
    on_st, on = go(path, str(tmp_path / "on"), dict(env, ABUB_GPU_UNZIP="1"), monkeypatch, batch_mb=64)
    assert on == off and on_st["events_per_batch"] == 3 and on_st["batches"] == 2, on_st
    assert on_st["frames_gpu_unzipped"] == unzippable(methods, "mixed") and off_st["frames_gpu_unzipped"] == 0, on_st
    same_counters(on_st, off_st)


@pytest.mark.parametrize("tag", ["mixed", "png"])
def test_train_on_device(archives, monkeypatch, tag):
    """two runs trained on the device one after the other, each against the host Trainer and against the knob unset"""
    path, methods = archives[tag]
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    got = {}
    for knob in (None, "1"):
        monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
        if knob:
            monkeypatch.setenv("ABUB_GPU_UNZIP", knob)
        dev = host.Run("zip", path, "Images", FORMAT)
        try:
            got[knob] = (dev.train_on_gpu(NCAMS, shape=(H, W)), dev.train_stats)
            assert dev.train_path == "device"
        finally:
            dev.close()
    ref = host.Run("zip", path, "Images", FORMAT)
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
    assert off["frames_gpu_unzipped"] == 0
    assert on["frames_gpu_unzipped"] == unzippable(methods, tag, lambda key: key[2] < 2) >= 6, on
    for k in off:
        if k not in ("seconds", "frames_gpu_unzipped"):
            assert off[k] == on[k], (k, off, on)


def test_repack_gpu_from_a_deflated_archive(archives, tmp_path, monkeypatch):
    path, methods = archives["whole"]
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.setenv("ABUB_REPACK_BATCH", "64")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
    run = host.Run("zip", path, "Images", FORMAT)
    try:
        sh = run.repack(str(tmp_path / "host" / RUN_ID), nthreads=4, ncams=NCAMS)
        soff = run.repack(str(tmp_path / "off" / RUN_ID), nthreads=4, ncams=NCAMS, device=0)
        monkeypatch.setenv("ABUB_GPU_UNZIP", "1")
        son = run.repack(str(tmp_path / "on" / RUN_ID), nthreads=4, ncams=NCAMS, device=0)
    finally:
        run.close()
    th, toff, ton = tree(str(tmp_path / "host")), tree(str(tmp_path / "off")), tree(str(tmp_path / "on"))
    assert sorted(th) == sorted(ton) == sorted(toff) and len(th) >= TOTAL
    for name in th:  # file by file against the host repack
        assert th[name] == ton[name] == toff[name], name
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sh[k] == son[k] == soff[k], (k, sh, son)
    assert son["batches"] == 3 and soff["frames_gpu_unzipped"] == 0, son
    assert son["frames_gpu_unzipped"] == unzippable(methods, "whole") == TOTAL - 1, son
    for k in soff:
        if not k.endswith("_s") and k not in ("seconds", "frames_gpu_unzipped"):
            assert soff[k] == son[k], (k, soff, son)


def test_verify_gpu_with_a_deflated_archive_as_the_source(archives, tmp_path, monkeypatch):
    path, methods = archives["whole"]
    monkeypatch.setenv("ABUB_GPU_BMP", "1")
    monkeypatch.setenv("ABUB_VERIFY_BATCH", "64")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
    out = str(tmp_path / "packed" / RUN_ID)
    src = host.Run("zip", path, "Images", FORMAT)
    try:
        src.repack(out, nthreads=4, ncams=NCAMS)
        victim = os.path.join(out, "1", "Images", name_of(1, 4))
        data = bytearray(host.abf_decode(open(victim, "rb").read(), W, H)[1])
        data[3 * W + 12] ^= 0x40
        open(victim, "wb").write(host.abf_encode(np.frombuffer(bytes(data), np.uint8).reshape(H, W)))
        other = host.Run("raw", out + "/", "Images", FORMAT)
        try:
            vh = src.verify(other, nthreads=4, ncams=NCAMS)
            voff = src.verify(other, nthreads=4, ncams=NCAMS, device=0)
            monkeypatch.setenv("ABUB_GPU_UNZIP", "1")
            von = src.verify(other, nthreads=4, ncams=NCAMS, device=0)
        finally:
            other.close()
    finally:
        src.close()
    for k in ("rc", "events", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra", "event_file",
              "findings"):
        assert vh[k] == von[k] == voff[k], (k, vh[k], von[k])
    assert von["rc"] == 1 and von["differ"] == 1 and von["frames"] == TOTAL and von["same"] == TOTAL - 1, von
    assert von["device"] == 0 and von["batches"] == 3, von
    assert voff["src_gpu_unzipped"] == 0 == voff["other_gpu_unzipped"] == von["other_gpu_unzipped"], voff
    assert von["src_gpu_unzipped"] == unzippable(methods, "whole") == TOTAL - 1 == von["frames_gpu_unzipped"], von
    for k in voff:
        if not k.endswith("_s") and k not in ("seconds", "src_gpu_unzipped", "frames_gpu_unzipped"):
            assert voff[k] == von[k], (k, voff[k], von[k])


def test_verify_gpu_when_only_one_side_waits_for_the_inflate(tmp_path, monkeypatch):
    """A deflated archive verified against a plain directory in batches of three: only the source side of a pair waits for
    the device's inflate, so the second reading round meets pairs whose other side is already final -- read and on its way
    to a decoder, or read and refused (a frame of another size).  A frame the directory lacks is never read on either side
    (its archive entry is stored, so that every deflated entry is one the kernel inflates).  Verdicts and findings are the
    host route's."""
    w, h, nev, nf = 64, 16, 2, 4
    missing, resized, changed = (0, 1), (1, 0), (1, 2)  # (event, frame): tasks 1, 4 and 6 of batches [0-2], [3-5], [6-7]
    r = np.random.RandomState(18)
    other_root = str(tmp_path / "dir" / RUN_ID)
    listing = "".join(f"{RUN_ID} {e} a b c d e f g h i\n" for e in range(nev)).encode()
    entries = [(RUN_ID + "/", b"", 0, None, None), (f"{RUN_ID}/{RUN_ID}.txt", listing, 8, None, None)]
    deflated = 0
    for e in range(nev):
        entries += [(f"{RUN_ID}/{e}/", b"", 0, None, None), (f"{RUN_ID}/{e}/Images/", b"", 0, None, None)]
        os.makedirs(os.path.join(other_root, str(e), "Images"))
        for k in range(nf):
            img = np.sort(r.randint(0, 256, (h, w)), axis=1).astype(np.uint8)
            method = 0 if (e, k) == missing else 8
            deflated += method == 8
            entries.append((f"{RUN_ID}/{e}/Images/{name_of(0, k)}", png_bytes(img), method, None, None))
            if (e, k) == missing:
                continue
            if (e, k) == resized:
                img = img[:, :w - 4]
            elif (e, k) == changed:
                img = img.copy()
                img[5, 9] ^= 0x10
            open(os.path.join(other_root, str(e), "Images", name_of(0, k)), "wb").write(png_bytes(img))
    open(os.path.join(other_root, RUN_ID + ".txt"), "wb").write(listing)
    zc.write_zip(str(tmp_path / "src.zip"), entries)
    monkeypatch.setenv("ABUB_VERIFY_BATCH", "3")
    monkeypatch.delenv("ABUB_GPU_DECODE", raising=False)
    monkeypatch.delenv("ABUB_GPU_UNZIP", raising=False)
    src = host.Run("zip", str(tmp_path / "src.zip"), "Images", FORMAT)
    other = host.Run("raw", other_root + "/", "Images", FORMAT)
    try:
        vh = src.verify(other, nthreads=4, ncams=1)
        monkeypatch.setenv("ABUB_GPU_UNZIP", "1")
        von = src.verify(other, nthreads=4, ncams=1, device=0)
    finally:
        other.close()
        src.close()
    for k in ("rc", "events", "frames", "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra", "event_file",
              "findings"):
        assert vh[k] == von[k], (k, vh[k], von[k])
    assert (von["rc"], von["frames"], von["missing"], von["differ"], von["same_not_packed"]) == (1, nev * nf, 1, 2, nev * nf - 3), von
    assert [(f["event"], f["name"]) for f in von["findings"] if f["verdict"] in ("missing", "differ")] == [
        (str(e), name_of(0, k)) for e, k in (missing, resized, changed)], von["findings"]
    assert von["device"] == 0 and von["batches"] == 3, von
    assert von["src_gpu_unzipped"] == deflated == nev * nf - 1 and von["other_gpu_unzipped"] == 0, von


def test_campaign_of_two_deflated_archives(tmp_path):
    """abub3hs --runs A,B -z (abub::RunCampaign): one FileBatch with its GpuUnzip is kept from run to run for the device
    training, and run B is trained on a thread and stream of its own while run A's batches pass through the look-ahead
    thread's GpuUnzip.  Every run's file with the knob on is the file with it unset and the file of ABUB_GPU_DECODE=0; the
    campaign's line counts the entries inflated for the detect and for the training (frames 0 and 1 of every stack)."""
    ids = ["20200925_0", "20200925_1"]
    data = str(tmp_path / "data")
    os.makedirs(data)
    expect_detect = expect_train = 0
    for r, rid in enumerate(ids):
        entries = [(rid + "/", b"", 0, None, None)]
        for e in range(NEV):
            entries += [(f"{rid}/{e}/", b"", 0, None, None), (f"{rid}/{e}/Images/", b"", 0, None, None)]
            for c in range(NCAMS):
                st = synth.render_event(W, H, synth.random_spec(W, H, F, 700 + 10 * r + e, c, margin=10), 700 + 10 * r + e, c)
                for k in range(F):
                    data_k = png_bytes(st[k]) if (k + e) % 2 else host.abf_encode(st[k])
                    stream = crc = None
                    good = True
                    if r == 0 and (e, c, k) == PNG16:
                        data_k = png_bytes(st[k], "I;16")
                    elif r == 0 and (e, c, k) == BAD_CRC:
                        crc, good = (zc.zlib.crc32(data_k) ^ 0x400) & 0xFFFFFFFF, False
                    elif r == 1 and (e, c, k) == CUT:
                        z = zc.deflate_raw(data_k, 6)
                        stream, good = z[:len(z) // 2], False
                    elif r == 1 and (e, c, k) == EMPTY:
                        data_k, good = b"", False
                    expect_detect += good
                    expect_train += good and k < 2
                    entries.append((f"{rid}/{e}/Images/{name_of(c, k)}", data_k, 8, stream, crc))
        zc.write_zip(os.path.join(data, rid + ".zip"), entries)
    texts, outs = {}, {}
    for tag, env in (("host", {"ABUB_GPU_DECODE": "0"}), ("off", {}), ("on", {"ABUB_GPU_UNZIP": "1"})):
        out = str(tmp_path / ("out_" + tag))
        os.makedirs(out)
        e = {k: v for k, v in os.environ.items() if k not in ("ABUB_GPU_UNZIP", "ABUB_GPU_DECODE", "ABUB_GPU_BMP", "ABUB_TRAIN_ON_GPU")}
        e.update({"ABUB_THREADS": "4", "ABUB_NUM_CAMS": "2"}, **env)
        p = run_cli_env(["-z", "-d", data, "--runs", ",".join(ids), "-o", out, "-D", "40l-19"], e)
        assert p.returncode == 0 and p.stdout.count("batched detect:") == 2, (tag, p.stdout[-3000:], p.stderr[-3000:])
        assert "device training not used" not in p.stdout, p.stdout[-3000:]
        texts[tag] = [open(os.path.join(out, f"abub3hs_{rid}.txt")).read() for rid in ids]
        outs[tag] = p.stdout
    assert texts["on"] == texts["off"] == texts["host"] and texts["on"][0] != texts["on"][1]
    assert f"{ids[1]}  {CUT[0]}  0  0  {CUT[1]}  -9  " in texts["on"][1]
    assert "archive entries inflated" not in outs["off"] and "archive entries inflated" not in outs["host"]
    m = re.search(r"campaign: (\d+) archive entries inflated on the GPU for the detect, (\d+) for the training", outs["on"])
    assert m and (int(m.group(1)), int(m.group(2))) == (expect_detect, expect_train) == (2 * TOTAL - 3, 4 * NEV * NCAMS - 1), outs["on"][-2000:]


def run_cli_env(args, env):
    """test_cli.run_cli with exactly this environment (that helper adds to os.environ)"""
    import subprocess

    from test_cli import EXE
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=env, timeout=300)
