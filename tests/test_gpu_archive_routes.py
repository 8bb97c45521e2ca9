"""abub3hs --archive on the GPU: the archive of --repack-gpu / --unpack-gpu is byte for byte the host route's (and with it the
restatement's, tests/zipref.py) -- with one batch and with batches of 5, with forced zip64, from a directory and from a zipped
source, on a run that mixes what the decoders take with what host threads pack, and on a batch whose files outgrow their
first reservation; the batched analysis and --verify-gpu read the archive."""
import os
import zipfile

import numpy as np
import pytest
from PIL import Image

from archiveruns import RUN_ID, check_archive, cli, make_run, tree, zip_run
from autobub3hs_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the mixed run (8-bit PNGs, a 16-bit PNG that a host thread decodes inside a device batch, a packed frame, a frame of
    another size, a truncated and an empty file) as a directory and as a deflated archive; the host routes' archives"""
    root = tmp_path_factory.mktemp("gpu_archive")
    rd, frames = make_run(str(root / "data"))
    data = os.path.dirname(rd)
    zip_run(rd, os.path.join(data, RUN_ID + ".zip"), zipfile.ZIP_DEFLATED)
    out = {"rd": rd, "data": data, "root": root}
    for what in ("repack", "unpack"):
        for z in (False, True):
            d = str(root / f"host_{what}_{int(z)}")
            cli(*(["-z"] if z else []), "-d", data, "-r", RUN_ID, f"--{what}", d, "--archive")
            out[(what, z)] = open(os.path.join(d, RUN_ID + ".zip"), "rb").read()
    return out


def gpu_archive(runs, tmp_path, what, zipped=False, tag="G", **more):
    out = str(tmp_path / tag)
    r = cli(*(["-z"] if zipped else []), "-d", runs["data"], "-r", RUN_ID, f"--{what}", out, f"--{what}-gpu", "--archive", **more)
    assert sorted(os.listdir(out)) == [RUN_ID + ".zip"]
    return open(os.path.join(out, RUN_ID + ".zip"), "rb").read(), r.stdout


@pytest.mark.parametrize("what", ["repack", "unpack"])
def test_gpu_archive_is_the_host_routes(runs, tmp_path, what):
    got, text = gpu_archive(runs, tmp_path, what)
    assert got == runs[(what, False)]
    # 24 frames: 20 encoded on the GPU (the packed one decoded by the packed kernel, the others by the PNG kernel); the 16-bit
    # PNG is decoded and packed by the thread that read it inside the device batch, and so are the frame of another size, the
    # truncated and the empty file
    lines = [l for l in text.splitlines() if l.startswith(what)]
    assert f"{what}: 4 events, 22 frames" in lines[0] and "2 copied as they are, 0 not written" in lines[0], text
    assert lines[1] == f"{what}: archive {tmp_path}/G/{RUN_ID}.zip: {len(got)} bytes, {1 + 1 + 4 * 2 + 24} entries", text
    assert "20 frames encoded on GPU 0 (19 decoded by the PNG kernel, 1 by the packed kernel, 0 by a host thread), 4 took the host " \
           "route, 1 batches" in lines[2], text
    assert lines[-1].startswith(f"{what}-gpu: archive entries formed on GPU 0: pack "), text
    # segment boundaries on other residues, and with them other paddings: the same bytes
    got5, text5 = gpu_archive(runs, tmp_path, what, tag="G5", ABUB_REPACK_BATCH="5")
    assert got5 == got and "5 batches" in text5, text5
    gotz, _ = gpu_archive(runs, tmp_path, what, zipped=True, tag="GZ", ABUB_REPACK_BATCH="7")
    assert gotz == runs[(what, True)]


@pytest.mark.parametrize("what", ["repack", "unpack"])
def test_gpu_archive_with_forced_zip64(runs, tmp_path, what):
    out = str(tmp_path / "H")
    cli("-d", runs["data"], "-r", RUN_ID, f"--{what}", out, "--archive", ABUB_ZIP64_FORCE="1")
    want = open(os.path.join(out, RUN_ID + ".zip"), "rb").read()
    assert want != runs[(what, False)] and b"PK\x06\x06" in want[-200:]
    got, _ = gpu_archive(runs, tmp_path, what, ABUB_ZIP64_FORCE="1", ABUB_REPACK_BATCH="5")
    assert got == want
    d = str(tmp_path / "D")
    cli("-d", runs["data"], "-r", RUN_ID, f"--{what}", d)
    check_archive(os.path.join(str(tmp_path / "G"), RUN_ID + ".zip"), tree(d), force64=True)


def test_python_entry_on_the_device(runs, tmp_path):
    run = host.Run("raw", runs["rd"] + "/", "Images")
    try:
        sh = run.repack(str(tmp_path / "H" / RUN_ID), nthreads=3, ncams=2, archive=True)
        sg = run.repack(str(tmp_path / "G" / RUN_ID), nthreads=3, ncams=2, device=0, archive=True)
    finally:
        run.close()
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out", "archive_bytes", "archive_entries"):
        assert sh[k] == sg[k], k
    assert sg["frames_gpu_encoded"] == 20 and sg["device"] == 0 and sg["batches"] == 1 and sg["pack_s"] > 0
    assert open(str(tmp_path / "G" / (RUN_ID + ".zip")), "rb").read() == runs[("repack", False)]


def test_a_batch_that_outgrows_its_reservation_is_redone(tmp_path):
    """frames of one noise row repeated: a PNG of 224 bytes, a packed file of 6,816 (the files of a batch of 8 are more than
    twice their PNGs and the slack: the encoder's buffer grows and the call is redone, once)"""
    W, H, F = 96, 64, 6
    rs = np.random.RandomState(2)
    rd = os.path.join(str(tmp_path / "data"), RUN_ID)
    pngs = packed = 0
    for e in range(2):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d)
        for c in range(2):
            for k in range(F):
                img = np.ascontiguousarray(np.broadcast_to(rs.randint(0, 256, W).astype(np.uint8), (H, W)))
                Image.fromarray(img).save(os.path.join(d, f"cam{c}_image{30 + k}.png"))
                if e == 0 and (c == 0 or k < 2):  # the first batch of 8
                    pngs += os.path.getsize(os.path.join(d, f"cam{c}_image{30 + k}.png"))
                    packed += len(host.abf_encode(img))
    assert packed > 2 * pngs + 8192, (packed, pngs)
    open(os.path.join(rd, RUN_ID + ".txt"), "w").write("".join(f"{RUN_ID} {e} a b c d e f g h i\n" for e in range(2)))
    data = os.path.dirname(rd)
    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    cli("-d", data, "-r", RUN_ID, "--repack", a, "--archive", ABUB_REPACK_BATCH="8")
    r = cli("-d", data, "-r", RUN_ID, "--repack", b, "--repack-gpu", "--archive", ABUB_REPACK_BATCH="8")
    assert "3 batches" in r.stdout and "0 not written" in r.stdout, r.stdout
    assert open(os.path.join(a, RUN_ID + ".zip"), "rb").read() == open(os.path.join(b, RUN_ID + ".zip"), "rb").read()
    assert zipfile.ZipFile(os.path.join(b, RUN_ID + ".zip")).testzip() is None


def test_round_trip_through_the_archive(tmp_path):
    """the batched analysis with -z on the packed archive writes the result file of the source run; --verify-gpu passes on it"""
    rd, _ = make_run(str(tmp_path / "data"), W=96, H=64, F=12, mixed=False)
    data, out = os.path.dirname(rd), str(tmp_path / "P")
    r = cli("-d", data, "-r", RUN_ID, "--repack", out, "--repack-gpu", "--archive", "--verify-repack", out, "--verify-gpu")
    assert "verify: 4 events, 72 frames: 72 same, 0 same but not packed, 0 copied, 0 differ, 0 missing, 0 undecodable, 0 extra; " \
           "event file same; " in r.stdout, r.stdout
    assert "verify-gpu: 72 frames compared on GPU 0" in r.stdout, r.stdout
    for tag, args in (("oa", ["-d", data]), ("ob", ["-z", "-d", out])):
        os.makedirs(str(tmp_path / tag))
        cli(*args, "-r", RUN_ID, "-o", str(tmp_path / tag))
    ra = open(str(tmp_path / "oa" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    rb = open(str(tmp_path / "ob" / f"abub3hs_{RUN_ID}.txt"), "rb").read()
    assert ra == rb and len(ra.splitlines()) >= 3
    # the row length of a real frame, once: 1280 wide, both routes, the same archive
    rd2, _ = make_run(str(tmp_path / "wide"), W=1280, H=32, F=2, nev=1, ncams=1, mixed=False)
    wa, wb = str(tmp_path / "WA"), str(tmp_path / "WB")
    cli("-d", os.path.dirname(rd2), "-r", RUN_ID, "--unpack", wa, "--archive")
    cli("-d", os.path.dirname(rd2), "-r", RUN_ID, "--unpack", wb, "--unpack-gpu", "--archive")
    assert open(os.path.join(wa, RUN_ID + ".zip"), "rb").read() == open(os.path.join(wb, RUN_ID + ".zip"), "rb").read()
