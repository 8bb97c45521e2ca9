"""abub3hs --archive on the CPU: the host writer of the canonical archive against its restatement (tests/zipref.py), byte for
byte; --repack / --unpack / --verify-repack with --archive on a directory source and on a zipped one; what a failed run
leaves behind; the refusals of the command line; and abub_zip_pack_dev as far as it goes without a device."""
import ctypes
import os
import stat
import zipfile

import numpy as np
import pytest
import torch

import zipref
from archiveruns import RUN_ID, check_archive, check_same_run, cli, make_run, tree, zip_run
from autobub3hs_amd import _lib, hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
LENGTHS = (0, 1, 15, 16, 17, 70001)
NAME_LENGTHS = (1, 2, 3, 4, 17, 255)


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def writer_cases():
    """Every length with every name length, twice, and every padding case p = 0 .. 15: in front of the k-th entry that has
    data, empty entries with names of three bytes (33 bytes each: the offset moves by 1 modulo 16) steer its p to k mod 16."""
    rs = np.random.RandomState(7)

    def name(m, directory=False):
        raw = bytes(rs.randint(97, 123, m).astype(np.uint8))
        return raw[:-1] + b"/" if directory else raw

    entries = [(name(m, m == 4), b"") for m in NAME_LENGTHS]
    off, k = sum(30 + len(n) for n, _ in entries), 0
    for _ in range(2):
        for n in LENGTHS[1:]:
            for m in NAME_LENGTHS:
                while -(off + 30 + m) % 16 != k % 16:
                    entries.append((name(3), b""))
                    off += 33
                entries.append((name(m), bytes(rs.randint(0, 256, n).astype(np.uint8))))
                off += 30 + m + zipref.extra_len(off, m, n) + n
                k += 1
    return entries


def test_the_cases_cover_every_padding():
    entries = writer_cases()
    lay = zipref.layout(entries)
    seen = {-(off + 30 + len(n)) % 16 for (n, d), (off, xl) in zip(entries, lay) if d}
    assert seen == set(range(16))
    assert {xl for _, xl in lay} == {0, 17, 18, 19} | set(range(4, 16))
    assert {(len(n), len(d)) for n, d in entries} >= {(m, n) for m in NAME_LENGTHS for n in LENGTHS}


@pytest.mark.parametrize("force64", [False, True])
def test_host_writer_writes_the_reference_bytes(tmp_path, monkeypatch, force64):
    if force64:
        monkeypatch.setenv("ABUB_ZIP64_FORCE", "1")
    else:
        monkeypatch.delenv("ABUB_ZIP64_FORCE", raising=False)
    entries = writer_cases()
    path = str(tmp_path / "w.zip")
    host.zip_write(path, entries)
    got = open(path, "rb").read()
    assert got == zipref.archive(entries, force64=force64)
    assert not os.path.exists(path + ".part")
    assert (b"PK\x06\x06" in got) == force64 and (b"PK\x06\x07" in got[-42:]) == force64
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert [i.filename.encode() for i in z.infolist()] == [n for n, _ in entries]
        for info, (n, d) in zip(z.infolist(), entries):
            assert z.read(info) == d
            assert not d or (info.header_offset + 30 + len(n) + zipref.extra_len(info.header_offset, len(n), len(d))) % 16 == 0


def test_host_writer_turns_to_zip64_at_65535_entries(tmp_path, monkeypatch):
    monkeypatch.delenv("ABUB_ZIP64_FORCE", raising=False)
    for count, z64 in ((65534, False), (65536, True)):
        entries = [(b"e/%07d" % i, b"") for i in range(count)]
        path = str(tmp_path / f"n{count}.zip")
        host.zip_write(path, entries)
        got = open(path, "rb").read()
        assert got == zipref.archive(entries)
        assert (b"PK\x06\x06" in got[-120:]) == z64
        with zipfile.ZipFile(path) as z:
            assert len(z.namelist()) == count and z.namelist()[-1] == "e/%07d" % (count - 1)


def test_host_writer_leaves_nothing_behind_when_it_fails(tmp_path):
    old = tmp_path / "keep.zip"
    host.zip_write(str(old), [(b"a", b"1")])
    before = old.read_bytes()
    with pytest.raises(RuntimeError, match="too long"):
        host.zip_write(str(old), [(b"ok", b"1"), (b"n" * 65536, b"")])
    assert old.read_bytes() == before and not os.path.exists(str(old) + ".part")
    with pytest.raises(RuntimeError, match="cannot write"):
        host.zip_write(str(tmp_path / "no" / "such" / "dir.zip"), [(b"a", b"1")])
    assert sorted(os.listdir(tmp_path)) == ["keep.zip"]


# ---- the routes ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the mixed run as a directory and as a stored archive, and what the directory routes write from the directory"""
    root = tmp_path_factory.mktemp("archive")
    rd, frames = make_run(str(root / "data"))
    data = os.path.dirname(rd)
    zip_run(rd, os.path.join(data, RUN_ID + ".zip"))
    out = {"rd": rd, "data": data, "root": root, "frames": frames}
    for what in ("repack", "unpack"):
        d = str(root / f"dir_{what}")
        cli("-d", data, "-r", RUN_ID, f"--{what}", d)
        out[what] = d
    return out


@pytest.mark.parametrize("what", ["repack", "unpack"])
@pytest.mark.parametrize("zipped", [False, True])
def test_archive_holds_the_files_of_the_directory_route(runs, tmp_path, what, zipped):
    out = str(tmp_path / "A")
    r = cli(*(["-z"] if zipped else []), "-d", runs["data"], "-r", RUN_ID, f"--{what}", out, "--archive")
    zpath = os.path.join(out, RUN_ID + ".zip")
    assert sorted(os.listdir(out)) == [RUN_ID + ".zip"]
    want = tree(runs[what])
    if zipped:  # (the directory route from the zipped source: its event file is of its own making)
        d = str(tmp_path / "D")
        cli("-z", "-d", runs["data"], "-r", RUN_ID, f"--{what}", d)
        assert {k: v for k, v in tree(d).items() if not k.endswith(".txt")} == {k: v for k, v in want.items() if not k.endswith(".txt")}
        want = tree(d)
    entries = check_archive(zpath, want)
    assert len(entries) == 1 + 1 + 4 * 2 + 24
    word = "written as PNG" if what == "unpack" else "packed"
    assert f"{what}: 4 events, 22 frames {word}" in r.stdout and "2 copied as they are, 0 not written" in r.stdout, r.stdout
    assert f"{what}: archive {out}/{RUN_ID}.zip: {os.path.getsize(zpath)} bytes, {len(entries)} entries\n" in r.stdout, r.stdout
    by_name = dict(entries)
    key = f"{RUN_ID}/1/Images/".encode()
    assert by_name[key + b"cam1_image32.png"] == open(os.path.join(runs["rd"], "1", "Images", "cam1_image32.png"), "rb").read()
    assert by_name[f"{RUN_ID}/{RUN_ID}.txt".encode()] == want[f"{RUN_ID}/{RUN_ID}.txt"]
    check_same_run(zpath, os.path.join(runs[what], RUN_ID))


def test_python_entry_and_a_row_of_1280(tmp_path, monkeypatch):
    monkeypatch.delenv("ABUB_ZIP64_FORCE", raising=False)
    rd, _ = make_run(str(tmp_path / "data"), W=1280, H=32, F=2, nev=1, ncams=1, mixed=False)
    run = host.Run("raw", rd + "/", "Images")
    try:
        sd = run.repack(str(tmp_path / "D" / RUN_ID), nthreads=2, ncams=2)
        sa = run.repack(str(tmp_path / "A" / RUN_ID), nthreads=2, ncams=2, archive=True)
        su = run.unpack(str(tmp_path / "U" / RUN_ID), nthreads=2, ncams=2, archive=True)
    finally:
        run.close()
    for k in ("packed", "copied", "failed", "bytes_in", "bytes_out"):
        assert sd[k] == sa[k], k
    assert sa["packed"] == su["packed"] == 2 and sa["archive_entries"] == 1 + 1 + 2 * 2 + 2
    assert sa["archive_bytes"] == os.path.getsize(str(tmp_path / "A" / (RUN_ID + ".zip")))
    with zipfile.ZipFile(str(tmp_path / "A" / (RUN_ID + ".zip"))) as z:
        want = tree(str(tmp_path / "D"))
        assert z.testzip() is None and {n: z.read(n) for n in z.namelist() if not n.endswith("/")} == want
    with zipfile.ZipFile(str(tmp_path / "U" / (RUN_ID + ".zip"))) as z:
        assert z.read(f"{RUN_ID}/0/Images/cam0_image30.png")[:4] == b"\x89PNG"


# ---- verify ------------------------------------------------------------------------------------------------------------------
def test_verify_reads_the_archive(runs, tmp_path):
    out = str(tmp_path / "A")
    r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", out, "--archive", "--verify-repack", out)
    assert "verify: 4 events, 24 frames: 22 same, 0 same but not packed, 2 copied, 0 differ, 0 missing, 0 undecodable, 0 extra; " \
           "event file same; " in r.stdout, r.stdout
    r = cli("-d", runs["data"], "-r", RUN_ID, "--verify-repack", out, "--archive")
    assert "22 same" in r.stdout and "event file same" in r.stdout and not [l for l in r.stdout.splitlines() if "differ:" in l]
    # the zipped source against the same archive: the event file is the source's own entry
    r = cli("-z", "-d", runs["data"], "-r", RUN_ID, "--verify-repack", out, "--archive")
    assert "22 same" in r.stdout and "event file same" in r.stdout, r.stdout
    # without --archive the copy is looked for as a directory, which is not there
    r = cli("-d", runs["data"], "-r", RUN_ID, "--verify-repack", out, ok=False)
    assert r.returncode != 0

    # one pixel of one frame changed inside the archive (the entry packed again, the archive still canonical)
    zpath = os.path.join(out, RUN_ID + ".zip")
    with zipfile.ZipFile(zpath) as z:
        entries = [(n.encode(), z.read(n)) for n in z.namelist()]
    assert zipref.archive(entries) == open(zpath, "rb").read()
    victim = f"{RUN_ID}/2/Images/cam1_image31.png".encode()
    img = runs["frames"][(2, 1, "cam1_image31.png")].copy()
    img[5, 21] = img[5, 21] + 6 if img[5, 21] < 128 else img[5, 21] - 6
    bad = str(tmp_path / "B")
    os.makedirs(bad)
    open(os.path.join(bad, RUN_ID + ".zip"), "wb").write(
        zipref.archive([(n, host.abf_encode(img) if n == victim else d) for n, d in entries]))
    r = cli("-d", runs["data"], "-r", RUN_ID, "--verify-repack", bad, "--archive", ok=False)
    assert r.returncode == 1, r.stdout + r.stderr
    found = [l for l in r.stdout.splitlines() if l.startswith("verify: ") and " events, " not in l]
    assert found == ["verify: 2/cam1_image31.png: differ: 1 pixels, first at (x=21, y=5), max |a-b| = 6"], r.stdout
    assert "21 same" in r.stdout and "1 differ" in r.stdout and "event file same" in r.stdout
    # the Python entry, and an event file that differs
    text = f"{RUN_ID}/{RUN_ID}.txt".encode()
    open(os.path.join(bad, RUN_ID + ".zip"), "wb").write(zipref.archive([(n, d + b"x" if n == text else d) for n, d in entries]))
    a, b = host.Run("raw", runs["rd"] + "/", "Images"), host.Run("zip", os.path.join(bad, RUN_ID + ".zip"), "Images")
    try:
        res = a.verify(b, nthreads=2, ncams=2, archive=True)
    finally:
        a.close()
        b.close()
    assert res["rc"] == 1 and res["same"] == 22 and res["event_file"] == "differs"
    assert [f["verdict"] for f in res["findings"]] == ["event_file_differs"]


# ---- failures ----------------------------------------------------------------------------------------------------------------
def test_a_failed_run_leaves_no_archive_and_keeps_an_older_one(runs, tmp_path):
    # a target that cannot be a directory
    blocked = tmp_path / "file"
    blocked.write_bytes(b"x")
    r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", str(blocked / "sub"), "--archive", ok=False)
    assert r.returncode != 0 and "repack failed" in r.stderr, r.stderr
    assert blocked.read_bytes() == b"x"
    # a directory that cannot be written
    locked = tmp_path / "locked"
    locked.mkdir()
    older = locked / (RUN_ID + ".zip")
    older.write_bytes(b"an older archive")
    os.chmod(locked, stat.S_IRUSR | stat.S_IXUSR)
    try:
        if not os.access(str(locked), os.W_OK):  # (a user who may write everywhere cannot be shown this)
            r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", str(locked), "--archive", ok=False)
            assert r.returncode != 0 and "repack failed" in r.stderr, r.stderr
    finally:
        os.chmod(locked, stat.S_IRWXU)
    assert sorted(os.listdir(locked)) == [RUN_ID + ".zip"] and older.read_bytes() == b"an older archive"
    # the .part file cannot be opened (its name is taken by a directory): the older archive stays, nothing else appears
    taken = tmp_path / "taken"
    (taken / (RUN_ID + ".zip.part")).mkdir(parents=True)
    (taken / (RUN_ID + ".zip")).write_bytes(b"an older archive")
    r = cli("-d", runs["data"], "-r", RUN_ID, "--unpack", str(taken), "--archive", ok=False)
    assert r.returncode != 0 and "unpack failed" in r.stderr, r.stderr
    assert sorted(os.listdir(taken)) == [RUN_ID + ".zip", RUN_ID + ".zip.part"] and os.listdir(taken / (RUN_ID + ".zip.part")) == []
    assert (taken / (RUN_ID + ".zip")).read_bytes() == b"an older archive"
    # a run that succeeds replaces the older archive, and leaves no .part
    os.rmdir(taken / (RUN_ID + ".zip.part"))
    cli("-d", runs["data"], "-r", RUN_ID, "--unpack", str(taken), "--archive")
    assert sorted(os.listdir(taken)) == [RUN_ID + ".zip"]
    assert zipfile.ZipFile(str(taken / (RUN_ID + ".zip"))).testzip() is None


def test_a_zipped_run_is_not_repacked_into_its_own_archive(runs):
    src = os.path.join(runs["data"], RUN_ID + ".zip")
    before = open(src, "rb").read()
    for target in (runs["data"], runs["data"] + "/./"):
        r = cli("-z", "-d", runs["data"], "-r", RUN_ID, "--repack", target, "--archive", ok=False)
        assert r.returncode != 0 and "is the run that is being read" in r.stderr, r.stderr
    assert open(src, "rb").read() == before and not os.path.exists(src + ".part")
    run = host.Run("zip", src, "Images")
    try:
        with pytest.raises(RuntimeError, match="is the run that is being read"):
            run.repack(os.path.join(runs["data"], RUN_ID), nthreads=2, ncams=2, archive=True)
    finally:
        run.close()
    assert open(src, "rb").read() == before
    # the directory source next to it may be archived there, as long as no archive of that name is being read: here one is
    # in the way, and it is replaced only by a complete archive
    cli("-d", runs["data"], "-r", RUN_ID, "--repack", str(runs["root"] / "side"), "--archive")
    assert zipfile.ZipFile(str(runs["root"] / "side" / (RUN_ID + ".zip"))).testzip() is None


# ---- the command line and the ABI --------------------------------------------------------------------------------------------
def test_cli_refusals_and_usage(runs, tmp_path):
    r = cli("-h", ok=False)
    assert "--archive" in r.stdout and "--repack out_data_dir [--repack-gpu] [--archive]" in r.stdout
    assert "--unpack out_data_dir [--unpack-gpu] [--archive]" in r.stdout
    assert "--verify-repack other_data_dir [--verify-gpu] [--archive]" in r.stdout
    r = cli("-d", runs["data"], "-r", RUN_ID, "-o", tmp_path, "--archive", ok=False)
    assert r.returncode != 0 and "--archive is valid only together with --repack, --unpack or --verify-repack" in r.stderr
    r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", tmp_path / "x", "--unpack", tmp_path / "x", "--archive", ok=False)
    assert r.returncode != 0 and "--unpack cannot be combined with --repack" in r.stderr
    r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", tmp_path / "x", "--archive", "--verify-repack", tmp_path / "y", ok=False)
    assert r.returncode != 0 and "must name the same directory" in r.stderr
    for extra in (["--merge", "2"], ["--runs", "a,b"], ["--gpu-shard", "0/2"], ["-e", "1"]):
        r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", tmp_path / "x", "--archive", *extra, ok=False)
        assert r.returncode != 0 and "--repack cannot be combined" in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "x"))
    if not torch.cuda.is_available():  # no silent fall-back to the host route
        r = cli("-d", runs["data"], "-r", RUN_ID, "--repack", tmp_path / "g", "--repack-gpu", "--archive", ok=False)
        assert r.returncode != 0 and "no such HIP device" in r.stderr, r.stdout + r.stderr
        assert not os.path.exists(str(tmp_path / "g" / (RUN_ID + ".zip"))) and not os.path.exists(str(tmp_path / "g" / (RUN_ID + ".zip.part")))


def test_packer_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_zip_pack_dev(" in hdr and "typedef struct abub_zip_item {" in hdr and "#define ABUB_ZIP_PACK_TILE 65536" in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_zip_pack_dev") and "abub_zip_pack_dev" in _lib.SIGNATURES
    assert callable(hip.zip_pack)
    for name in ("abh_run_repack_archive", "abh_run_verify_archive", "abh_zip_write"):
        assert name in host.SIGNATURES and hasattr(host.lib(), name)


def test_packer_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p += -p % 16
    ok = dict(buf=p, buf_bytes=1024, items=p + 1024, nitems=1, names=p + 2048, names_bytes=16, seg=p + 2560, seg_bytes=1024,
              crc=p + 2064, status=p + 2068, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_zip_pack_dev(a["buf"], a["buf_bytes"], a["items"], a["nitems"], a["names"], a["names_bytes"], a["seg"],
                                   a["seg_bytes"], a["crc"], a["status"], a["stream"])

    bad = [dict(buf=None), dict(items=None), dict(names=None), dict(seg=None), dict(crc=None), dict(status=None), dict(nitems=-1),
           dict(buf=p + 8), dict(seg=p + 2568), dict(items=p + 1028), dict(crc=p + 2066), dict(status=p + 2070)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_zip_pack_dev" in L.abub_last_error(), kw
    assert call(nitems=0) == 0  # nothing to do, nothing touched
    assert not any(buf)
    if not torch.cuda.is_available():  # no fall-back without a device: a CPU tensor is refused, a launch fails
        t = torch.zeros(64, dtype=torch.uint8)
        with pytest.raises(_lib.AbubError):
            hip.zip_pack(t, [(0, 0, 0, 0, 1, 0)], t, t)
