"""abub_unzip_dev and the archive-entry calls of the parsers on the CPU side: the entry points are declared, exported and
bound and validate their arguments before anything touches a device; Parser::GetImageEntryInfo / ReadImageEntryRaw agree
with Python's zipfile on archives zipfile wrote (stored, deflated, local headers with an extra field, zip64 records) and on
the hand-written ones of the route tests; every stream of the GPU tests gets from zlib the verdict those tests state."""
import ctypes
import os
import zipfile
import zlib

import numpy as np
import pytest

import zipcraft as zc
from autobub3hs_amd import _lib, hip, host
from test_ingest import make_run_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


class ZipEntry(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint32), ("clen", ctypes.c_uint32), ("ulen", ctypes.c_uint32), ("crc", ctypes.c_uint32),
                ("dst", ctypes.c_uint64)]


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_unzip_dev(const uint8_t *comp, size_t comp_bytes, const abub_zip_entry *entries, int nentries," in hdr
    body = hdr.split("typedef struct abub_zip_entry {")[1].split("} abub_zip_entry;")[0]
    for field in ("uint32_t off, clen;", "uint32_t ulen, crc;", "uint64_t dst;"):
        assert field in body, field
    assert ctypes.sizeof(ZipEntry) == 24 and ZipEntry.dst.offset == 16
    codes = zc.status_codes()
    assert codes["DESC"] == 1 and codes["CRC"] == 16 and (codes["TRUNCATED"], codes["TOOLITTLE"], codes["INTERNAL"]) == (3, 12, 15)
    L = ctypes.CDLL(_lib.build())
    for name, nargs in (("abub_unzip_dev", 8), ("abub_crc32_dev", 7)):
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(hip.unzip) and callable(hip.crc32)
    H = ctypes.CDLL(host.SO)
    assert hasattr(H, "abh_run_entry_info") and hasattr(H, "abh_run_entry_raw")


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(comp=p, comp_bytes=1024, entries=p + 1024, n=1, out=p + 2048, out_bytes=1024, status=p + 3072, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_unzip_dev(a["comp"], a["comp_bytes"], a["entries"], a["n"], a["out"], a["out_bytes"], a["status"], a["stream"])

    for kw in (dict(comp=None), dict(entries=None), dict(out=None), dict(status=None), dict(n=-1), dict(n=-5, comp=None),
               dict(comp=p + 4), dict(out=p + 2048 + 8)):
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_unzip_dev" in L.abub_last_error(), kw
    for args in ((None, 64, p, 1, p, p, None), (p, 64, None, 1, p, p, None), (p, 64, p, 1, None, p, None), (p, 64, p, 1, p, None, None),
                 (p, 64, p, -1, p, p, None)):
        assert L.abub_k2_set_option(None, 0) == -1
        assert L.abub_crc32_dev(*args) == E_INVALID
        assert b"abub_crc32_dev" in L.abub_last_error()
    assert not any(buf)


def test_no_entries_is_ok_and_touches_nothing():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
    p = ctypes.addressof(buf)
    assert L.abub_unzip_dev(p, 256, p, 0, p, 256, p, None) == 0
    assert L.abub_crc32_dev(p, 256, p, 0, p, p, None) == 0
    assert bytes(buf) == bytes([0x5A]) * 256


def test_no_host_fallback():
    import torch
    c = zc.good_cases()[5]
    comp = torch.frombuffer(bytearray(zc.Batch([c]).comp), dtype=torch.uint8)
    out = torch.full((64,), 0x5A, dtype=torch.uint8)
    with pytest.raises(_lib.AbubError, match="no CPU fallback"):
        hip.unzip(comp, zc.Batch([c]).rows, out)
    with pytest.raises(_lib.AbubError, match="no CPU fallback"):
        hip.crc32(out, [[0, 0, 16, 0, 0]])
    assert bool((out == 0x5A).all())


def check_against_zipfile(path, run):
    """every frame entry of the archive: method, sizes, CRC and the compressed bytes as zipfile finds them"""
    n = 0
    with zipfile.ZipFile(path) as z, open(path, "rb") as f:
        for zi in z.infolist():
            parts = zi.filename.split("/")
            if zi.is_dir() or not parts[-1].startswith("cam"):
                continue
            info = run.entry_info(parts[1], parts[-1])
            assert info == dict(method=zi.compress_type, compress_size=zi.compress_size, file_size=zi.file_size, crc=zi.CRC), zi.filename
            f.seek(zi.header_offset)
            lh = f.read(30)
            f.seek(zi.header_offset + 30 + int.from_bytes(lh[26:28], "little") + int.from_bytes(lh[28:30], "little"))
            raw = f.read(zi.compress_size)
            assert run.entry_raw(parts[1], parts[-1]) == raw, zi.filename
            if zi.compress_type == 8:
                assert zlib.decompress(raw, -15) == z.read(zi)
            n += 1
    return n


def write_archive(rd, path, how):
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, allowZip64=True) as z:
        k = 0
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for name in sorted(fn):
                data = open(os.path.join(dp, name), "rb").read()
                zi = zipfile.ZipInfo(os.path.join(rel, name))
                zi.compress_type = {"stored": 0, "deflated": 8, "mixed": (0, 8)[k % 2]}.get(how, 8)
                if how == "extra":  # a local header with an extra field (of an unknown kind, 12 bytes)
                    zi.extra = b"\x99\x99\x08\x00abcdefgh"
                if how == "zip64":
                    with z.open(zi, "w", force_zip64=True) as dst:
                        dst.write(data)
                else:
                    z.writestr(zi, data)
                k += 1


@pytest.mark.parametrize("how", ["stored", "deflated", "mixed", "extra", "zip64"])
def test_entry_calls_agree_with_zipfile(tmp_path, how):
    rd, frames = make_run_dir(str(tmp_path), nev=2, ncams=2, F=4)
    path = str(tmp_path / (how + ".zip"))
    write_archive(rd, path, how)
    run = host.Run("zip", path, "Images")
    try:
        assert check_against_zipfile(path, run) == len(frames)
        assert run.entry_info("0", "cam0_image99.png") is None and run.entry_raw("7", "cam0_image30.png") is None
    finally:
        run.close()


def test_hand_written_archive_reads_like_one_of_zipfile(tmp_path):
    """zipcraft.write_zip, the writer of the route tests' archives, against zipfile and the parser"""
    rd, frames = make_run_dir(str(tmp_path), nev=2, ncams=1, F=3)
    root, entries = os.path.dirname(rd), []
    for dp, dn, fn in os.walk(rd):
        rel = os.path.relpath(dp, root)
        entries.append((rel + "/", b"", 0, None, None))
        for k, name in enumerate(sorted(fn)):
            entries.append((os.path.join(rel, name), open(os.path.join(dp, name), "rb").read(), (8, 0)[k % 2], None, None))
    path = str(tmp_path / "hand.zip")
    zc.write_zip(path, entries)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
    run = host.Run("zip", path, "Images")
    try:
        assert check_against_zipfile(path, run) == len(frames)
        for (e, c, name), img in frames.items():
            assert np.array_equal(run.image(e, name)[1], img)
    finally:
        run.close()


def test_a_directory_run_has_no_entries(tmp_path):
    rd, frames = make_run_dir(str(tmp_path), nev=1, ncams=1, F=2)
    raw = host.Run("raw", rd + "/", "Images")
    try:
        assert raw.entry_info("0", "cam0_image30.png") is None and raw.entry_raw("0", "cam0_image30.png") is None
        assert lib_raw(raw, "0", "cam0_image30.png") == -1
    finally:
        raw.close()


def lib_raw(run, ev, name):
    buf = np.zeros(16, np.uint8)
    return host.lib().abh_run_entry_raw(run._h, ev.encode(), name.encode(), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 16)


def test_zlib_gives_the_stated_verdict_on_every_stream():
    good, bad = zc.good_cases(), zc.refused_cases()
    assert len(good) > 200 and len(bad) >= 15
    for c in good:
        assert c.code is None and zc.zlib_verdict(c), c.name
        assert zlib.decompress(c.z, -15) == c.raw
    for c in bad:
        assert c.code is not None
        # (a descriptor refusal is about the batch's layout: its stream is a good one)
        assert zc.zlib_verdict(c) == (c.code == "DESC"), c.name
    names = {c.name for c in good}
    assert {"dist-32768-and-1", "15-bit-codes", "eob-only-blocks", "stored-after-partial-byte", "trailing-bytes", "empty-fixed"} <= names
