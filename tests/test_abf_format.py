"""The packed frame format "ABF1" on the CPU: the host codec (host/abf.cpp) against the numpy restatement of the format
(tests/abfref.py), the magic sniffed by imdecode and the parsers, damaged files, the C-ABI entry, and abub3hs --repack."""
import ctypes
import os
import subprocess
import zipfile

import numpy as np
import pytest
from PIL import Image

import abfref
from autobub3hs_amd import _lib, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1), (1, 3), (63, 2), (64, 2), (65, 3), (130, 2), (257, 1), (1280, 4), (2050, 2)]  # W x H


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def sources():
    """the sample frame of the reference's data and a synthetic event frame, cropped (tiled where too small) per shape"""
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = synth.render_event(320, 128, spec, 300, 0)[spec.F - 1]
    return {"sample": sample, "synth": np.ascontiguousarray(frame)}


def crop(img, W, H, x0=0, y0=0):
    img = img[y0:, x0:]
    reps = (-(-H // img.shape[0]), -(-W // img.shape[1]))
    return np.ascontiguousarray(np.tile(img, reps)[:H, :W])


def all_contents(sources, W, H, seed=0):
    out = abfref.contents(W, H, seed)
    out["sample"] = crop(sources["sample"], W, H, 700, 400)
    out["synth"] = crop(sources["synth"], W, H)
    return out


@pytest.mark.parametrize("W,H", SHAPES)
def test_host_encoder_writes_the_reference_bytes_and_decodes_them(sources, W, H):
    for name, img in all_contents(sources, W, H, seed=W).items():
        ref = abfref.encode(img)
        got = host.abf_encode(img)
        assert got == ref, (name, len(got), len(ref))
        rc, back = host.abf_decode(got, W, H)
        assert rc == 0 and np.array_equal(back, img), name
        rc, back = abfref.decode(got, W, H)
        assert rc == 0 and np.array_equal(back, img), name
    z = abfref.encode(np.zeros((H, W), np.uint8))
    assert len(z) == abfref.regions(W, H)[2] + H * ((W + 63) // 64)  # b = 0: one byte per block


@pytest.mark.parametrize("W,H", SHAPES)
def test_imdecode_reads_packed_frames_also_with_wider_widths(sources, W, H):
    for name, img in all_contents(sources, W, H, seed=W + 1).items():
        got = host.imdecode(host.abf_encode(img), cap=1 << 23)
        assert got is not None and got.shape == (H, W) and np.array_equal(got, img), name
        wide = abfref.encode(img, extra_bits=1)  # non-minimal widths are accepted
        if name not in ("random",):
            assert wide != abfref.encode(img) or W == 1, name
        got = host.imdecode(wide, cap=1 << 23)
        assert got is not None and np.array_equal(got, img), name
        assert host.abf_decode(wide, W, H)[0] == 0


def test_host_decoder_refuses_what_the_reference_refuses(sources):
    """200 damaged files (and 20 intact controls): every kind of fault, and for the cuts every place of abfref.CUTS, on every
    shape -- the plan below is fixed, only which width, row, bit or payload byte is hit comes from the seed"""
    rs = np.random.RandomState(77)
    shapes = [(1, 3), (63, 2), (65, 3), (130, 5), (320, 4)]
    faults = [("cut", c) for c in abfref.CUTS] + [(k, None) for k in abfref.KINDS if k != "cut"]  # 8 + 6 = 14
    plan = [(s, f) for s in shapes for f in faults]                                           # 70: each fault on each shape
    plan = (plan * 3)[:200]
    plan += [(shapes[i % len(shapes)], ("intact", None)) for i in range(20)]
    seen, refused = set(), 0
    for i, ((W, H), (kind, cut)) in enumerate(plan):
        imgs = all_contents(sources, W, H, seed=i)
        img = imgs[sorted(imgs)[i % len(imgs)]]
        data = abfref.encode(img, extra_bits=(i // 7) % 2)
        if kind == "intact":
            name, bad, want = "intact", data, 0
        else:
            name, bad, want = abfref.damage(data, W, H, rs, kind, cut)
        seen.add(((W, H), name))
        ref, _ = abfref.decode(bad, W, H)
        got, pix = host.abf_decode(bad, W, H)
        assert (got != 0) == (ref != 0), (i, name, W, H, got, ref)
        assert got == ref == want, (i, name, W, H, got, ref, want)
        dec = host.imdecode(bad)
        if name == "w4":  # imdecode has no expected size: a header of W + 4 that is consistent in itself (all-equal blocks,
            assert dec is None or dec.shape == (H, W + 4), (i, name)  # same nblk) is an image of that other size
        else:
            assert (dec is None) == (ref != 0), (i, name)
        if ref == 0:
            assert np.array_equal(pix, img) and np.array_equal(dec, img)
        refused += ref != 0
    assert refused == 200
    names = ["cut:" + c for c in abfref.CUTS] + [k for k in abfref.KINDS if k != "cut"]
    assert all((s, n) in seen for s in shapes for n in names), sorted(seen)


def test_size_never_exceeds_header_tables_and_pixels():
    rs = np.random.RandomState(5)
    for W, H in SHAPES + [(64, 64), (200, 33)]:
        img = rs.randint(0, 256, (H, W)).astype(np.uint8)
        n = len(host.abf_encode(img))
        assert n <= abfref.regions(W, H)[2] + W * H, (W, H, n)
    # b = 8 everywhere: exactly that bound
    img = np.tile(np.array([0, 128], np.uint8), (3, 64))
    assert len(host.abf_encode(img)) == abfref.regions(128, 3)[2] + 128 * 3


def test_abf_decode_dev_is_declared_exported_bound_and_validates_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_abf_decode_dev(" in hdr and "typedef struct abub_abf_frame" in hdr
    for code, name in enumerate(("DESC", "HEADER", "SIZE", "WIDTH", "ROWS", "CHECK"), 1):
        assert f"#define ABUB_ABF_E_{name} {code} " in hdr
    assert "abub_abf_decode_dev" in _lib.SIGNATURES
    from autobub3hs_amd import hip

    assert callable(hip.abf_decode)
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    E_INVALID = -1
    ok = dict(files=p, files_bytes=64, frames=p, nframes=1, W=8, H=2, out=p, out_bytes=64, status=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_abf_decode_dev(a["files"], a["files_bytes"], a["frames"], a["nframes"], a["W"], a["H"], a["out"],
                                     a["out_bytes"], a["status"], a["stream"])

    for bad in (dict(files=None), dict(frames=None), dict(out=None), dict(status=None), dict(nframes=-1), dict(W=0), dict(H=0),
                dict(W=65536), dict(H=65536), dict(W=-4)):
        assert call(**bad) == E_INVALID, bad
        assert b"abub_abf_decode_dev" in L.abub_last_error()
    assert call(nframes=0) == 0  # nothing to do, nothing touched


def make_packed_run(root, W=96, H=64, F=6, nev=2, ncams=2):
    run_id = "20200925_1"
    rd = os.path.join(root, run_id)
    frames = {}
    for e in range(nev):
        for c in range(ncams):
            spec = synth.random_spec(W, H, F, 300 + e, c, margin=10)
            st = synth.render_event(W, H, spec, 300 + e, c)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                name = f"cam{c}_image{30 + k}.png"
                open(os.path.join(d, name), "wb").write(host.abf_encode(st[k]))
                frames[(e, c, name)] = st[k]
    with open(os.path.join(rd, run_id + ".txt"), "w") as f:
        for e in range(nev):
            f.write(f"{run_id} {e} a b c d e f g h i\n")
    return rd, frames


def zip_run(rd, path, compress):
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", compression=compress, allowZip64=True) as z:
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))


def test_parsers_read_a_run_of_packed_frames(tmp_path):
    rd, frames = make_packed_run(str(tmp_path))
    zs, zd = os.path.join(str(tmp_path), "s.zip"), os.path.join(str(tmp_path), "d.zip")
    zip_run(rd, zs, zipfile.ZIP_STORED)
    zip_run(rd, zd, zipfile.ZIP_DEFLATED)
    for kind, src in (("raw", rd + "/"), ("zip", zs), ("zip", zd)):
        run = host.Run(kind, src, "Images")
        assert run.events() == ["0", "1"]
        for (e, c, name), img in frames.items():
            assert name in run.frames(e, c)
            rc, got = run.image(e, name)
            assert rc == 1 and np.array_equal(got, img), (kind, src, e, name)
        run.close()


def make_run_dir(root, W=96, H=64, F=12, nev=3, ncams=2):
    """the run of test_ingest.make_run_dir: PNG frames, a run file, and an event directory the run file does not list"""
    frames = {}
    run_id = "20200925_1"
    rd = os.path.join(root, run_id)
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
    with open(os.path.join(rd, run_id + ".txt"), "w") as f:
        for e in range(nev):
            f.write(f"{run_id} {e} a b c d e f g h i\n")
    os.makedirs(os.path.join(rd, "9", "Images"))
    return rd, frames


def check_repacked(src_kind, src, out_rd, frames, truncated):
    a, b = host.Run(src_kind, src, "Images"), host.Run("raw", out_rd + "/", "Images")
    try:
        assert a.events() == b.events() == ["0", "1", "2", "9"]
        for e in a.events():
            for c in range(2):
                assert a.frames(e, c) == b.frames(e, c)
        for (e, c, name), img in frames.items():
            path = os.path.join(out_rd, str(e), "Images", name)
            if (e, c, name) == truncated[0]:
                assert open(path, "rb").read() == truncated[1]  # copied unchanged: still undecodable
                assert b.image(e, name)[1] is None
                continue
            assert open(path, "rb").read(4) == b"ABF1"
            rc, got = b.image(e, name)
            assert rc == 1 and np.array_equal(got, img), (e, name)
    finally:
        a.close()
        b.close()
    run_id = os.path.basename(out_rd)
    listed = [line.split()[1] for line in open(os.path.join(out_rd, run_id + ".txt"))]
    assert listed == ["0", "1", "2"]


def test_repack_cli_and_python_entry(tmp_path):
    rd, frames = make_run_dir(str(tmp_path / "data"))
    key = (1, 1, "cam1_image33.png")
    victim = os.path.join(rd, "1", "Images", key[2])
    cut = open(victim, "rb").read()[:200]
    open(victim, "wb").write(cut)
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
    out = str(tmp_path / "packed")
    r = subprocess.run([exe, "-d", os.path.dirname(rd), "-r", "20200925_1", "--repack", out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "repack: 4 events, 71 frames packed" in r.stdout and "1 copied as they are, 0 not written" in r.stdout, r.stdout
    check_repacked("raw", rd + "/", os.path.join(out, "20200925_1"), frames, (key, cut))
    assert open(os.path.join(out, "20200925_1", "20200925_1.txt")).read() == open(os.path.join(rd, "20200925_1.txt")).read()
    # from a zip archive, through the Python entry
    zpath = str(tmp_path / "data" / "20200925_1.zip")
    zip_run(rd, zpath, zipfile.ZIP_DEFLATED)
    run = host.Run("zip", zpath, "Images")
    out2 = str(tmp_path / "packed2" / "20200925_1")
    st = run.repack(out2, nthreads=3, ncams=2)
    run.close()
    assert st["packed"] == 71 and st["copied"] == 1 and st["failed"] == 0 and 0 < st["bytes_out"]
    check_repacked("zip", zpath, out2, frames, (key, cut))
    r = subprocess.run([exe, "-z", "-d", os.path.dirname(rd), "-r", "20200925_1", "--repack", str(tmp_path / "packed3")], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    check_repacked("zip", zpath, str(tmp_path / "packed3" / "20200925_1"), frames, (key, cut))
    # refused combinations, and a target that cannot be written
    for extra in (["--merge", "2"], ["--runs", "a,b"], ["--gpu-shard", "0/2"], ["-e", "1"]):
        r = subprocess.run([exe, "-d", os.path.dirname(rd), "-r", "20200925_1", "--repack", out] + extra, env=env,
                           capture_output=True, text=True)
        assert r.returncode != 0 and "--repack cannot be combined" in r.stderr, (extra, r.stderr)
    # into the data directory it reads: refused before a single frame is replaced
    before = open(os.path.join(rd, "0", "Images", "cam0_image30.png"), "rb").read()
    for target in (os.path.dirname(rd), os.path.dirname(rd) + "/./"):
        r = subprocess.run([exe, "-d", os.path.dirname(rd), "-r", "20200925_1", "--repack", target], env=env, capture_output=True,
                           text=True)
        assert r.returncode != 0 and "is the run that is being read" in r.stderr, r.stderr
    run = host.Run("raw", rd + "/", "Images")
    with pytest.raises(RuntimeError, match="is the run that is being read"):
        run.repack(rd, nthreads=2, ncams=2)
    run.close()
    assert open(os.path.join(rd, "0", "Images", "cam0_image30.png"), "rb").read() == before and before[:4] == b"\x89PNG"
    blocked = tmp_path / "file"
    blocked.write_bytes(b"x")
    r = subprocess.run([exe, "-d", os.path.dirname(rd), "-r", "20200925_1", "--repack", str(blocked)], env=env, capture_output=True,
                       text=True)
    assert r.returncode != 0
