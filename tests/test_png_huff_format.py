"""The canonical Huffman-only PNG ("Unpacking a run") on the host: cv::pngHuffEncode against the numpy
restatement of the format (tests/pnghuffref.py), byte for byte; the files through three independent decoders; their
checksums and the Kraft sums of both codes; and abub3hs --unpack / Run.unpack on the host route."""
import io
import os
import subprocess
import zipfile
import zlib

import numpy as np
import pytest
from PIL import Image

import pnghuffref as ref
from autobub3hs_amd import host, synth
from test_abf_format import make_packed_run, make_run_dir, zip_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RUN_ID = "20200925_1"
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def cases():
    """name -> (image, the restatement's file): computed once, shared, never changed"""
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    spec = synth.random_spec(320, 128, 12, 300, 0, margin=10)
    frame = np.ascontiguousarray(synth.render_event(320, 128, spec, 300, 0)[spec.F - 1])
    imgs = ref.small_cases(sample, frame)
    imgs["limit15"] = ref.limit15_case()
    imgs["limit7"] = ref.limit7_case()
    imgs["sample"] = sample
    return {k: (v, ref.encode(v)) for k, v in imgs.items()}


NAMES = ["w1_ones", "w1_sevens", "w2_ones", "3x5", "7x65", "63x3", "64x3", "65x3", "127x3", "128x3", "129x3", "1280x8", "1680x6",
         "160x96", "limit15", "limit7", "sample"]


def test_the_shapes_cover_what_they_are_for(cases):
    assert sorted(cases) == sorted(NAMES)
    lens = lambda name: sorted(v for v in ref.code_lengths(ref.lit_counts(cases[name][0]), 15) if v)
    assert lens("w1_ones") == [1, 1] and lens("w1_sevens") == [1, 2, 2] and lens("w2_ones") == [1, 2, 2]
    # the repair of the literal code must run: the unlimited tree is deeper than 15
    c15 = ref.lit_counts(cases["limit15"][0])
    assert ref.unlimited_depth(c15) == 18 and max(ref.code_lengths(c15, 15)) == 15
    cs = ref.lit_counts(cases["sample"][0])
    assert ref.unlimited_depth(cs) == 20 and int((cs > 0).sum()) == 122
    # the repair of the code-length code must run: the tree over the histogram of the 258 lengths is deeper than 7
    l7 = ref.code_lengths(ref.lit_counts(cases["limit7"][0]), 15) + [0]
    h7 = np.bincount(l7, minlength=19)
    assert ref.unlimited_depth(h7) == 8 and max(ref.code_lengths(h7, 7)) == 7
    assert len(cases["sample"][1]) == 784351  # (the figure of the format's prototype)


@pytest.mark.parametrize("name", NAMES)
def test_host_encoder_writes_the_restatements_bytes(cases, name):
    img, want = cases[name]
    got = host.png_huff_encode(img)
    assert got == want
    H, W = img.shape
    assert len(got) <= ref.file_bound(W, H)


@pytest.mark.parametrize("name", NAMES)
def test_three_decoders_read_the_file_and_the_checksums_hold(cases, name):
    img, png = cases[name]
    H, W = img.shape
    assert np.array_equal(np.array(Image.open(io.BytesIO(png))), img)
    got = host.imdecode(png)
    assert got is not None and np.array_equal(got, img)
    ch = ref.chunks(png)
    assert [c[0] for c in ch] == [b"IHDR", b"IDAT", b"IEND"]
    for kind, data, crc in ch:
        assert zlib.crc32(kind + data) & 0xFFFFFFFF == crc
    z = ch[1][1]
    assert z[:2] == b"\x78\x01"
    raw = zlib.decompress(z)
    assert len(raw) == H * (W + 1) and np.array_equal(ref.unfilter(raw, W, H), img)
    assert int.from_bytes(z[-4:], "big") == zlib.adler32(raw) & 0xFFFFFFFF
    # both codes are complete: the lengths the header states have Kraft sum 1; 16, 17, 18 and the distance code are unused
    cl, sent = ref.header_lengths(z)
    assert cl[16:] == [0, 0, 0] and sent[257] == 0
    assert sum(2.0 ** -v for v in cl if v) == 1.0 and max(cl) <= 7
    assert sum(2.0 ** -v for v in sent if v) == 1.0 and max(sent) <= 15
    assert sent == ref.code_lengths(ref.lit_counts(img), 15) + [0]


def test_length_procedure_of_the_host_is_the_restatements():
    """through the probe abh_png_huff_lengths: hand-made histograms of both alphabets, the repair included"""
    fib = [0, 0, 0, 300, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 0, 0, 0, 0]
    got, depth = host.png_huff_lengths(fib, 7)
    assert depth == ref.unlimited_depth(fib) == 11
    assert list(got) == ref.code_lengths(fib, 7) and sum(2.0 ** -int(v) for v in got if v) == 1.0
    rs = np.random.RandomState(3)
    for trial in range(20):
        counts = (rs.randint(0, 4, 257) * rs.randint(0, 1 << rs.randint(1, 24), 257)).astype(np.uint64)
        counts[256] = 1
        counts[1] += 5
        got, depth = host.png_huff_lengths(counts, 15)
        assert depth == ref.unlimited_depth(counts) and list(got) == ref.code_lengths(counts, 15), trial
    with pytest.raises(ValueError):
        host.png_huff_lengths([0, 5, 0], 7)  # one used symbol: no complete code
    with pytest.raises(ValueError):
        host.png_huff_encode(np.zeros((1, 65536), np.uint8))


# ---- abub3hs --unpack / Run.unpack on the host ------------------------------------------------------------------------------
def tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def check_unpacked(out_rd, frames, copied=()):
    for (e, c, name), img in frames.items():
        data = open(os.path.join(out_rd, str(e), "Images", name), "rb").read()
        if (e, c, name) in copied:
            continue
        assert data == host.png_huff_encode(img), (e, name)
        assert np.array_equal(np.array(Image.open(io.BytesIO(data))), img)


def verify_all_same_not_packed(src_kind, src, out_rd, total, copied=0):
    a, b = host.Run(src_kind, src, "Images"), host.Run("raw", out_rd + "/", "Images")
    try:
        res = a.verify(b, nthreads=4, ncams=2)
    finally:
        a.close()
        b.close()
    assert res["rc"] == 0 and res["same_not_packed"] == total - copied and res["copied"] == copied and res["same"] == 0, res
    assert res["event_file"] == ("same" if src_kind == "raw" else "not compared")  # (an archive has no event file of its own)


def test_unpack_from_a_packed_directory_and_its_archives(tmp_path):
    rd, frames = make_packed_run(str(tmp_path / "data"))
    total = len(frames)
    zs, zd = str(tmp_path / "s.zip"), str(tmp_path / "d.zip")
    zip_run(rd, zs, zipfile.ZIP_STORED)
    zip_run(rd, zd, zipfile.ZIP_DEFLATED)
    trees = []
    for tag, kind, src in (("dir", "raw", rd + "/"), ("stored", "zip", zs), ("deflated", "zip", zd)):
        out = str(tmp_path / tag / RUN_ID)
        run = host.Run(kind, src, "Images")
        try:
            st = run.unpack(out, nthreads=3, ncams=2)
        finally:
            run.close()
        assert st["packed"] == total and st["copied"] == 0 and st["failed"] == 0 and st["bytes_out"] > 0
        assert set(st) == {"packed", "copied", "failed", "bytes_in", "bytes_out", "seconds"}
        check_unpacked(out, frames)
        verify_all_same_not_packed(kind, src, out, total)
        trees.append(tree(out))
    frames_of = lambda t: {k: v for k, v in t.items() if not k.endswith(".txt")}  # (an archive's event file is rebuilt)
    assert frames_of(trees[0]) == frames_of(trees[1]) == frames_of(trees[2]) and len(frames_of(trees[0])) == total
    assert trees[0][RUN_ID + ".txt"] == open(os.path.join(rd, RUN_ID + ".txt"), "rb").read()


def test_unpack_of_a_mixed_run_copies_what_does_not_decode_and_verifies(tmp_path):
    W, H, F = 96, 64, 12
    rd, frames = make_run_dir(str(tmp_path / "data"), W, H, F, nev=3, ncams=2)
    total = len(frames)
    d1 = os.path.join(rd, "1", "Images")
    key = (1, 1, "cam1_image33.png")
    cut = open(os.path.join(d1, key[2]), "rb").read()[:200]
    open(os.path.join(d1, key[2]), "wb").write(cut)  # a truncated PNG
    for name in ("cam0_image31.png", "cam0_image35.png"):  # packed already
        open(os.path.join(d1, name), "wb").write(host.abf_encode(frames[(1, 0, name)]))
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4", ABUB_GPU_DECODE="0")
    data = os.path.dirname(rd)
    out = str(tmp_path / "U")
    r = subprocess.run([EXE, "-d", data, "-r", RUN_ID, "--unpack", out, "--verify-repack", out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"unpack: 4 events, {total - 1} frames written as PNG" in r.stdout and "1 copied as they are, 0 not written" in r.stdout
    assert f"{total - 1} same but not packed, 1 copied, 0 differ, 0 missing, 0 undecodable, 0 extra; event file same" in r.stdout, r.stdout
    out_rd = os.path.join(out, RUN_ID)
    check_unpacked(out_rd, frames, copied={key})
    assert open(os.path.join(out_rd, "1", "Images", key[2]), "rb").read() == cut
    assert os.path.isdir(os.path.join(out_rd, "9", "Images"))
    assert open(os.path.join(out_rd, RUN_ID + ".txt")).read() == open(os.path.join(rd, RUN_ID + ".txt")).read()
    verify_all_same_not_packed("raw", rd + "/", out_rd, total, copied=1)


def test_cli_refusals(tmp_path):
    rd, _ = make_run_dir(str(tmp_path / "data"), F=2, nev=1)
    data = os.path.dirname(rd)
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="2")
    out = str(tmp_path / "U")

    def cli(*args):
        return subprocess.run([EXE, "-d", data, "-r", RUN_ID] + list(args), env=env, capture_output=True, text=True)

    h = subprocess.run([EXE, "-h"], env=env, capture_output=True, text=True).stdout
    assert "--unpack = Dir" in h and "--unpack-gpu" in h and "--unpack out_data_dir [--unpack-gpu]" in h
    r = cli("-o", str(tmp_path), "--unpack-gpu")
    assert r.returncode != 0 and "--unpack-gpu is valid only together with --unpack" in r.stderr, r.stderr
    r = cli("--repack", out, "--unpack-gpu")
    assert r.returncode != 0 and "--unpack-gpu is valid only together with --unpack" in r.stderr, r.stderr
    r = cli("--unpack", out, "--repack-gpu")
    assert r.returncode != 0 and "--repack-gpu is valid only together with --repack" in r.stderr, r.stderr
    for args in (["--unpack", out, "--repack", out], ["--repack", out, "--unpack", out]):
        r = cli(*args)
        assert r.returncode != 0 and "--unpack cannot be combined with --repack" in r.stderr, r.stderr
    for extra in (["--merge", "2"], ["--runs", "a,b"], ["--gpu-shard", "0/2"], ["-e", "1"]):
        r = cli("--unpack", out, *extra)
        assert r.returncode != 0 and "--unpack cannot be combined" in r.stderr, (extra, r.stderr)
    r = cli("--unpack", out, "--verify-repack", out + "x")
    assert r.returncode != 0 and "--unpack and --verify-repack together must name the same directory" in r.stderr, r.stderr
    assert not os.path.exists(out)
    # into the data directory it reads: refused before a single frame is replaced
    first = os.path.join(rd, "0", "Images", "cam0_image30.png")
    before = open(first, "rb").read()
    r = cli("--unpack", data)
    assert r.returncode != 0 and "is the run that is being read" in r.stderr, r.stderr
    run = host.Run("raw", rd + "/", "Images")
    try:
        with pytest.raises(RuntimeError, match="unpack: .* is the run that is being read"):
            run.unpack(rd, nthreads=2, ncams=2)
    finally:
        run.close()
    assert open(first, "rb").read() == before
    blocked = tmp_path / "file"
    blocked.write_bytes(b"x")
    r = cli("--unpack", str(blocked))
    assert r.returncode != 0  # (as --repack: something could not be written)
