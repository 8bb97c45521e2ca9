"""abub3hs --verify-repack / Run.verify on the CPU side: abub_frames_compare_dev is declared, exported, bound and validates
its arguments without a device; the host route (the definition) on a clean repacked run, on one tampering per case, on 25 at
once (order of the findings, the CLI's cap of 20 lines); the CLI's flags and refusals; and --verify-gpu / verify(device=...)
refuse to run without a device.  The tamperings (CASES) are shared with tests/test_gpu_verify.py, which puts every one of
them through the device route as well."""
import ctypes
import io
import os
import shutil
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

from autobub3hs_amd import _lib, hip, host
from test_abf_format import make_run_dir, zip_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
ENV = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
RUN_ID = "20200925_1"
W, H, F, NEV, NCAMS = 96, 64, 12, 3, 2
TOTAL = F * NEV * NCAMS
E_INVALID = -1
VERDICTS = ("same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_compare_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "typedef struct abub_cmp_pair { uint64_t a, b; } abub_cmp_pair;" in hdr
    assert "typedef struct abub_cmp_result {" in hdr and "#define ABUB_CMP_E_RANGE 1 " in hdr
    assert "int abub_frames_compare_dev(const uint8_t *a, size_t a_bytes, const uint8_t *b, size_t b_bytes, const abub_cmp_pair *pairs," in hdr
    assert "memcmp" in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frames_compare_dev") and "abub_frames_compare_dev" in _lib.SIGNATURES
    assert callable(hip.frames_compare)


def test_compare_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(a=p, a_bytes=4096, b=p, b_bytes=4096, pairs=p, npairs=1, frame_bytes=64, results=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frames_compare_dev(a["a"], a["a_bytes"], a["b"], a["b_bytes"], a["pairs"], a["npairs"], a["frame_bytes"],
                                         a["results"], a["stream"])

    bad = [dict(a=None), dict(b=None), dict(pairs=None), dict(results=None), dict(npairs=-1), dict(frame_bytes=0),
           dict(frame_bytes=(1 << 32) - 1), dict(frame_bytes=1 << 32), dict(pairs=p + 4), dict(results=p + 4)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frames_compare_dev" in L.abub_last_error(), kw
    assert call(npairs=0) == 0  # nothing to do, nothing touched
    assert call(npairs=0, frame_bytes=(1 << 32) - 2) == 0
    assert not any(buf)


# ---- runs and tamperings ---------------------------------------------------------------------------------------------------
def png_bytes(img):
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG")
    return b.getvalue()


class World:
    """a source run (a directory), its repacked copy, and what the source's frames hold"""

    def __init__(self, root, src, out, frames):
        self.root, self.src, self.out, self.frames = root, src, out, frames

    def path(self, tree, e, name):
        return os.path.join(tree, str(e), "Images", name)

    def repack(self):
        shutil.rmtree(self.out, ignore_errors=True)
        run = host.Run("raw", self.src + "/", "Images")
        try:
            return run.repack(self.out, nthreads=4, ncams=NCAMS)
        finally:
            run.close()

    def open_src(self, kind="raw"):
        """kind: raw, or the source as a stored / deflated archive"""
        if kind == "raw":
            return host.Run("raw", self.src + "/", "Images")
        z = os.path.join(self.root, kind + ".zip")
        if not os.path.exists(z):
            zip_run(self.src, z, zipfile.ZIP_STORED if kind == "stored" else zipfile.ZIP_DEFLATED)
        return host.Run("zip", z, "Images")

    def verify(self, kind="raw", other=None, **kw):
        a = self.open_src(kind)
        b = host.Run("raw", (other or self.out) + "/", "Images")
        try:
            return a.verify(b, nthreads=kw.pop("nthreads", 4), ncams=NCAMS, **kw)
        finally:
            a.close()
            b.close()


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("verify_base"))
    rd, frames = make_run_dir(os.path.join(root, "data"), W, H, F, NEV, NCAMS)
    w = World(root, rd, os.path.join(root, "packed", RUN_ID), frames)
    st = w.repack()
    assert st["packed"] == TOTAL and st["copied"] == 0 and st["failed"] == 0
    return w


def fresh(base, tmp_path):
    """the base world copied, for a test to tamper with"""
    root = str(tmp_path)
    src, out = os.path.join(root, "data", RUN_ID), os.path.join(root, "packed", RUN_ID)
    shutil.copytree(base.src, src)
    shutil.copytree(base.out, out)
    return World(root, src, out, base.frames)


def rewrite(path, change):
    """the file's bytes replaced by change(bytes)"""
    data = open(path, "rb").read()
    open(path, "wb").write(change(data))


def bumped(img, pixels):
    """img with the pixels (x, y, d) moved by d grey levels (down where up would leave the range)"""
    img = img.copy()
    for x, y, d in pixels:
        v = int(img[y, x])
        img[y, x] = v + d if v + d <= 255 else v - d
    return img


KEY = (1, 1, "cam1_image33.png")  # the frame most cases tamper with


def finding(verdict, key=KEY, **kw):
    return dict(dict(event=str(key[0]), name=key[2], verdict=verdict, ndiff=0, x=-1, y=-1, max_abs=0, w=0, h=0, other_w=0,
                     other_h=0), **kw)


def case_one_pixel(w):
    open(w.path(w.out, *KEY[::2]), "wb").write(host.abf_encode(bumped(w.frames[KEY], [(12, 3, 5)])))
    return [finding("differ", ndiff=1, x=12, y=3, max_abs=5)]


def case_two_pixels(w):
    open(w.path(w.out, *KEY[::2]), "wb").write(host.abf_encode(bumped(w.frames[KEY], [(7, 10, 5), (90, 2, 9)])))
    return [finding("differ", ndiff=2, x=90, y=2, max_abs=9)]


def case_deleted(w):
    os.remove(w.path(w.out, *KEY[::2]))
    return [finding("missing")]


def case_truncated(w):
    rewrite(w.path(w.out, *KEY[::2]), lambda d: d[:-1])
    return [finding("undecodable")]


def case_flipped_payload_byte(w):
    p = w.path(w.out, *KEY[::2])
    data = bytearray(open(p, "rb").read())
    payload = 32 + 8 * H + ((H * ((W + 63) // 64) + 3) & ~3)
    data[payload] ^= 1  # the first pixel of row 0: the row's check no longer holds
    open(p, "wb").write(bytes(data))
    return [finding("undecodable")]


def case_png_copy(w):
    open(w.path(w.out, *KEY[::2]), "wb").write(png_bytes(w.frames[KEY]))
    return [finding("same_not_packed")]


def case_other_size(w):
    open(w.path(w.out, *KEY[::2]), "wb").write(host.abf_encode(np.ascontiguousarray(w.frames[KEY][:32, :48])))
    return [finding("differ", w=W, h=H, other_w=48, other_h=32)]


def case_source_does_not_decode(w):
    rewrite(w.path(w.src, *KEY[::2]), lambda d: d[:200])
    st = w.repack()
    assert st["copied"] == 1 and st["packed"] == TOTAL - 1
    return []  # copied: no finding, no failure


def case_source_does_not_decode_copy_altered(w):
    case_source_does_not_decode(w)
    p = w.path(w.out, *KEY[::2])
    data = bytearray(open(p, "rb").read())
    data[150] ^= 0x40
    open(p, "wb").write(bytes(data))
    return [finding("undecodable")]


def case_extra_frame_and_event(w):
    shutil.copy(w.path(w.out, 2, "cam0_image30.png"), w.path(w.out, 2, "cam0_image99.png"))
    os.makedirs(os.path.join(w.out, "5", "Images"))
    return [finding("extra", key=(2, 0, "cam0_image99.png")), finding("extra", key=(5, 0, ""))]


def case_event_file_altered(w):
    open(os.path.join(w.out, RUN_ID + ".txt"), "a").write(f"{RUN_ID} 9 a b c d e f g h i\n")
    return [dict(finding("event_file_differs"), event="", name=RUN_ID + ".txt")]


def case_event_file_deleted(w):
    os.remove(os.path.join(w.out, RUN_ID + ".txt"))
    return [dict(finding("event_file_missing"), event="", name=RUN_ID + ".txt")]


CASES = {f.__name__[5:]: f for f in (case_one_pixel, case_two_pixels, case_deleted, case_truncated, case_flipped_payload_byte,
                                     case_png_copy, case_other_size, case_source_does_not_decode,
                                     case_source_does_not_decode_copy_altered, case_extra_frame_and_event, case_event_file_altered,
                                     case_event_file_deleted)}
FAILURES = ("differ", "missing", "undecodable", "extra", "event_file_differs", "event_file_missing")


def check(res, expected, copied=0, event_file=None, total=TOTAL):
    """the findings are the expected ones, and the counters are theirs: every other frame is `same`"""
    assert res["findings"] == expected, res["findings"]
    n = {v: sum(1 for f in expected if f["verdict"] == v) for v in VERDICTS}
    n["copied"] = copied
    n["same"] = total - sum(n[v] for v in VERDICTS if v not in ("same", "extra"))
    for v in VERDICTS:
        assert res[v] == n[v], (v, res)
    assert res["frames"] == total == sum(res[v] for v in VERDICTS if v != "extra") and res["events"] == NEV + 1
    if event_file is None:
        event_file = {"event_file_differs": "differs", "event_file_missing": "missing"}.get(expected[-1]["verdict"] if expected else "", "same")
    assert res["event_file"] == event_file
    assert res["rc"] == (1 if any(f["verdict"] in FAILURES for f in expected) else 0)


def test_clean_run_verifies(base):
    res = base.verify()
    check(res, [])
    assert res["same"] == TOTAL and res["device"] == -1 and res["seconds"] > 0
    for kind in ("stored", "deflated"):  # an archive has no event file of its own: repack writes one, nothing to compare it with
        check(base.verify(kind), [], event_file="not compared")
    # the source against itself: the same pixels everywhere, and not a packed frame among them
    res = base.verify(other=base.src)
    assert res["rc"] == 0 and res["same_not_packed"] == TOTAL and res["same"] == 0 and res["event_file"] == "same"
    assert [f["verdict"] for f in res["findings"]] == ["same_not_packed"] * TOTAL
    names = [(f["event"], f["name"]) for f in res["findings"]]
    assert names == sorted(names, key=lambda t: (int(t[0]), t[1])) and len(set(names)) == TOTAL


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_tampering(base, tmp_path, name):
    w = fresh(base, tmp_path)
    expected = CASES[name](w)
    check(w.verify(), expected, copied=1 if name.startswith("source_does_not_decode") and not expected else 0)
    if name == "other_size":
        r = subprocess.run([EXE, "-d", os.path.dirname(w.src), "-r", RUN_ID, "--verify-repack", os.path.dirname(w.out)], env=ENV,
                           capture_output=True, text=True)
        assert r.returncode == 1 and f"verify: 1/{KEY[2]}: differ: size 96x64 in the source, 48x32 in the other run" in r.stdout, r.stdout
    if name == "one_pixel":
        r = subprocess.run([EXE, "-d", os.path.dirname(w.src), "-r", RUN_ID, "--verify-repack", os.path.dirname(w.out)], env=ENV,
                           capture_output=True, text=True)
        assert r.returncode == 1 and f"verify: 1/{KEY[2]}: differ: 1 pixels, first at (x=12, y=3), max |a-b| = 5\n" in r.stdout, r.stdout


def tamper_25(w):
    """25 frames tampered with, in an order that is not the tasks'; -> the findings in task order"""
    rng = np.random.default_rng(7)
    keys = sorted(w.frames, key=lambda k: (k[0], k[1], k[2]))
    picked = [keys[i] for i in rng.permutation(len(keys))[:25]]
    want = {}
    for n, key in enumerate(picked):
        p = w.path(w.out, key[0], key[2])
        if n % 3 == 0:
            os.remove(p)
            want[key] = finding("missing", key=key)
        elif n % 3 == 1:
            rewrite(p, lambda d: d[:-1])
            want[key] = finding("undecodable", key=key)
        else:
            x, y = int(rng.integers(W)), int(rng.integers(H))
            open(p, "wb").write(host.abf_encode(bumped(w.frames[key], [(x, y, 3)])))
            want[key] = finding("differ", key=key, ndiff=1, x=x, y=y, max_abs=3)
    return [want[k] for k in keys if k in want]


def summary_and_findings(stdout):
    lines = stdout.splitlines()
    return [l for l in lines if l.startswith("verify: ") and " events, " not in l], [l for l in lines if l.startswith("verify: ") and " events, " in l]


def test_findings_come_in_task_order_and_the_cli_caps_them(base, tmp_path):
    w = fresh(base, tmp_path)
    expected = tamper_25(w)
    assert len(expected) == 25
    for threads in (1, 4):
        check(w.verify(nthreads=threads), expected)
    r = subprocess.run([EXE, "-d", os.path.dirname(w.src), "-r", RUN_ID, "--verify-repack", os.path.dirname(w.out)], env=ENV,
                       capture_output=True, text=True)
    assert r.returncode == 1, r.stdout + r.stderr
    found, summary = summary_and_findings(r.stdout)
    assert len(found) == 20 and len(summary) == 1
    assert [l.split(": ")[1] for l in found] == [f"{f['event']}/{f['name']}" for f in expected[:20]]
    lines = r.stdout.splitlines()
    assert lines[20] == "... and 5 more" and lines[21] == summary[0]
    n = {v: sum(1 for f in expected if f["verdict"] == v) for v in VERDICTS}
    assert summary[0].startswith(f"verify: {NEV + 1} events, {TOTAL} frames: {TOTAL - 25} same, 0 same but not packed, 0 copied, "
                                 f"{n['differ']} differ, {n['missing']} missing, {n['undecodable']} undecodable, 0 extra; event file same; ")
    assert summary[0].endswith(" frames/s")


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def cli(*args):
    return subprocess.run([EXE] + list(args), env=ENV, capture_output=True, text=True)


def test_cli_flags_and_refusals(base, tmp_path):
    r = cli("-h")
    assert "--verify-repack" in r.stdout and "--verify-gpu" in r.stdout
    assert "-r run_ID --verify-repack other_data_dir [--verify-gpu]" in r.stdout
    data, packed = os.path.dirname(base.src), os.path.dirname(base.out)
    r = cli("-d", data, "-r", RUN_ID, "-o", str(tmp_path), "--verify-gpu")
    assert r.returncode != 0 and "--verify-gpu is valid only together with --verify-repack" in r.stderr, r.stderr
    for extra in (["--merge", "2"], ["--runs", "a,b"], ["--gpu-shard", "0/2"], ["-e", "1"]):
        r = cli("-d", data, "-r", RUN_ID, "--verify-repack", packed, *extra)
        assert r.returncode != 0 and "--verify-repack cannot be combined" in r.stderr, (extra, r.stderr)
    x, y = str(tmp_path / "X"), str(tmp_path / "Y")
    r = cli("-d", data, "-r", RUN_ID, "--repack", x, "--verify-repack", y)
    assert r.returncode != 0 and "must name the same directory" in r.stderr and not os.path.exists(x) and not os.path.exists(y)
    r = cli("-d", data, "-r", RUN_ID, "--verify-repack")
    assert r.returncode != 0 and "--verify-repack needs" in r.stderr
    # verify alone, of a clean copy: no -o, exit status 0, the summary line and nothing else
    r = cli("-d", data, "-r", RUN_ID, "--verify-repack", packed)
    assert r.returncode == 0, r.stdout + r.stderr
    found, summary = summary_and_findings(r.stdout)
    assert not found and len(summary) == 1 and f"{TOTAL} frames: {TOTAL} same, " in summary[0] and "event file same" in summary[0]
    # repack, then verify what it wrote
    r = cli("-d", data, "-r", RUN_ID, "--repack", x, "--verify-repack", x)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith(f"repack: {NEV + 1} events, {TOTAL} frames packed") and lines[1].startswith(f"verify: {NEV + 1} events, {TOTAL} frames: {TOTAL} same, ")
    assert open(os.path.join(x, RUN_ID, "0", "Images", "cam0_image30.png"), "rb").read(4) == b"ABF1"
    # ... from an archive: the event file is one repack made up
    zip_run(base.src, os.path.join(str(tmp_path), RUN_ID + ".zip"), zipfile.ZIP_DEFLATED)
    r = cli("-z", "-d", str(tmp_path), "-r", RUN_ID, "--repack", y, "--verify-repack", y)
    assert r.returncode == 0 and f"{TOTAL} frames: {TOTAL} same, " in r.stdout and "event file not compared" in r.stdout, r.stdout + r.stderr
    # a copy that is not there: every frame is missing, and so is the event file
    r = cli("-d", data, "-r", RUN_ID, "--verify-repack", str(tmp_path / "nowhere"))
    assert r.returncode == 1 and f"{TOTAL} missing" in r.stdout and "event file missing" in r.stdout and "... and " in r.stdout


def test_verify_gpu_is_refused_without_a_device(base):
    """there is no silent fall-back to the host route (as test_abf_encode_abi.test_repack_gpu_is_refused_without_a_device)"""
    if torch.cuda.is_available():
        return
    r = cli("-d", os.path.dirname(base.src), "-r", RUN_ID, "--verify-repack", os.path.dirname(base.out), "--verify-gpu")
    assert r.returncode != 0 and "no such HIP device" in r.stderr and "verify: " not in r.stdout, r.stdout + r.stderr
    with pytest.raises(RuntimeError, match="no such HIP device"):
        base.verify(device=0)
    with pytest.raises(RuntimeError, match="no such HIP device"):
        base.verify(device=-1)
