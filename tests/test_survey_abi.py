"""abub3hs --survey / Run.survey on the CPU side: abub_frame_stats_dev is declared, exported, bound and validates its
arguments without a device; frameStatsHost (the definition) against the numpy restatement (tests/surveyref.py); the report
against known-answer text; the CLI's host route on a small damaged run in five source forms, which must all give the report
surveyref gives; a run that does not train; the flags and refusals; and a detect run is not changed by a survey before it.
The run (make_survey_run) is shared with tests/test_gpu_survey_routes.py, which puts it through the device route as well."""
import ctypes
import os
import shutil
import subprocess
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import bmpfiles
import surveyref
from autobub3hs_amd import _lib, hip, host
from test_abf_format import zip_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
ENV = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
RUN_ID = "20200925_1"
W, H, F, NEV, NCAMS = 40, 24, 12, 3, 2
TOTAL = F * NEV * NCAMS
E_INVALID = -1
SIZES = [1, 3, 15, 16, 17, 63, 64, 65, 960, 4095, 16383, 16384, 16385, 3 * 16384 + 5]
# the damage of the run: what the frame's file is made to be
TRUNCATED, EMPTY, REMOVED, WIDER = (0, 0, "cam0_image33.png"), (0, 1, "cam1_image35.png"), (1, 0, "cam0_image36.png"), (1, 1, "cam1_image32.png")
WHITE, BLACK = (2, 0, "cam0_image34.png"), (2, 1, "cam1_image41.png")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_frame_stats_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "typedef struct abub_stat_job { uint64_t cur, ref, model; } abub_stat_job;" in hdr
    assert "typedef struct abub_stat_result {   /* 64 bytes */" in hdr and "#define ABUB_STAT_E_RANGE 1 " in hdr
    assert "int abub_frame_stats_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6," in hdr
    for cite in ("AnalyzerUnit.cpp:341-351", "L3Localizer.cpp:779-787", "Trainer.cpp:191-195"):
        assert cite in hdr, cite
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_stats_dev") and "abub_frame_stats_dev" in _lib.SIGNATURES
    assert callable(hip.frame_stats) and callable(host.Run.survey)
    for name in ("abh_run_survey", "abh_run_survey_dev", "abh_frame_stats_host"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_frame_stats_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, sigma6=p, model_bytes=4096, jobs=p, njobs=1, frame_bytes=64, results=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_stats_dev(a["frames"], a["frames_bytes"], a["mu"], a["sigma6"], a["model_bytes"], a["jobs"], a["njobs"],
                                      a["frame_bytes"], a["results"], a["stream"])

    bad = [dict(frames=None), dict(jobs=None), dict(results=None), dict(sigma6=None), dict(njobs=-1), dict(frame_bytes=0),
           dict(frame_bytes=(1 << 32) - 1), dict(frame_bytes=1 << 32), dict(jobs=p + 4), dict(results=p + 4)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_stats_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, mu=None, sigma6=None, frame_bytes=(1 << 32) - 2) == 0
    assert not any(buf)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def stat_contents(n, rs):
    """the jobs of one size -> [(cur, ref or None, mu or None, sigma6 or None)]: random; all 0; all 255; p = m +- s exactly
    and one beyond on either side; s = 0 and s = 255; cur == ref; no ref; no model"""
    rnd = lambda: rs.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    full = lambda v: np.full(n, v, np.uint8)  # noqa: E731
    m = rs.randint(40, 200, n).astype(np.uint8)
    s = rs.randint(0, 30, n).astype(np.uint8)
    step = np.resize(np.array([0, 1, -1, 0], np.int16), n)  # on the bound, one beyond it, one inside it
    up = (m.astype(np.int16) + s + step).astype(np.uint8)
    down = (m.astype(np.int16) - s - step).astype(np.uint8)
    cur = rnd()
    return [(cur, rnd(), rnd(), rnd()), (full(0), full(0), full(0), full(0)), (full(255), full(255), full(255), full(255)),
            (full(255), full(0), full(0), full(0)), (full(0), full(255), full(255), full(3)), (up, down, m, s), (down, up, m, s),
            (rnd(), rnd(), rnd(), full(0)), (rnd(), rnd(), rnd(), full(255)), (cur, cur, rnd(), rnd()), (rnd(), None, rnd(), rnd()),
            (rnd(), rnd(), None, None), (rnd(), None, None, None)]


@pytest.mark.parametrize("n", SIZES)
def test_host_definition_against_numpy(n):
    rs = np.random.RandomState(n % 9973)
    for k, (cur, ref, mu, s6) in enumerate(stat_contents(n, rs)):
        want = surveyref.record(cur, ref, mu, s6)
        assert host.frame_stats_host(cur, ref, mu, s6) == want, (n, k)
    # the bounds themselves: exactly m +- s leaves nothing, one beyond leaves 1
    m, s = np.full(n, 100, np.uint8), np.full(n, 7, np.uint8)
    for p, left in ((107, 0), (93, 0), (108, 1), (92, 1)):
        got = host.frame_stats_host(np.full(n, p, np.uint8), m, m, s)
        assert (got["n_out"], got["sum_out"], got["n_moved"], got["sum_moved"], got["flags"]) == (n * left, n * left, n * left, n * left, 3)


def test_host_definition_where_sumsq_passes_2_to_the_32():
    n = 1680 * 1050
    got = host.frame_stats_host(np.full(n, 255, np.uint8))
    assert got["sumsq"] == n * 255 * 255 > 1 << 32 and got["sum"] == n * 255 and got["n_sat"] == n and got["min"] == 255 and got["flags"] == 0


# ---- runs --------------------------------------------------------------------------------------------------------------------
def png_bytes(img):
    import io
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG")
    return b.getvalue()


def make_survey_run(root, damaged=True, w=W, h=H, frames_per_stack=F):
    """3 events x 2 cameras x 12 frames of 40 x 24: a steady background per camera with a little noise, and from frame 6 on a
    bright patch that grows.  damaged: one truncated file, one empty file, one removed file, one 44 x 24 file, one all-255
    frame and one all-0 frame -> (run dir, {(event, cam, name): image, None (does not decode) or "missing"})"""
    rs = np.random.RandomState(19)
    rd = os.path.join(root, RUN_ID)
    frames = {}
    for e in range(NEV):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d)
        for c in range(NCAMS):
            back = (np.add.outer(np.arange(h), np.arange(w)) * 2 + 60 + 20 * c).astype(np.int16)
            for k in range(frames_per_stack):
                img = back + rs.randint(-2, 3, (h, w))
                if k >= 6:
                    img[4:4 + k, 8 + e:8 + e + k] += 90
                frames[(e, c, f"cam{c}_image{30 + k}.png")] = np.clip(img, 0, 255).astype(np.uint8)
    if damaged:
        frames[WHITE] = np.full((h, w), 255, np.uint8)
        frames[BLACK] = np.zeros((h, w), np.uint8)
        frames[WIDER] = np.ascontiguousarray(np.pad(frames[WIDER], ((0, 0), (0, 4)), mode="edge"))
    for (e, c, name), img in frames.items():
        open(os.path.join(rd, str(e), "Images", name), "wb").write(png_bytes(img))
    if damaged:
        p = os.path.join(rd, str(TRUNCATED[0]), "Images", TRUNCATED[2])
        data = open(p, "rb").read()
        open(p, "wb").write(data[:len(data) // 2])
        open(os.path.join(rd, str(EMPTY[0]), "Images", EMPTY[2]), "wb").close()
        os.remove(os.path.join(rd, str(REMOVED[0]), "Images", REMOVED[2]))
        frames[TRUNCATED] = frames[EMPTY] = None
        frames[REMOVED] = "missing"
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(NEV):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd, frames


def stacks_of(frames):
    """the frames dict as surveyref.rows_of takes it: stacks in (event, camera) order, their frames in name order"""
    keys = sorted({(e, c) for e, c, _ in frames})
    return [(e, c, sorted((n, img) for (ee, cc, n), img in frames.items() if (ee, cc) == (e, c))) for e, c in keys]


def trained_models(rd, w=W, h=H):
    """what the host Trainer makes of the run per camera (None where it does not train: always, without a GPU)"""
    models = []
    run = host.Run("raw", rd + "/", "Images")
    try:
        for c in range(NCAMS):
            try:
                st, tss, mu, sg = run.train(c, shape=(h, w))
            except RuntimeError:
                st = -7
            models.append(None if st else dict(trained=tss, mu=mu, sigma=sg))
    finally:
        run.close()
    return models


def expected_report(rd, frames, w=W, h=H):
    models = trained_models(rd, w, h)
    return surveyref.report(models, surveyref.rows_of(stacks_of(frames), w, h, models)), models


def bmp_copy(rd, dst):
    """the run with every file that decodes rewritten as a BMP under its own name"""
    shutil.copytree(rd, dst)
    for dp, _, fn in os.walk(dst):
        for f in fn:
            p = os.path.join(dp, f)
            try:
                img = np.array(Image.open(p).convert("L")) if f.endswith(".png") else None
            except Exception:
                img = None
            if img is not None:
                open(p, "wb").write(bmpfiles.pillow_bmp(img, "L"))


class Sources:
    """the five forms of a run: name -> the CLI's arguments in front of --survey"""

    def __init__(self, root, rd):
        self.rd = rd
        self.cli = {"dir": ["-d", os.path.dirname(rd), "-r", RUN_ID]}
        for kind, comp in (("stored", zipfile.ZIP_STORED), ("deflated", zipfile.ZIP_DEFLATED)):
            os.makedirs(os.path.join(root, kind))
            zip_run(rd, os.path.join(root, kind, RUN_ID + ".zip"), comp)
            self.cli[kind] = ["-z", "-d", os.path.join(root, kind), "-r", RUN_ID]
        run = host.Run("raw", rd + "/", "Images")
        try:
            run.repack(os.path.join(root, "packed", RUN_ID), nthreads=4, ncams=NCAMS)
        finally:
            run.close()
        self.cli["packed"] = ["-d", os.path.join(root, "packed"), "-r", RUN_ID]
        bmp_copy(rd, os.path.join(root, "bmp", RUN_ID))
        self.cli["bmp"] = ["-d", os.path.join(root, "bmp"), "-r", RUN_ID]

    def open(self, name):
        args = self.cli[name]
        if args[0] == "-z":
            return host.Run("zip", os.path.join(args[2], RUN_ID + ".zip"), "Images")
        return host.Run("raw", os.path.join(args[1], RUN_ID) + "/", "Images")


@pytest.fixture(scope="module")
def damaged(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("survey_damaged"))
    rd, frames = make_survey_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("survey_clean"))
    rd, frames = make_survey_run(os.path.join(root, "data"), damaged=False)
    return Sources(root, rd), frames


def cli(*args, env=ENV):
    return subprocess.run([EXE] + list(args), env=env, capture_output=True, text=True)


def survey_cli(src_args, out, *more, env=ENV):
    r = cli(*src_args, "--survey", out, *more, env=env)
    return r, (open(out).read() if os.path.exists(out) else None)


def test_cli_host_route_on_every_source_form(damaged, clean, tmp_path):
    src, frames = damaged
    want, models = expected_report(src.rd, frames)
    for name in src.cli:
        r, text = survey_cli(src.cli[name], str(tmp_path / (name + ".txt")))
        assert r.returncode == 1, (name, r.stdout, r.stderr)
        assert text == want, name
        assert f"survey: {NEV} events, {TOTAL} frames {W}x{H}: {TOTAL - 4} ok, 2 undecodable, 1 missing, 1 of another size; " in r.stdout
    states = {(l.split("\t")[0], l.split("\t")[3]): l.split("\t")[4] for l in want.splitlines() if l[0].isdigit()}
    assert states[("0", TRUNCATED[2])] == states[("0", EMPTY[2])] == "undecodable" and states[("1", REMOVED[2])] == "missing"
    assert states[("1", WIDER[2])] == "other_size" and len(states) == TOTAL
    white = [l for l in want.splitlines() if l.startswith(f"2\t0\t4\t{WHITE[2]}\tok\t{W}\t{H}\t255\t255\t{255 * W * H}\t")]
    black = [l for l in want.splitlines() if l.startswith(f"2\t1\t11\t{BLACK[2]}\tok\t{W}\t{H}\t0\t0\t0\t0\t{W * H}\t0\t")]
    assert len(white) == 1 and len(black) == 1
    src, frames = clean
    want, _ = expected_report(src.rd, frames)
    for name in src.cli:
        r, text = survey_cli(src.cli[name], str(tmp_path / ("clean_" + name + ".txt")))
        assert r.returncode == 0 and text == want, (name, r.stdout, r.stderr)
    assert want.splitlines()[-1].startswith(f"run frames {TOTAL} ok {TOTAL} undecodable 0 missing 0 other_size 0 ")


def test_run_survey_agrees_with_the_cli(damaged, tmp_path):
    src, frames = damaged
    want, models = expected_report(src.rd, frames)
    for name in ("dir", "deflated"):
        run = src.open(name)
        try:
            res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS)
        finally:
            run.close()
        assert text == want == open(str(tmp_path / "r.txt")).read()
        assert (res["rc"], res["frames"], res["ok"], res["undecodable"], res["missing"], res["other_size"]) == (1, TOTAL, TOTAL - 4, 2, 1, 1)
        assert res["device"] == -1 and res["frames_kernel"] == 0 and res["frames_host_route"] == TOTAL and res["batches"] == 0
        assert (res["W"], res["H"], res["events"]) == (W, H, NEV) and res["model_cams"] == sum(m is not None for m in models)


KNOWN = """# abub3hs survey 1
model cam 0 none
model cam 1 none
event\tcam\tframe\tname\tstate\tw\th\tmin\tmax\tsum\tsumsq\tn_zero\tn_sat\tn_out\tsum_out\tn_moved\tsum_moved\tmean\tsd
0\t0\t0\tcam0_image30.png\tok\t4\t2\t0\t255\t465\t74125\t1\t1\t-\t-\t-\t-\t58.125000\t76.727501
0\t0\t1\tcam0_image31.png\tundecodable\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-
0\t1\t0\tcam1_image30.png\tok\t4\t2\t7\t7\t56\t392\t0\t0\t-\t-\t-\t-\t7.000000\t0.000000
0\t1\t1\tcam1_image31.png\tundecodable\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-
1\t0\t0\tcam0_image30.png\tmissing\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-
1\t0\t1\tcam0_image31.png\tother_size\t2\t2\t1\t4\t10\t30\t0\t0\t-\t-\t-\t-\t2.500000\t1.118034
1\t1\t0\tcam1_image30.png\tundecodable\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-
1\t1\t1\tcam1_image31.png\tundecodable\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-
run frames 8 ok 2 undecodable 4 missing 1 other_size 1 sigma_zero_share - moved_share_median -
"""


def test_report_against_known_answer_text_and_a_run_that_does_not_train(tmp_path):
    """no stack has a second frame that decodes, so no camera trains (the Trainer wants frames 0 and 1 of an event):
    `model ... none`, the model columns are `-`, the raw columns stay valid"""
    rd = str(tmp_path / "data" / RUN_ID)
    a, seven, small = np.array([[0, 255, 10, 20], [30, 40, 50, 60]], np.uint8), np.full((2, 4), 7, np.uint8), np.array([[1, 2], [3, 4]], np.uint8)
    frames = {(0, 0, "cam0_image30.png"): a, (0, 0, "cam0_image31.png"): None, (0, 1, "cam1_image30.png"): seven,
              (0, 1, "cam1_image31.png"): None, (1, 0, "cam0_image30.png"): "missing", (1, 0, "cam0_image31.png"): small,
              (1, 1, "cam1_image30.png"): None, (1, 1, "cam1_image31.png"): None}
    for (e, c, name), img in frames.items():
        os.makedirs(os.path.join(rd, str(e), "Images"), exist_ok=True)
        if not isinstance(img, str):
            open(os.path.join(rd, str(e), "Images", name), "wb").write(b"not an image" if img is None else png_bytes(img))
    r, text = survey_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "known.txt"))
    assert r.returncode == 1 and text == KNOWN, (r.stdout, r.stderr, text)
    assert "survey: a camera did not train" in r.stdout
    assert surveyref.report([None, None], surveyref.rows_of(stacks_of(frames), 4, 2, [None, None])) == KNOWN


def test_cli_flags_and_refusals(clean, tmp_path):
    src, _ = clean
    r = cli("-h")
    assert "--survey = File" in r.stdout and "--survey-gpu" in r.stdout
    assert "-r run_ID --survey FILE [--survey-gpu]" in r.stdout
    out = str(tmp_path / "s.txt")
    x = str(tmp_path / "X")
    for extra, word in ((["--repack", x], "--repack"), (["--unpack", x], "--unpack"), (["--verify-repack", x], "--verify-repack"),
                        (["--merge", "2"], "--merge"), (["--debug", "101"], "--debug"), (["--per-event"], "--per-event")):
        r = cli(*src.cli["dir"], "--survey", out, *extra)
        assert r.returncode != 0 and f"--survey cannot be combined with {word}" in r.stderr, (extra, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(x)
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-gpu")
    assert r.returncode != 0 and "--survey-gpu is valid only together with --survey" in r.stderr
    r = cli(*src.cli["dir"], "--survey")
    assert r.returncode != 0 and "--survey needs" in r.stderr
    r = cli("-z", "-d", str(tmp_path / "nowhere"), "-r", RUN_ID, "--survey", out)  # an archive that cannot be read: -5
    assert r.returncode == 256 - 5 and not os.path.exists(out), (r.returncode, r.stderr)


def test_survey_gpu_is_refused_without_a_device(clean, tmp_path):
    """there is no silent fall-back to the host route (as test_verify_repack.test_verify_gpu_is_refused_without_a_device)"""
    if torch.cuda.is_available():
        return
    src, _ = clean
    out = str(tmp_path / "s.txt")
    r = cli(*src.cli["dir"], "--survey", out, "--survey-gpu")
    assert r.returncode != 0 and "no such HIP device" in r.stderr and not os.path.exists(out), r.stdout + r.stderr
    run = src.open("dir")
    try:
        with pytest.raises(RuntimeError, match="no such HIP device"):
            run.survey(device=0)
        with pytest.raises(RuntimeError, match="no such HIP device"):
            run.survey(device=-1)
    finally:
        run.close()


def test_a_detect_run_is_the_same_after_a_survey(clean, tmp_path):
    src, _ = clean
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a)
    os.makedirs(b)
    first = cli(*src.cli["dir"], "-o", a)
    r, text = survey_cli(src.cli["dir"], str(tmp_path / "s.txt"))
    assert r.returncode == 0 and text
    second = cli(*src.cli["dir"], "-o", b)
    assert first.returncode == second.returncode
    name = f"abub3hs_{RUN_ID}.txt"
    assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read() != b""
