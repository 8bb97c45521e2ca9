"""abub3hs --survey --survey-planes / Run.survey(planes=...) on the CPU side: abub_pixel_activity_dev is declared, exported,
bound and validates its arguments without a device; activityAddHost (the definition) against the numpy restatement
(tests/activityref.py) onto planes that start at random values; the CLI's host route on the damaged run of
tests/test_survey_abi.py in five source forms, which must all write the files the restatement gives, next to an unchanged
report; the column identity between the planes and the report; a camera that does not train; the flags and refusals."""
import ctypes
import io
import os

import numpy as np
import pytest
from PIL import Image

import activityref
import surveyref
from autobub3hs_amd import _lib, hip, host
from test_survey_abi import (ENV, H, NCAMS, RUN_ID, W, clean, cli, damaged, expected_report, png_bytes, stacks_of,  # noqa: F401
                             stat_contents, survey_cli, trained_models)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SIZES = [1, 3, 15, 16, 17, 64, 255, 960, 1023, 1025, 16401]


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def read_planes_dir(d):
    """a planes directory -> {file name: bytes, a PNG decoded}"""
    out = {}
    for f in sorted(os.listdir(d)):
        data = open(os.path.join(d, f), "rb").read()
        out[f] = np.array(Image.open(io.BytesIO(data))) if f.endswith(".png") else data
    return out


def same_files(got, want):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for f in want:
        if f.endswith(".png"):
            assert got[f].dtype == np.uint8 and np.array_equal(got[f], want[f]), f
        else:
            assert got[f] == want[f], (f, got[f][:200], want[f][:200])


def planes_of_npy(data, w=W, h=H):
    """the data of a cam<c>_activity.npy as numpy itself reads it: u32 [6, h * w]"""
    a = np.load(io.BytesIO(data))
    assert a.dtype == np.dtype("<u4") and a.shape == (6, h, w) and (len(data) - a.nbytes) % 64 == 0
    return a.reshape(6, -1).astype(np.int64)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_pixel_activity_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "typedef struct abub_act_job { uint64_t cur, ref; } abub_act_job;" in hdr and "#define ABUB_ACT_E_RANGE 1" in hdr
    assert "int abub_pixel_activity_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6," in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_pixel_activity_dev") and "abub_pixel_activity_dev" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.ActJob) == 16 and callable(hip.pixel_activity) and hip.ACT_PLANES == activityref.PLANES
    for name in ("abh_run_survey_planes", "abh_run_survey_planes_dev", "abh_activity_add_host", "abh_run_survey", "abh_run_survey_dev"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_pixel_activity_validates_before_it_touches_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(frames=p, frames_bytes=4096, mu=p, sigma6=p, jobs=p, njobs=1, frame_bytes=64, planes=p, plane_stride=64, status=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_pixel_activity_dev(a["frames"], a["frames_bytes"], a["mu"], a["sigma6"], a["jobs"], a["njobs"], a["frame_bytes"],
                                         a["planes"], a["plane_stride"], a["status"], a["stream"])

    bad = [dict(frames=None), dict(jobs=None), dict(planes=None), dict(status=None), dict(mu=None), dict(sigma6=None), dict(njobs=-1),
           dict(frame_bytes=0), dict(frame_bytes=(1 << 32) - 1, plane_stride=1 << 32), dict(frame_bytes=1 << 32, plane_stride=1 << 33),
           dict(plane_stride=60), dict(frame_bytes=63, plane_stride=63), dict(plane_stride=66), dict(planes=p + 4), dict(planes=p + 8),
           dict(jobs=p + 4), dict(status=p + 2)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_pixel_activity_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, mu=None, sigma6=None, frame_bytes=(1 << 32) - 2, plane_stride=(1 << 32) - 4 + 4) == 0
    assert not any(buf)


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_host_definition_against_numpy(n):
    rs = np.random.RandomState(n % 9973)
    for k, (cur, ref, mu, s6) in enumerate(stat_contents(n, rs)):
        start = rs.randint(0, 1 << 31, (6, n)).astype(np.uint32)  # (an overwrite would show)
        planes = start.copy()
        host.activity_add_host(planes, cur, ref, mu, s6)
        want = start.astype(np.int64) + activityref.terms(cur, ref if mu is not None else None, mu, s6)
        assert np.array_equal(planes.astype(np.int64), want), (n, k)
        # and the terms are those the per-frame record sums
        rec, t = surveyref.record(cur, ref if mu is not None else None, mu, s6), activityref.terms(cur, ref if mu is not None else None, mu, s6)
        assert [int(x) for x in t.sum(axis=1)] == [rec[key] for key in activityref.PLANES], (n, k)
    planes = np.zeros((6, n), np.uint32)
    for _ in range(3):  # it adds
        host.activity_add_host(planes, np.full(n, 255, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8))
    assert np.array_equal(planes, np.outer([0, 3, 3, 765, 3, 765], np.ones(n, np.int64)))


# ---- runs --------------------------------------------------------------------------------------------------------------------
def test_cli_host_route_on_every_source_form(damaged, tmp_path):  # noqa: F811
    src, frames = damaged
    want_report, models = expected_report(src.rd, frames)
    want = activityref.files_of(stacks_of(frames), W, H, models)
    assert sum(f.endswith(".npy") for f in want) == NCAMS
    for name in src.cli:
        bare, report_bare = survey_cli(src.cli[name], str(tmp_path / (name + "_bare.txt")))
        out = str(tmp_path / name)
        r, report = survey_cli(src.cli[name], str(tmp_path / (name + ".txt")), "--survey-planes", out)
        assert r.returncode == bare.returncode == 1, (name, r.stdout, r.stderr)
        assert report == report_bare == want_report, name
        same_files(read_planes_dir(os.path.join(out, RUN_ID)), want)
        assert f"survey-planes: {out}/{RUN_ID}: 0 rows added on the GPU, {NCAMS * 36 - 4} on the host" in r.stdout, r.stdout
        assert "survey-planes" not in bare.stdout
    # Run.survey agrees with the CLI
    run = src.open("deflated")
    try:
        res, text = run.survey(None, nthreads=4, ncams=NCAMS, planes=str(tmp_path / "py" / "sub"))
    finally:
        run.close()
    assert text == want_report and res["plane_rows_host"] == NCAMS * 36 - 4 and res["plane_rows_kernel"] == 0
    same_files(read_planes_dir(str(tmp_path / "py" / "sub")), want)


def test_plane_totals_equal_the_reports_columns(clean, tmp_path):  # noqa: F811
    """per camera and plane: the plane's total over the pixels = the sum of the report's column over the counted rows"""
    for (src, _), tag in ((clean, "clean"),):
        out = str(tmp_path / tag)
        r, report = survey_cli(src.cli["dir"], str(tmp_path / (tag + ".txt")), "--survey-planes", out)
        assert r.returncode == 0, r.stderr
        txt = open(os.path.join(out, RUN_ID, "activity.txt")).read().splitlines()
        assert txt[0] == "# abub3hs activity 1"
        for c in range(NCAMS):
            planes = planes_of_npy(open(os.path.join(out, RUN_ID, f"cam{c}_activity.npy"), "rb").read())
            sums, counted = np.zeros(6, np.int64), np.zeros(3, np.int64)
            for line in report.splitlines():
                f = line.split("\t")
                if len(f) != 19 or f[1] != str(c) or f[4] != "ok":
                    continue
                counted += [1, f[13] != "-", f[15] != "-"]
                sums += [int(f[11]), int(f[12])] + [0 if v == "-" else int(v) for v in f[13:17]]
            assert counted[0] == 36 and np.array_equal(planes.sum(axis=1), sums), (c, planes.sum(axis=1), sums)
            assert f"cam {c} w {W} h {H} frames {counted[0]} frames_model {counted[1]} frames_moved {counted[2]}" in txt


def test_a_camera_that_does_not_train(tmp_path):
    """camera 1 has no second frame that decodes in any event, so it has no model (the Trainer wants frames 0 and 1 of an
    event): its planes 2 to 5 stay zero, frames_model is 0 and it gets no image"""
    rd = str(tmp_path / "data" / RUN_ID)
    rs = np.random.RandomState(4)
    frames = {}
    for e in range(2):
        for k in range(4):
            frames[(e, 0, f"cam0_image{30 + k}.png")] = rs.randint(0, 256, (6, 8)).astype(np.uint8)
            frames[(e, 1, f"cam1_image{30 + k}.png")] = None if k == 1 else rs.randint(0, 256, (6, 8)).astype(np.uint8)
    frames[(0, 1, "cam1_image30.png")][0, :3] = (0, 255, 0)
    for (e, c, name), img in frames.items():
        os.makedirs(os.path.join(rd, str(e), "Images"), exist_ok=True)
        open(os.path.join(rd, str(e), "Images", name), "wb").write(b"not an image" if img is None else png_bytes(img))
    out = str(tmp_path / "planes")
    r, report = survey_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "r.txt"), "--survey-planes", out)
    assert r.returncode == 1 and "model cam 1 none" in report, (r.stdout, r.stderr)
    models = trained_models(rd, 8, 6)
    assert models[1] is None
    got = read_planes_dir(os.path.join(out, RUN_ID))
    same_files(got, activityref.files_of(stacks_of(frames), 8, 6, models))
    assert "cam1_moved.png" not in got and ("cam0_moved.png" in got) == (models[0] is not None)
    planes = planes_of_npy(got["cam1_activity.npy"], 8, 6)
    assert not planes[2:].any() and planes[0].sum() > 0 and planes[1].sum() > 0
    assert b"cam 1 w 8 h 6 frames 6 frames_model 0 frames_moved 0\ncam 1 dead 0 stuck_sat 0 ever_out 0 ever_moved 0 moved_10pct 0 moved_50pct 0\n" \
        in got["activity.txt"]


def test_cli_flags_and_refusals(clean, tmp_path):  # noqa: F811
    src, _ = clean
    r = cli("-h")
    assert "--survey-planes = Dir" in r.stdout and "-r run_ID --survey FILE [--survey-gpu] [--survey-planes DIR]" in r.stdout
    out, x, y = str(tmp_path / "s.txt"), str(tmp_path / "X"), str(tmp_path / "Y")
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-planes", x)
    assert r.returncode != 0 and "--survey-planes is valid only together with --survey" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-planes")
    assert r.returncode != 0 and "--survey-planes needs the directory to write to" in r.stderr
    for extra, word in ((["--repack", y], "--repack"), (["--unpack", y], "--unpack"), (["--verify-repack", y], "--verify-repack"),
                        (["--merge", "2"], "--merge"), (["--debug", "101"], "--debug"), (["--per-event"], "--per-event")):
        r = cli(*src.cli["dir"], "--survey", out, "--survey-planes", x, *extra)
        assert r.returncode != 0 and f"--survey cannot be combined with {word}" in r.stderr, (extra, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(x) and not os.path.exists(y)
    # the run's own directory is refused, as --repack refuses it
    r = cli(*src.cli["dir"], "--survey", out, "--survey-planes", os.path.dirname(src.rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(os.path.join(src.rd, "activity.txt"))
    assert not os.path.exists(out)
