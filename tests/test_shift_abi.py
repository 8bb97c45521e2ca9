"""abub3hs --survey-shift / Run.survey(shift=...) on the CPU side: abub_frame_shift_dev is declared, exported, bound and
validates its arguments without a device; frameShiftHost (the definition) and shiftBest (the tie rule) against the numpy
restatement (tests/shiftref.py); the CLI's host route on a small run whose camera moves, in five source forms, which must all
give the shift file shiftref gives and leave the survey's report as it is; the flags and refusals.
The contents (shift_contents) and the run (make_shift_run) are shared with tests/test_gpu_frame_shift.py and
tests/test_gpu_shift_routes.py, which put them through the kernel and the device route."""
import ctypes
import os

import numpy as np
import pytest

import shiftref
from autobub3hs_amd import _lib, hip, host
from test_survey_abi import ENV, NCAMS, RUN_ID, Sources, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
RADII = (1, 2, 4, 8)
W, H, F, NEV = 48, 32, 8, 3
TOTAL = F * NEV * NCAMS
MARGIN = 8
MOVED_STACK, MOVED_BY = (2, 1), (2, -1)           # every frame of event 2, camera 1
FAR, FAR_BY = (1, 0, "cam0_image35.png"), (6, 0)  # one frame beyond the default radius
# the truncated file is the first frame of the moved stack: the Trainer leaves an event without its frames 0 and 1 out, so
# camera 1's model is made of the two events in which it had not moved
TRUNCATED = (2, 1, "cam1_image30.png")


def sizes(R):
    """the sizes of the definition's tests: the smallest frame (an interior of one pixel), one column more, and widths
    around the dword, the wave (64 lanes x 4 pixels = 256 interior pixels) and odd ones; heights of a few rows"""
    return [(2 * R + 1, 2 * R + 1), (2 * R + 2, 2 * R + 1), (64, 20), (67, 19), (131, 21), (260, 18)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_frame_shift_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "typedef struct abub_shift_job { uint64_t cur, model; } abub_shift_job;" in hdr and "#define ABUB_SHIFT_E_RANGE 1\n" in hdr
    assert "int abub_frame_shift_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes," in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_shift_dev") and "abub_frame_shift_dev" in _lib.SIGNATURES
    assert callable(hip.frame_shift) and callable(host.frame_shift_host) and callable(host.shift_best)
    for name in ("abh_run_survey_shift", "abh_run_survey_shift_dev", "abh_frame_shift_host", "abh_shift_best"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_frame_shift_validates_before_it_touches_the_device():
    """every refusal comes before the first HIP call, so it is the same with and without a device; the buffers are host
    memory that a launch could not even read"""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, model_bytes=4096, jobs=p, njobs=1, W=16, H=12, R=4, status=p, sad=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_shift_dev(a["frames"], a["frames_bytes"], a["mu"], a["model_bytes"], a["jobs"], a["njobs"], a["W"], a["H"],
                                      a["R"], a["status"], a["sad"], a["stream"])

    bad = [dict(frames=None), dict(mu=None), dict(jobs=None), dict(status=None), dict(sad=None), dict(njobs=-1), dict(R=0), dict(R=9),
           dict(R=-1), dict(W=8), dict(H=8), dict(W=0), dict(H=-3), dict(W=65536), dict(H=65536), dict(R=1, W=2), dict(R=8, H=16),
           dict(jobs=p + 4), dict(sad=p + 4), dict(status=p + 2)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_shift_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, W=65535, H=65535, R=8) == 0 and call(njobs=0, W=9, H=9) == 0 and call(njobs=0, R=1, W=3, H=3) == 0
    assert call(njobs=0, status=p + 4) == 0
    assert not any(buf)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def shift_contents(w, h, R, rs):
    """the jobs of one size -> [(frame, model)]: random; all equal; 0 against 255; 255 against 0; a random frame against
    itself"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    full = lambda v: np.full((h, w), v, np.uint8)  # noqa: E731
    a = rnd()
    return [(rnd(), rnd()), (full(77), full(77)), (full(0), full(255)), (full(255), full(0)), (a, a.copy())]


def interior(w, h, R):
    return (w - 2 * R) * (h - 2 * R)


@pytest.mark.parametrize("R", RADII)
def test_host_definition_against_numpy(R):
    for w, h in sizes(R):
        rs = np.random.RandomState(1000 * R + w)
        for k, (p, m) in enumerate(shift_contents(w, h, R, rs)):
            want = shiftref.surface(p, m, R)
            got = host.frame_shift_host(p, m, R)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (R, w, h, k)
            b = shiftref.best(want, R)
            assert host.shift_best(got, R) == (b["dx"], b["dy"], b["at_edge"]), (R, w, h, k)
            if k == 1:  # all equal: the whole surface is one value and the best is (0, 0)
                assert (got == 0).all() and host.shift_best(got, R) == (0, 0, False)
            if k in (2, 3):  # every entry 255 |I|
                assert (got == 255 * interior(w, h, R)).all() and host.shift_best(got, R) == (0, 0, False)
    with pytest.raises(ValueError):
        host.frame_shift_host(np.zeros((2 * R, 2 * R + 1), np.uint8), np.zeros((2 * R, 2 * R + 1), np.uint8), R)


def test_host_definition_at_every_radius():
    rs = np.random.RandomState(55)
    for R in range(1, 9):
        for w, h in ((300, 2 * R + 6), (2 * R + 3, 2 * R + 2)):
            p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
            assert np.array_equal(host.frame_shift_host(p, m, R), shiftref.surface(p, m, R)), (R, w, h)


@pytest.mark.parametrize("R", (2, 4))
def test_a_planted_displacement_is_found(R):
    """a random texture; the frame is the model seen by a camera that moved by (dx, dy), every displacement in turn: the
    restatement finds it with sad_best 0, and the definition agrees with the restatement"""
    w, h = 37, 29
    tex = np.random.RandomState(5 + R).randint(0, 256, (h + 2 * R, w + 2 * R)).astype(np.uint8)
    model = shiftref.displaced(tex, 0, 0, w, h, R)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            frame = shiftref.displaced(tex, dx, dy, w, h, R)
            want = shiftref.surface(frame, model, R)
            b = shiftref.best(want, R)
            assert (b["dx"], b["dy"], b["sad_best"]) == (dx, dy, 0) and b["at_edge"] == (abs(dx) == R or abs(dy) == R)
            got = host.frame_shift_host(frame, model, R)
            assert np.array_equal(got, want) and host.shift_best(got, R) == (dx, dy, b["at_edge"]), (dx, dy)


def test_the_tie_order():
    """ties built by hand.  A frame equal to the model except in one uniform row: in the middle of the interior every
    displacement sees that row once, a tie of the whole surface; at the top only dy = -R sees it, a tie of all the others:
    (0, 0) wins both.  Then surfaces written down directly, one per clause of the rule."""
    R, w, h = 2, 12, 9
    model = np.full((h, w), 50, np.uint8)
    frame = model.copy()
    frame[4, :] = 60  # the middle row of the 5-row interior [2, 7): rows 2 .. 6 are summed, row 4 + dy is the bright one
    sad = host.frame_shift_host(frame, model, R)
    assert np.array_equal(sad, shiftref.surface(frame, model, R))
    assert (sad == 10 * (w - 2 * R)).all()  # every dy sees the bright row once: a tie of all 25
    assert host.shift_best(sad, R) == (0, 0, False) and shiftref.best(sad, R)["dx"] == 0
    frame[4, :] = 50
    frame[0, :] = 60  # seen only by dy = -2: every other entry is 0, a 20-way tie that (0, 0) wins
    sad = host.frame_shift_host(frame, model, R)
    assert np.array_equal(sad, shiftref.surface(frame, model, R)) and (sad[0] == 10 * (w - 2 * R)).all() and (sad[1:] == 0).all()
    assert host.shift_best(sad, R) == (0, 0, False)

    def best_of(entries, fill=9):
        s = np.full((2 * R + 1, 2 * R + 1), fill, np.uint64)
        for (dx, dy), v in entries.items():
            s[dy + R, dx + R] = v
        got = host.shift_best(s, R)
        b = shiftref.best(s, R)
        assert got == (b["dx"], b["dy"], b["at_edge"])
        return got[:2]

    assert best_of({(1, 1): 3, (2, 0): 3}) == (1, 1)            # the smaller dx^2 + dy^2 (2 against 4)
    assert best_of({(2, 0): 3, (1, 1): 3, (0, 0): 4}) == (1, 1)  # ... and a smaller value beats a nearer place
    assert best_of({(1, 0): 3, (0, 1): 3, (-1, 0): 3, (0, -1): 3}) == (0, -1)  # equal distance: the smaller dy
    assert best_of({(1, 0): 3, (-1, 0): 3}) == (-1, 0)           # equal distance and dy: the smaller dx
    assert best_of({(1, -1): 3, (-1, 1): 3, (1, 1): 3, (-1, -1): 3}) == (-1, -1)
    assert best_of({(2, 2): 0}) == (2, 2) and host.shift_best(np.zeros(25, np.uint64), R) == (0, 0, False)
    assert host.shift_best(np.array([0, 1, 1, 1, 1, 1, 1, 1, 1], np.uint64), 1) == (-1, -1, True)


# ---- runs --------------------------------------------------------------------------------------------------------------------
def smooth_texture(h, w, seed):
    """grey levels that change over about eight pixels (a coarse random grid, enlarged eight times and box-filtered), so
    that the sum of absolute differences grows with the distance from the true displacement for many pixels around it"""
    rs = np.random.RandomState(seed)
    coarse = rs.randint(20, 236, (h // 8 + 3, w // 8 + 3)).astype(np.float64)
    big = np.kron(coarse, np.ones((8, 8)))
    k = np.ones(8) / 8
    big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, big)
    big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, big)
    return np.round(big[:h, :w]).astype(np.uint8)


def make_shift_run(root, untrained_cam=None, w=W, h=H):
    """3 events x 2 cameras x 8 frames of 48 x 32: per camera a smooth texture seen through a window, one grey level of
    noise per frame.  Every frame of event 2, camera 1 is displaced by (+2, -1); frame 5 of event 1, camera 0 by (+6, 0),
    beyond a radius of 4; the first file of the moved stack is truncated.  untrained_cam: that camera's second frame differs from its first in
    every event, so the entropy veto leaves it no training frames
    -> (run dir, {(event, cam, name): image or None (does not decode)})"""
    rs = np.random.RandomState(23)
    rd = os.path.join(root, RUN_ID)
    tex = [smooth_texture(h + 2 * MARGIN, w + 2 * MARGIN, 40 + c) for c in range(NCAMS)]
    frames = {}
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for c in range(NCAMS):
            for k in range(F):
                key = (e, c, f"cam{c}_image{30 + k}.png")
                dx, dy = MOVED_BY if (e, c) == MOVED_STACK else FAR_BY if key == FAR else (0, 0)
                img = shiftref.displaced(tex[c], dx, dy, w, h, MARGIN).astype(np.int16) + rs.randint(-1, 2, (h, w))
                if c == untrained_cam and k == 1:
                    img[:, :w // 2] += 70
                frames[key] = np.clip(img, 0, 255).astype(np.uint8)
    for (e, c, name), img in frames.items():
        open(os.path.join(rd, str(e), "Images", name), "wb").write(png_bytes(img))
    if w == W:
        p = os.path.join(rd, str(TRUNCATED[0]), "Images", TRUNCATED[2])
        data = open(p, "rb").read()
        open(p, "wb").write(data[:len(data) // 2])
        frames[TRUNCATED] = None
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(NEV):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd, frames


def expected_shift(rd, frames, R, w=W, h=H):
    models = trained_models(rd, w, h)
    return shiftref.report(models, shiftref.rows_of(stacks_of(frames), w, h, models, R), R), models


@pytest.fixture(scope="module")
def moving(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("shift_moving"))
    rd, frames = make_shift_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def half_trained(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("shift_half"))
    return make_shift_run(os.path.join(root, "data"), untrained_cam=0)


def shift_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-shift stem.shift.txt -> (the process, the report, the shift file)"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-shift", stem + ".shift.txt", *more, env=env)
    return r, text, (open(stem + ".shift.txt").read() if os.path.exists(stem + ".shift.txt") else None)


def test_the_restatement_sees_the_run_move(moving):
    """the run is what its description says, with the textures themselves as the models: the restatement finds (0, 0)
    everywhere but in the moved stack, and the far frame on the edge of a radius of 4 and inside one of 8"""
    _, frames = moving
    models = [dict(mu=shiftref.displaced(smooth_texture(H + 2 * MARGIN, W + 2 * MARGIN, 40 + c), 0, 0, W, H, MARGIN)) for c in range(NCAMS)]
    rows = shiftref.rows_of(stacks_of(frames), W, H, models, 4)
    for r in rows:
        key = (int(r["event"]), r["cam"], r["name"])
        if key == TRUNCATED:
            assert r["state"] == "undecodable" and r["best"] is None
            continue
        got = (r["best"]["dx"], r["best"]["dy"], r["best"]["at_edge"])
        assert got == ((2, -1, False) if key[:2] == MOVED_STACK else (4, 0, True) if key == FAR else (0, 0, False)), (key, got)
    text = shiftref.report(models, rows, 4)
    assert text.startswith("# abub3hs shift 1\nradius 4\n" + shiftref.HEADER)
    assert f"shift cam 0 frames {F * NEV} at_zero {F * NEV - 1} shifted 1 at_edge 1 max_abs_dx 4 max_abs_dy 0 first_shifted_event 1\n" in text
    assert f"shift cam 1 frames {F * NEV - 1} at_zero {F * (NEV - 1)} shifted {F - 1} at_edge 0 max_abs_dx 2 max_abs_dy 1 first_shifted_event 2\n" in text
    assert text.endswith(f"run frames {TOTAL - 1} shifted {F} at_edge 1\n")
    far8 = [r for r in shiftref.rows_of(stacks_of(frames), W, H, models, 8) if (int(r["event"]), r["cam"], r["name"]) == FAR][0]["best"]
    assert (far8["dx"], far8["dy"], far8["at_edge"]) == (6, 0, False)
    assert shiftref.report([None, models[1]], shiftref.rows_of(stacks_of(frames), W, H, [None, models[1]], 4), 4).count("shift cam 0 none\n") == 1


def test_cli_host_route_on_every_source_form(moving, tmp_path):
    src, frames = moving
    want, models = expected_shift(src.rd, frames, 4)
    files = []
    for name in src.cli:
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / (name + "_plain.txt")))
        r, report, shift = shift_cli(src.cli[name], str(tmp_path / name))
        assert r.returncode == plain.returncode == 1, (name, r.stdout, r.stderr)  # (the truncated file: the survey's status)
        assert report == report_plain and report is not None, name  # the report does not change
        assert shift == want, name
        assert "survey-shift: " in r.stdout and "survey-shift" not in plain.stdout
        files.append(shift)
    assert len(files) == 5 and len(set(files)) == 1
    lines = want.splitlines()
    assert lines[:2] == ["# abub3hs shift 1", "radius 4"] and len(lines) == 3 + TOTAL + NCAMS + 1
    undecodable = [l for l in lines if l.startswith(f"{TRUNCATED[0]}\t{TRUNCATED[1]}\t0\t{TRUNCATED[2]}\tundecodable")]
    assert undecodable == [f"{TRUNCATED[0]}\t{TRUNCATED[1]}\t0\t{TRUNCATED[2]}\tundecodable" + "\t-" * 6]
    for c, m in enumerate(models):  # (without a GPU the host Trainer trains no camera: every row is `-`)
        assert (f"shift cam {c} none" in lines) == (m is None)
    # another radius: its own file, the same report
    want8, _ = expected_shift(src.rd, frames, 8)
    r, report, shift = shift_cli(src.cli["dir"], str(tmp_path / "r8"), "--survey-shift-radius", "8")
    assert r.returncode == 1 and shift == want8 and report == report_plain and want8.splitlines()[1] == "radius 8"
    r, report, shift = shift_cli(src.cli["packed"], str(tmp_path / "r1"), "--survey-shift-radius=1")
    assert r.returncode == 1 and shift == expected_shift(src.rd, frames, 1)[0]


def test_a_camera_that_does_not_train_has_no_shift_columns(half_trained, tmp_path):
    rd, frames = half_trained
    want, models = expected_shift(rd, frames, 4)
    assert models[0] is None
    r, report, shift = shift_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "half"))
    assert r.returncode == 1 and shift == want, (r.stdout, r.stderr)
    assert "shift cam 0 none\n" in shift and "survey: a camera did not train" in r.stdout
    assert all(l.endswith("\t-" * 6) for l in shift.splitlines()[3:3 + TOTAL] if l.split("\t")[1] == "0")


def test_run_survey_agrees_with_the_cli(moving, tmp_path):
    src, frames = moving
    want, models = expected_shift(src.rd, frames, 4)
    for name in ("dir", "deflated"):
        run = src.open(name)
        try:
            plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
            res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, shift=str(tmp_path / "s.txt"))
            res2, _ = run.survey(nthreads=4, ncams=NCAMS, shift=str(tmp_path / "s2.txt"), shift_radius=2)
        finally:
            run.close()
        assert text == text_plain and open(str(tmp_path / "s.txt")).read() == want
        assert open(str(tmp_path / "s2.txt")).read() == expected_shift(src.rd, frames, 2)[0]
        with_model = sum(1 for (e, c, n), img in frames.items() if img is not None and models[c] is not None)
        assert res["shift_frames_kernel"] == 0 and res["shift_launches"] == 0 and res["shift_frames_host"] == with_model
        assert res2["shift_frames_host"] == with_model and "shift_frames_host" not in plain
        assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
               {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}
    run = src.open("dir")
    try:
        with pytest.raises(RuntimeError, match="radius"):
            run.survey(nthreads=4, ncams=NCAMS, shift=str(tmp_path / "bad.txt"), shift_radius=9)
    finally:
        run.close()
    assert not os.path.exists(str(tmp_path / "bad.txt"))


def test_cli_flags_and_refusals(moving, tmp_path):
    src, _ = moving
    r = cli("-h")
    assert "--survey-shift = File" in r.stdout and "--survey-shift-radius = R" in r.stdout
    assert "[--survey-shift FILE [--survey-shift-radius R]]" in r.stdout
    out, sh = str(tmp_path / "s.txt"), str(tmp_path / "shift.txt")
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-shift", sh)
    assert r.returncode != 0 and "--survey-shift is valid only together with --survey" in r.stderr and not os.path.exists(sh)
    r = cli(*src.cli["dir"], "--survey", out, "--survey-shift-radius", "2")
    assert r.returncode != 0 and "--survey-shift-radius is valid only together with --survey-shift" in r.stderr
    for radius in ("0", "9", "-1", "four", "4x"):
        r = cli(*src.cli["dir"], "--survey", out, "--survey-shift", sh, "--survey-shift-radius", radius)
        assert r.returncode != 0 and "--survey-shift-radius expects a radius from 1 to 8" in r.stderr, radius
    r = cli(*src.cli["dir"], "--survey", out, "--survey-shift")
    assert r.returncode != 0 and "--survey-shift needs the file to write to" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-shift", sh, "--repack", str(tmp_path / "X"))
    assert r.returncode != 0 and "--survey cannot be combined with --repack" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(sh)


def test_a_run_smaller_than_the_search_is_refused(tmp_path):
    rd, _ = make_shift_run(str(tmp_path / "data"), w=7, h=7)
    out, sh = str(tmp_path / "s.txt"), str(tmp_path / "shift.txt")
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-shift", sh)
    assert r.returncode != 0 and "needs frames of at least 9x9, the run's are 7x7" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(sh)
    r = cli(*args, "--survey", out, "--survey-shift", sh, "--survey-shift-radius", "3")  # 7 = 2 * 3 + 1: an interior of one pixel
    assert r.returncode == 0 and os.path.exists(out) and open(sh).read().startswith("# abub3hs shift 1\nradius 3\n"), r.stderr
