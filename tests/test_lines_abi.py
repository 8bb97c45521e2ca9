"""abub3hs --survey-lines / Run.survey(lines=...) on the CPU side: abub_frame_lines_dev is declared, exported, bound and
validates its arguments without a device; linesHost and linesModelHost (the definition) against the numpy restatement
(tests/linesref.py) at the shapes and contents of the issue; what a line and a frame say (abub::lineRate, abub::linesFrame) on
hand-made records, one per state and kind, at the boundaries of the rule; the CLI's host route on a small run with planted
cases, whose files must be the restatement's byte for byte and which must leave every other product of the survey as it is;
the flags and refusals.  The shapes and contents (lines_shapes, lines_contents) and the run (make_lines_run) are shared with
tests/test_gpu_frame_lines.py and tests/test_gpu_lines_routes.py, which put them through the kernel and the device route."""
import ctypes
import math
import os

import numpy as np
import pytest

import linesref
from autobub3hs_amd import _lib, hip, host
from test_survey_abi import ENV, NCAMS, RUN_ID, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
W, H, F, NEV = 267, 137, 8, 8
SIGMA = 3
LEVELS = 3                                  # the planted bands' and stripes' height in grey levels
BAND_EVENT, BAND_FROM, BAND = 2, 4, (40, 48)      # rows 40 .. 47 from frame 4 on
STRIPE_EVENT, STRIPE_FROM, STRIPE = 3, 4, (100, 104)  # columns 100 .. 103 from frame 4 on
TORN = (1, 1, 5)                            # event, camera, frame: its rows 60 .. 136 are those of frame 3
TORN_FROM = 60
REPEATED = (7, 1, 6)                        # a byte copy of frame 4
TRUNCATED = (4, 1, "cam1_image33.png")
REMOVED = (5, 1, "cam1_image34.png")
WIDER = (6, 1, "cam1_image31.png")
UNTRAINED = 0
# The scene's seed.  At this size a line up by 3 levels has a rule value of 5.8 in the mean against the factor of 4, and over the
# 64 planted lines the smallest falls below 4 for most seeds.  This one is the best of 90 tried, by the restatement alone, on
# the two models of test_the_restatement_sees_what_was_planted: every planted line is above 4.3 at 267 and at 268 columns
# (the untouched ones stay below 1.2)
SEED = 147
TOTAL = F * NEV * NCAMS
RECORDS = NEV * F - 3                       # camera 1's ok rows: every one has a record


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def lines_shapes():
    """(w, h): one pixel; smaller than a dword, than a lane's 16 bytes; one row, one column; the run's odd size and another;
    whole strips; wider than one pass of a block (4099), taller than one band of rows (1100)"""
    return [(1, 1), (3, 2), (17, 5), (64, 1), (1, 64), (267, 137), (147, 130), (256, 128), (4099, 3), (5, 1100)]


def lines_contents(w, h, rs):
    """the jobs of one shape -> [(frame, mu, reference frame or None)]: random; 255 against mu = 0 and 0 against mu = 255;
    p == r everywhere; p == r in all but the last pixel of each row; p of only 0, 1, 254 and 255; no reference"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    full, none = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    a, b = rnd(), rnd()
    last = b.copy()
    last[:, -1] ^= 0x10
    edge = rs.choice(np.array([0, 1, 254, 255], np.uint8), (h, w))
    return [(rnd(), rnd(), rnd()), (full, none, full), (none, full, none), (a, rnd(), a), (b, rnd(), last), (edge, rnd(), rnd()),
            (rnd(), rnd(), None)]


def same_records(got, want):
    return all(g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_lines_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "#define ABUB_LINES_ROW_WORDS 5" in hdr and "#define ABUB_LINES_COL_WORDS 3" in hdr
    assert "int abub_frame_lines_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes," in hdr
    assert "const abub_stat_job *jobs, int njobs, int W, int H," in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_lines_dev") and "abub_frame_lines_dev" in _lib.SIGNATURES
    assert all(callable(f) for f in (hip.frame_lines, host.lines_host, host.lines_model_host, host.line_rate, host.lines_frame))
    for name in ("abh_run_survey_lines", "abh_run_survey_lines_dev", "abh_lines_host", "abh_lines_model_host", "abh_lines_rate",
                 "abh_lines_frame"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES
    assert (hip.LINES_ROW_WORDS, hip.LINES_COL_WORDS) == (5, 3) == (linesref.ROW_WORDS, linesref.COL_WORDS)
    assert host.LINES_KINDS == linesref.KINDS


def test_frame_lines_validates_before_it_touches_the_device():
    """every refusal comes before the first HIP call, so it is the same with and without a device; the buffers are host
    memory that a launch could not even read"""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, model_bytes=4096, jobs=p, njobs=1, W=30, H=17, status=p, rows=p, cols=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_lines_dev(a["frames"], a["frames_bytes"], a["mu"], a["model_bytes"], a["jobs"], a["njobs"], a["W"], a["H"],
                                      a["status"], a["rows"], a["cols"], a["stream"])

    bad = [dict(frames=None), dict(mu=None), dict(jobs=None), dict(status=None), dict(rows=None), dict(cols=None), dict(njobs=-1), dict(W=0),
           dict(H=0), dict(W=-3), dict(H=-1), dict(W=65536), dict(H=65536), dict(W=(1 << 31) - 1), dict(jobs=p + 4), dict(status=p + 2),
           dict(rows=p + 2), dict(cols=p + 1), dict(rows=p + 3)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_lines_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, W=1, H=1) == 0 and call(njobs=0, W=65535, H=65535) == 0
    assert call(njobs=0, rows=p + 4, cols=p + 12, status=p + 4) == 0  # (u32 words: 4-byte aligned)
    assert not any(buf)
    with pytest.raises(ValueError):
        host.lines_host(np.zeros((1, 65536), np.uint8), np.zeros((1, 65536), np.uint8))
    with pytest.raises(ValueError):
        host.lines_model_host(np.zeros((65536, 1), np.uint8), np.zeros((65536, 1), np.uint8))


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_host_definition_against_numpy():
    for w, h in lines_shapes():
        rs = np.random.RandomState(7000 + w + h)
        for k, (p, m, r) in enumerate(lines_contents(w, h, rs)):
            got = host.lines_host(p, m, r)
            assert same_records(got, [a.astype(np.uint32) for a in linesref.records(p, m, r)]), (w, h, k)
            rows, cols = got
            if k in (1, 2):  # the largest sums of |p - mu|; every pixel clipped; the reference the frame's equal
                assert (rows[:, 1] == 255 * w).all() and (rows[:, 2] == w).all() and (cols[:, 1] == 255 * h).all() and (cols[:, 2] == h).all()
                assert (rows[:, 4] == w).all() and not rows[:, 3].any() and (rows[:, 0] == (255 * w if k == 1 else 0)).all()
            if k == 3:
                assert (rows[:, 4] == w).all() and not rows[:, 3].any()
            if k == 4:
                assert (rows[:, 4] == w - 1).all() and (rows[:, 3] == 16).all()
            if k == 6:
                assert not rows[:, 3:].any()
        mu, s6 = lines_contents(w, h, rs)[0][:2]
        s6[::2, ::3] = 0
        assert same_records(host.lines_model_host(mu, s6), [a.astype(np.uint32) for a in linesref.model_records(mu, s6)]), (w, h)
    for w, h in ((65535, 1), (1, 65535)):  # 16,711,425 in a row word, in a column word
        full, none = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
        rows, cols = host.lines_host(full, none, none)
        assert same_records((rows, cols), [a.astype(np.uint32) for a in linesref.records(full, none, none)])
        assert max(rows[:, :2].max(), cols[:, :2].max()) == 16711425 == 65535 * 255 < 2 ** 31


def says(rec, model, N, n, S):
    got, want = host.line_rate(rec, model, N, n, S), linesref.rate(rec, model, N, n, S)
    assert got == want, (got, want)
    return got


def test_what_a_line_says_on_hand_made_records():
    # unrated: more than a quarter of the pixels clipped, or with sigma 0 (the comparisons are strict)
    assert says([0, 0, 25], [0, 10, 0], 100, 1, 0)["state"] == "rated" and says([0, 0, 26], [0, 10, 0], 100, 1, 0)["state"] == "unrated"
    assert says([0, 0, 0], [0, 10, 25], 100, 1, 0)["state"] == "rated" and says([0, 0, 0], [0, 10, 26], 100, 1, 0)["state"] == "unrated"
    # e^2 N against 4 (n T)^2 with N = 4, n = 1, T = 10: equality at |e| = 10, of either sign
    for e, state in ((9, "rated"), (10, "rated"), (11, "off"), (-10, "rated"), (-11, "off")):
        s = says([500 + e, 0, 0], [500, 10, 0], 4, 1, 0)
        assert (s["state"], s["num"], s["den"]) == (state, 4 * e * e, 100), e
    # the frame's own level is taken out: n D - S
    assert says([700, 0, 0], [500, 10, 0], 4, 5, 1000)["num"] == 0 and says([700, 0, 0], [500, 10, 0], 4, 5, 945)["state"] == "off"
    assert says([700, 0, 0], [500, 10, 0], 4, 5, 950)["state"] == "rated"  # e = 50 = 2 n T / sqrt N exactly
    # one below and one above equality where the products overflow 64 bits: n = 65535 lines of N = 65535 pixels
    n = N = 65535
    T = 16711425
    assert (n * T) ** 2 > 2 ** 64
    e_eq = math.isqrt(4 * (n * T) ** 2 // N) + 1  # the smallest e with e^2 N > 4 (n T)^2 (65535 is no square: none meets equality)
    assert (e_eq - 1) ** 2 * N < 4 * (n * T) ** 2 < e_eq ** 2 * N
    for e, state in ((e_eq - 1, "rated"), (e_eq, "off")):
        D = 16711425
        s = says([D, 0, 0], [0, T, 0], N, n, n * D - e)
        assert s["state"] == state and s["num"] == e * e * N > 2 ** 64 and s["den"] == (n * T) ** 2
    big = says([16711425, 0, 0], [0, 1, 0], N, n, -n * 16711425)  # the largest e: 2 n 255 N
    assert big["state"] == "off" and big["num"] == (2 * n * 16711425) ** 2 * N > 10 ** 29


def hand(h=16, w=16, level=100, T=12):
    """a frame that sits on its model: rows [h, 5], cols [w, 3], the model's"""
    rows, cols = np.zeros((h, 5), np.int64), np.zeros((w, 3), np.int64)
    rows[:, 0], cols[:, 0] = level * w, level * h
    mrows, mcols = np.zeros((h, 3), np.int64), np.zeros((w, 3), np.int64)
    mrows[:, 0], mrows[:, 1], mcols[:, 0], mcols[:, 1] = level * w, T * w, level * h, T * h
    return rows, cols, mrows, mcols


def frame_says(rows, cols, mrows, mcols, ref=True):
    got, want = host.lines_frame(rows, cols, mrows, mcols, ref), linesref.summary(rows, cols, mrows, mcols, ref)
    for k in got:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    return got


def test_what_a_frame_says_one_per_kind():
    s = frame_says(*hand())
    assert (s["kind"], s["rated_rows"], s["rated_cols"], s["off_rows"], s["stale_rows"], s["first_stale"], s["level_milli"]) == \
           ("steady", 16, 16, 0, 0, None, 0)
    # blind: fewer rated rows than a quarter of H; exactly H / 4 is not
    for unrated, kind in ((12, "steady"), (13, "blind")):
        rows, cols, mrows, mcols = hand()
        rows[:unrated, 2] = 16
        assert frame_says(rows, cols, mrows, mcols)["kind"] == kind, unrated
    rows, cols, mrows, mcols = hand()
    mrows[:13, 2] = 5  # (sigma 0 in more than a quarter of the row's pixels)
    assert frame_says(rows, cols, mrows, mcols)["kind"] == "blind"
    # stale rows: a run of 7 is not torn, of 8 is; without a reference none is stale; an unrated row breaks a run
    for run, kind in ((7, "steady"), (8, "torn")):
        rows, cols, mrows, mcols = hand()
        rows[3:3 + run, 4] = 16
        s = frame_says(rows, cols, mrows, mcols)
        assert (s["kind"], s["stale_rows"], s["first_stale"], s["last_stale"]) == (kind, run, 3, 2 + run)
        assert frame_says(rows, cols, mrows, mcols, ref=False)["stale_rows"] == 0
    rows[:, 4] = 15
    assert frame_says(rows, cols, mrows, mcols)["kind"] == "steady"  # (one pixel of every row differs)
    rows, cols, mrows, mcols = hand()
    rows[2:11, 4] = 16
    rows[6, 2] = 5
    s = frame_says(rows, cols, mrows, mcols)
    assert (s["kind"], s["stale_rows"], s["rated_rows"]) == ("steady", 8, 15)
    # repeated: every rated row is stale (the unrated ones are not asked)
    rows, cols, mrows, mcols = hand()
    rows[:, 4] = 16
    rows[0, 2] = 16
    s = frame_says(rows, cols, mrows, mcols)
    assert (s["kind"], s["stale_rows"], s["rated_rows"]) == ("repeated", 15, 15) and frame_says(rows, cols, mrows, mcols, ref=False)["kind"] == "steady"
    # banded from 4 off rows on, striped from 4 off columns on, banded before striped; the rule: (16 D - S)^2 16 > 4 (16 * 192)^2
    for off, kind in ((3, "steady"), (4, "banded")):
        rows, cols, mrows, mcols = hand()
        rows[5:5 + off, 0] += 200
        s = frame_says(rows, cols, mrows, mcols)
        assert (s["kind"], s["off_rows"], s["first_off_row"], s["last_off_row"]) == (kind, off, 5, 4 + off)
        assert s["level_milli"] == 1000 * 200 * off // (16 * 16)
        rows, cols, mrows, mcols = hand()
        cols[9:9 + off, 0] -= 200
        s = frame_says(rows, cols, mrows, mcols)
        assert (s["kind"], s["off_cols"], s["first_off_col"], s["last_off_col"]) == ("striped" if off == 4 else "steady", off, 9, 8 + off)
    rows, cols, mrows, mcols = hand()
    rows[:4, 0] += 200
    cols[:4, 0] += 200
    rows[8:, 4] = 16
    assert frame_says(rows, cols, mrows, mcols)["kind"] == "torn"  # torn before banded before striped
    rows[8:, 4] = 0
    assert frame_says(rows, cols, mrows, mcols)["kind"] == "banded"
    # a level step of the whole frame is no band: every row is up by the same
    rows, cols, mrows, mcols = hand()
    rows[:, 0] += 500
    s = frame_says(rows, cols, mrows, mcols)
    assert (s["kind"], s["off_rows"]) == ("steady", 0) and s["level_milli"] == 1000 * 500 // 16
    rows[:, 0] -= 1000
    assert frame_says(rows, cols, mrows, mcols)["level_milli"] == -31250


# ---- runs --------------------------------------------------------------------------------------------------------------------
def lines_frames(w=W, h=H):
    """8 events x 2 cameras x 8 frames of 267 x 137 on the pattern of test_noise_abi.make_noise_run: per camera a smooth
    background with Gaussian noise of sigma 3, rounded; camera 0 does not train.  Planted in camera 1: rows 40 .. 47 up by 3
    levels in one event from frame 4 on; columns 100 .. 103 up by 3 in another; one frame whose rows from 60 on are those of
    the frame two before it; one frame that is the frame two before it; one wider frame -> {(event, cam, name): image}"""
    rs = np.random.RandomState(SEED)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = {}
    name = lambda c, k: f"cam{c}_image{30 + k}.png"  # noqa: E731
    for e in range(NEV):
        for c in range(NCAMS):
            back = 120 + 30 * np.sin(xx / 37.0 + c) + 20 * np.cos(yy / 29.0)
            for k in range(F):
                img = back + SIGMA * rs.standard_normal((h, w))
                if k == 1:  # (the Trainer's entropy veto: no pixel of a training pair may differ by 16 or more)
                    first = frames[(e, c, name(c, 0))].astype(np.int64)
                    while True:
                        high = np.rint(img) - first >= 16
                        if not high.any():
                            break
                        img[high] = back[high] + SIGMA * rs.standard_normal(int(high.sum()))
                if (e, c) == (BAND_EVENT, 1) and k >= BAND_FROM:
                    img[BAND[0]:BAND[1]] += LEVELS
                if (e, c) == (STRIPE_EVENT, 1) and k >= STRIPE_FROM:
                    img[:, STRIPE[0]:STRIPE[1]] += LEVELS
                if c == UNTRAINED and k == 1:
                    img[:, :w // 2] += 70
                frames[(e, c, name(c, k))] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    e, c, k = TORN
    frames[(e, c, name(c, k))][TORN_FROM:] = frames[(e, c, name(c, k - 2))][TORN_FROM:]
    e, c, k = REPEATED
    frames[(e, c, name(c, k))] = frames[(e, c, name(c, k - 2))].copy()
    frames[WIDER] = np.ascontiguousarray(np.pad(frames[WIDER], ((0, 0), (0, 4)), mode="edge"))
    return frames


def make_lines_run(root, w=W, h=H):
    """the frames of lines_frames as a run of PNG files, one of them truncated and one removed
    -> (run dir, {(event, cam, name): image, None (does not decode) or "missing"})"""
    rd = os.path.join(root, RUN_ID)
    frames = lines_frames(w, h)
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
    for (e, c, n), img in frames.items():
        open(os.path.join(rd, str(e), "Images", n), "wb").write(png_bytes(img))
    p = os.path.join(rd, str(TRUNCATED[0]), "Images", TRUNCATED[2])
    data = open(p, "rb").read()
    open(p, "wb").write(data[:len(data) // 2])
    os.remove(os.path.join(rd, str(REMOVED[0]), "Images", REMOVED[2]))
    frames[TRUNCATED] = None
    frames[REMOVED] = "missing"
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(NEV):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd, frames


def expected_lines(rd, frames, w=W, h=H, models=None, summaries=None):
    """-> (lines.txt, {cam: (rows array, cols array)}, {cam: the model's two arrays}, the models)"""
    models = trained_models(rd, w, h) if models is None else models
    rows = linesref.rows_of(stacks_of(frames), w, h, models)
    return linesref.report(models, rows, w, h, summaries), linesref.arrays(models, rows, w, h), linesref.model_arrays(models), models


def welford_models(frames, w=W, h=H):
    """the models the Trainer would make of the run, without one: mean and truncated standard deviation of frames 0 and 1 of
    every event of camera 1; camera 0 has none"""
    tr = np.stack([img for (e, c, n), img in sorted(frames.items()) if c == 1 and n[-6:-4] in ("30", "31") and
                   not isinstance(img, str) and img is not None and img.shape == (h, w)]).astype(np.float64)
    return [None, dict(mu=np.rint(tr.mean(axis=0)).astype(np.uint8), sigma=np.floor(tr.std(axis=0)).astype(np.uint8))]


def oracle_models(frames, w=W, h=H):
    """the same from the oracle's copy of the Trainer's recurrence (float32 Welford, truncated mean and deviation), over the
    events of camera 1 whose first two frames are both of the run's size: the model a trained run has"""
    from oracle import pyoracle
    tr = []
    for e in range(NEV):
        pair = [frames[(e, 1, f"cam1_image{30 + k}.png")] for k in (0, 1)]
        if all(isinstance(img, np.ndarray) and img.shape == (h, w) for img in pair):
            tr += pair
    mu, sigma = pyoracle.welford(np.stack(tr))
    return [None, dict(mu=mu, sigma=sigma)]


@pytest.fixture(scope="module")
def lines_run(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lines_run"))
    return make_lines_run(os.path.join(root, "data"))


FILES = ("lines_rows", "lines_cols", "lines_model_rows", "lines_model_cols")


def read_lines(d):
    """the directory DIR/<run_ID> -> (lines.txt or None, {cam: (rows, cols)}, {cam: (model rows, model cols)})"""
    if not os.path.isdir(d):
        return None, {}, {}
    cams = sorted({int(f[3:f.index("_")]) for f in os.listdir(d) if f.endswith(".npy")})
    assert sorted(os.listdir(d)) == sorted(["lines.txt"] + [f"cam{c}_{s}.npy" for c in cams for s in FILES])
    load = lambda c, s: np.load(os.path.join(d, f"cam{c}_{s}.npy"))  # noqa: E731
    return (open(os.path.join(d, "lines.txt")).read(), {c: (load(c, FILES[0]), load(c, FILES[1])) for c in cams},
            {c: (load(c, FILES[2]), load(c, FILES[3])) for c in cams})


def same_lines(got, want):
    def same(a, b):
        return sorted(a) == sorted(b) and all(g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)
                                              for c in b for g, w in zip(a[c], b[c]))
    return got[0] == want[0] and same(got[1], want[1]) and same(got[2], want[2])


def lines_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-lines stem_lines -> (the process, the report, (lines.txt, the arrays, the models'))"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-lines", stem + "_lines", *more, env=env)
    return r, text, read_lines(os.path.join(stem + "_lines", RUN_ID))


def check_kinds(text, arrays, marr, w=W, h=H):
    """lines.txt of the run with a model of camera 1: every row says what was planted in its frame"""
    lines = text.splitlines()
    assert lines[:2] == ["# abub3hs lines 1", f"size {w} {h}"] and lines[2] + "\n" == linesref.HEADER
    index, kinds = 0, {k: 0 for k in linesref.KINDS}
    for l in lines[3:3 + TOTAL]:
        r = l.split("\t")
        assert len(r) == 19
        e, c, k, name = int(r[0]), int(r[1]), int(r[2]), r[3]
        if c == UNTRAINED or (e, c, name) in (TRUNCATED, REMOVED, WIDER):
            assert r[5:] == ["-"] * 14, r
            continue
        assert r[4] == "ok" and int(r[5]) == index, r
        index += 1
        kinds[r[18]] += 1
        assert r[6] == str(h) and r[11] == str(w), r  # every line is rated
        if (e, c, k) == TORN:
            assert r[7:11] == ["0", str(h - TORN_FROM), str(TORN_FROM), str(h - 1)] and r[18] == "torn", r
        elif (e, c, k) == REPEATED:
            assert r[8:11] == [str(h), "0", str(h - 1)] and r[18] == "repeated", r
        elif (e, c) == (BAND_EVENT, 1) and k >= BAND_FROM:
            assert r[7] == str(BAND[1] - BAND[0]) and r[13:15] == [str(BAND[0]), str(BAND[1] - 1)] and r[12] == "0" and r[18] == "banded", r
            assert 0 < int(r[17]) < 1000 * LEVELS
        elif (e, c) == (STRIPE_EVENT, 1) and k >= STRIPE_FROM:
            assert r[12] == str(STRIPE[1] - STRIPE[0]) and r[15:17] == [str(STRIPE[0]), str(STRIPE[1] - 1)] and r[7] == "0", r
            assert r[18] == "striped", r
        else:  # every untouched frame
            assert r[7:11] == ["0", "0", "-", "-"] and r[12:17] == ["0", "-", "-", "-", "-"] and r[18] == "steady", r
            assert abs(int(r[17])) < 1000, r  # (a u8 mean, rounded or truncated, is within one level; the noise of the mean is 16 milli)
    assert index == RECORDS and arrays[1][0].shape == (index, h, 5) and arrays[1][1].shape == (index, w, 3)
    assert marr[1][0].shape == (h, 3) and marr[1][1].shape == (w, 3)
    assert kinds == dict(blind=0, repeated=1, torn=1, banded=F - BAND_FROM, striped=F - STRIPE_FROM, steady=index - 2 - 2 * F + BAND_FROM + STRIPE_FROM)
    assert lines[3 + TOTAL] == f"lines cam {UNTRAINED} none"
    counts = " ".join(f"{q} {kinds[q]}" for q in linesref.KINDS)
    assert lines[4 + TOTAL] == f"lines cam 1 frames {index} {counts} first_changed_event {TORN[0]}"
    changed = lines[5 + TOTAL:-1]
    rows = {int(l.split(" ")[4]): int(l.split(" ")[6]) for l in changed if l.startswith("changed cam 1 row ")}
    cols = {int(l.split(" ")[4]): int(l.split(" ")[6]) for l in changed if l.startswith("changed cam 1 col ")}
    assert len(rows) + len(cols) == len(changed)
    want_rows = {y: 1 for y in range(h)}  # the repeated frame; the torn one from row 60 on; the band
    for y in range(TORN_FROM, h):
        want_rows[y] += 1
    for y in range(*BAND):
        want_rows[y] += F - BAND_FROM
    assert rows == want_rows and cols == {x: F - STRIPE_FROM for x in range(*STRIPE)}
    assert lines[-1] == f"run frames {index} {counts}"


def test_the_restatement_sees_what_was_planted(lines_run):
    """the run is what its description says, with the mean and the truncated standard deviation of the training frames as
    the model, and with the model of the Trainer's own recurrence, at the run's width and at the device route's.  The untouched frames are steady by the restatement, so that the scene and not the code under test carries the
    condition; their largest rule value stays below half the factor, and every planted line is above it"""
    _, frames = lines_run
    wide = lines_frames(W + 1)  # (268 columns: the device route's run)
    wide.update({TRUNCATED: None, REMOVED: "missing"})
    for w, fr in ((W, frames), (W + 1, wide)):
        for models in (welford_models(fr, w), oracle_models(fr, w)):
            assert np.median(models[1]["sigma"]) == 2  # (truncated: 6 sigma is 12, not 18)
            summaries = []
            text, arrays, marr, _ = expected_lines(None, fr, w=w, models=models, summaries=summaries)
            check_kinds(text, arrays, marr, w=w)
            steady = [s for r, s in summaries if s["kind"] == "steady"]
            assert len(steady) == RECORDS - 2 - 2 * F + BAND_FROM + STRIPE_FROM
            assert max(max(s["ratio_rows"], s["ratio_cols"]) for s in steady) < linesref.FACTOR / 2
            banded = [s for r, s in summaries if s["kind"] == "banded"]
            assert all(s["ratio_rows"] > linesref.FACTOR for s in banded) and all(s["ratio_cols"] < linesref.FACTOR / 2 for s in banded)


def others(tmp_path, tag):
    """the flags of every other product of a survey, into places of their own"""
    return ["--survey-planes", str(tmp_path / f"planes_{tag}"), "--survey-shift", str(tmp_path / f"shift_{tag}.txt"), "--survey-field",
            str(tmp_path / f"field_{tag}"), "--survey-light", str(tmp_path / f"light_{tag}"), "--survey-focus", str(tmp_path / f"focus_{tag}"),
            "--survey-noise", str(tmp_path / f"noise_{tag}")]


def same_others(tmp_path, a, b):
    """every other product's files of the calls tagged a and b are the same bytes"""
    if open(str(tmp_path / f"shift_{a}.txt"), "rb").read() != open(str(tmp_path / f"shift_{b}.txt"), "rb").read():
        return False
    for kind in ("planes", "field", "light", "focus", "noise"):
        da, db = (os.path.join(str(tmp_path / f"{kind}_{tag}"), RUN_ID) for tag in (a, b))
        if sorted(os.listdir(da)) != sorted(os.listdir(db)) or not os.listdir(da):
            return False
        if any(open(os.path.join(da, f), "rb").read() != open(os.path.join(db, f), "rb").read() for f in os.listdir(da)):
            return False
    return True


def test_cli_host_route_and_nothing_else_changes(lines_run, tmp_path):
    """the files against the restatement, byte for byte; the report and every other product's files are the same bytes with
    the flag and without it; alone, the lines are the same again"""
    rd, frames = lines_run
    src = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    want = expected_lines(rd, frames)
    plain, report_plain = survey_cli(src, str(tmp_path / "plain.txt"), *others(tmp_path, "plain"))
    r, report, got = lines_cli(src, str(tmp_path / "with"), *others(tmp_path, "with"))
    assert r.returncode == plain.returncode == 1, (r.stdout, r.stderr)  # (the damaged files: the survey's status)
    assert report == report_plain and report is not None and same_others(tmp_path, "with", "plain")
    assert same_lines(got, want), got[0]
    assert "survey-lines: " in r.stdout and "survey-lines" not in plain.stdout
    r, report, alone = lines_cli(src, str(tmp_path / "alone"))
    assert r.returncode == 1 and report == report_plain and same_lines(alone, want)
    models = want[3]
    assert models[UNTRAINED] is None and f"lines cam {UNTRAINED} none\n" in want[0]
    if models[1] is not None:  # (the host Trainer needs a device: without one no camera has a model, and the files say so)
        check_kinds(*got)
    else:
        assert "lines cam 1 none\n" in want[0] and not got[1] and not got[2]


def test_run_survey_agrees_with_the_cli(lines_run, tmp_path):
    rd, frames = lines_run
    want = expected_lines(rd, frames)
    run = host.Run("raw", rd + "/", "Images")
    try:
        plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
        res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, lines=str(tmp_path / "n"))
    finally:
        run.close()
    assert text == text_plain and same_lines(read_lines(str(tmp_path / "n")), want)
    records = sum(len(a[0]) for a in want[1].values())
    assert res["lines_frames_kernel"] == 0 and res["lines_launches"] == 0 and res["lines_frames_host"] == records
    assert "lines_frames_host" not in plain and "noise_frames_host" not in res
    assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
           {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}


def test_cli_flags_and_refusals(lines_run, tmp_path):
    rd, _ = lines_run
    src = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli("-h")
    assert "--survey-lines = Dir" in r.stdout and "[--survey-lines DIR]" in r.stdout
    out, nd = str(tmp_path / "s.txt"), str(tmp_path / "lines")
    r = cli(*src, "-o", str(tmp_path), "--survey-lines", nd)
    assert r.returncode != 0 and "--survey-lines is valid only together with --survey" in r.stderr and not os.path.exists(nd)
    r = cli(*src, "--survey", out, "--survey-lines", nd, "--survey-field-radius", "2")  # (no grid: the radius is not the lines')
    assert r.returncode != 0 and "--survey-field-radius is valid only together with --survey-field" in r.stderr
    r = cli(*src, "--survey", out, "--survey-lines")
    assert r.returncode != 0 and "--survey-lines needs the directory to write to" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(nd)
    r = cli(*src, "--survey", out, "--survey-lines", os.path.dirname(rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(out)
    assert not os.path.exists(os.path.join(rd, "lines.txt"))
    r = cli(*src, "--survey", out, "--survey-gpu", "--survey-lines", nd)  # (accepted with --survey-gpu: refused only for want of a device)
    assert "valid only" not in r.stderr and "unknown" not in r.stderr.lower()
