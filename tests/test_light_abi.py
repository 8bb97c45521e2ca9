"""abub3hs --survey-light / Run.survey(light=...) on the CPU side: abub_frame_light_cells_dev is declared, exported, bound and
validates its arguments without a device; lightCellsHost and lightModelHost (the definition) against the numpy restatement
(tests/lightref.py) and, cell by cell, against frameStatsHost of the cell's crop and fieldCellsHost's entry at (0, 0); what a
frame says (abub::lightFrame) against the restatement and against known answers, every one exact; the CLI's host route on a
small run that holds a level change, an uneven one, a saturated frame and a truncated file, in five source forms, which must
all give the files lightref gives and leave the survey's report, planes, shift file and field as they are; the flags and
refusals.  The sizes and contents (light_sizes, light_contents) and the run (make_light_run) are shared with
tests/test_gpu_frame_light.py and tests/test_gpu_light_routes.py, which put them through the kernel and the device route."""
import ctypes
import os

import numpy as np
import pytest

import fieldref
import lightref
import shiftref
from autobub3hs_amd import _lib, hip, host
from test_field_abi import field_sizes
from test_shift_abi import smooth_texture
from test_survey_abi import ENV, NCAMS, RUN_ID, Sources, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
C = lightref.CELL
N = C * C
W, H, F, NEV = 300, 170, 5, 5
TOTAL = F * NEV * NCAMS
GRID = (22, 21, 2, 1)  # x0, y0, ncx, ncy of 300 x 170 at R = 4
MARGIN = 8
STEP = 9  # grey levels: more than the 6 of a model with sigma 1
LEVEL = (1, 0, "cam0_image33.png")      # the whole frame brighter by STEP
UNEVEN = (2, 0, "cam0_image34.png")     # only the right cell brighter by STEP
SATURATED = (2, 1, "cam1_image33.png")  # all 255
TRUNCATED = (NEV - 1, 1, "cam1_image30.png")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def light_sizes():
    """(w, h, x0, y0, ncx, ncy) of the definition's and the kernel's tests: 128 x 128 with the grid at the origin, then the
    field's sizes at R = 4 on the field's grid: the origin at every residue mod 4, odd widths, grids of 2 x 1, 2 x 2 and
    3 x 1 cells"""
    out = [(C, C, 0, 0, 1, 1)]
    for w, h in field_sizes(4)[1:]:
        ncx, ncy, x0, y0 = fieldref.grid(w, h, 4)
        out.append((w, h, x0, y0, ncx, ncy))
    return out


def light_contents(w, h, rs):
    """the jobs of one size -> [(frame, model)]: random; a random frame against itself; a flat frame on a random model; 0
    against 255; 255 against 255; a frame of many 0 and 255 against a random model"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    a = rnd()
    full = np.full((h, w), 255, np.uint8)
    ends = rs.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (h, w))
    return [(rnd(), rnd()), (a, a.copy()), (np.full((h, w), 90, np.uint8), rnd()), (np.zeros((h, w), np.uint8), full), (full, full.copy()),
            (ends, rnd())]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_light_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_frame_light_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes," in hdr
    assert "const abub_shift_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy," in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_light_cells_dev") and "abub_frame_light_cells_dev" in _lib.SIGNATURES
    assert callable(hip.frame_light_cells) and callable(host.light_cells_host) and callable(host.light_model_host)
    for name in ("abh_run_survey_light", "abh_run_survey_light_dev", "abh_light_cells_host", "abh_light_model_host"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_frame_light_cells_validates_before_it_touches_the_device():
    """every refusal comes before the first HIP call, so it is the same with and without a device; the buffers are host
    memory that a launch could not even read"""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, model_bytes=4096, jobs=p, njobs=1, W=300, H=170, x0=22, y0=21, ncx=2, ncy=1, status=p,
              rec=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_light_cells_dev(a["frames"], a["frames_bytes"], a["mu"], a["model_bytes"], a["jobs"], a["njobs"], a["W"],
                                            a["H"], a["x0"], a["y0"], a["ncx"], a["ncy"], a["status"], a["rec"], a["stream"])

    bad = [dict(frames=None), dict(mu=None), dict(jobs=None), dict(status=None), dict(rec=None), dict(njobs=-1), dict(W=127, ncx=1, x0=0),
           dict(H=127, y0=0), dict(W=0), dict(H=-3), dict(W=65536), dict(H=65536), dict(ncx=0), dict(ncy=0), dict(ncx=-1), dict(ncy=-2),
           dict(x0=-1), dict(y0=-1), dict(x0=45), dict(y0=43), dict(ncx=3), dict(ncy=2), dict(ncx=1 << 24), dict(ncy=1 << 24),
           dict(x0=(1 << 31) - 1), dict(y0=(1 << 31) - 1), dict(jobs=p + 4), dict(rec=p + 2), dict(status=p + 2), dict(rec=p + 1)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_light_cells_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, x0=44, y0=42) == 0 and call(njobs=0, x0=0, y0=0) == 0 and call(njobs=0, W=128, H=128, x0=0, y0=0, ncx=1) == 0
    assert call(njobs=0, W=65535, H=65535, x0=127, y0=127, ncx=511, ncy=511) == 0
    assert call(njobs=0, rec=p + 4, status=p + 4) == 0  # (u32 words: 4-byte aligned)
    assert not any(buf)
    for fn in (host.light_cells_host, host.light_model_host):  # the host entries refuse a grid outside the frame too
        a = np.zeros((170, 300), np.uint8)
        for x0, y0, ncx, ncy in ((45, 21, 2, 1), (22, 43, 2, 1), (-1, 0, 1, 1), (0, 0, 0, 1), (0, 0, 3, 1), (0, 0, 1, 2)):
            with pytest.raises(ValueError):
                fn(a, a, x0, y0, ncx, ncy)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_rdiv_floors_toward_minus_infinity():
    assert [lightref.rdiv(a, 2) for a in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]
    assert lightref.rdiv(-7, 3) == -2 and lightref.rdiv(7, 3) == 2 and lightref.rdiv(-15, 10) == -1 and lightref.rdiv(15, 10) == 2


def test_host_definition_against_numpy_and_against_the_existing_definitions():
    sizes = light_sizes()
    assert len(sizes) == 8 and sorted({s[2] % 4 for s in sizes}) == [0, 1, 2, 3] and any(s[0] % 2 for s in sizes)
    assert {(s[4], s[5]) for s in sizes} == {(1, 1), (2, 1), (2, 2), (3, 1)}
    for w, h, x0, y0, ncx, ncy in sizes:
        rs = np.random.RandomState(4000 + w)
        s6 = rs.randint(0, 256, (h, w)).astype(np.uint8)
        for k, (p, m) in enumerate(light_contents(w, h, rs)):
            want = lightref.records(p, m, x0, y0, ncx, ncy)
            rec = host.light_cells_host(p, m, x0, y0, ncx, ncy)
            assert rec.dtype == np.uint32 and rec.shape == (ncy, ncx, 6) and np.array_equal(rec, want), (w, h, k)
            model = host.light_model_host(m, s6, x0, y0, ncx, ncy)
            assert model.dtype == np.uint32 and np.array_equal(model, lightref.model_records(m, s6, x0, y0, ncx, ncy)), (w, h, k)
            if k in (0, 5):  # other code, another decomposition: the crop's statistics, the field's surface at (0, 0)
                for cy in range(ncy):
                    for cx in range(ncx):
                        crop = p[y0 + C * cy:y0 + C * (cy + 1), x0 + C * cx:x0 + C * (cx + 1)]
                        s = host.frame_stats_host(crop)
                        assert [s["sum"], s["sumsq"], s["n_zero"], s["n_sat"]] == [int(rec[cy, cx, q]) for q in (0, 1, 4, 5)], (w, h, cx, cy)
                if (x0, y0) != (0, 0):
                    sad, _ = host.field_cells_host(p, m, 4)
                    assert np.array_equal(sad[:, :, 4, 4], rec[:, :, 3]), (w, h)
            if k == 1:
                assert not rec[..., 3].any() and np.array_equal(rec[..., 1], rec[..., 2])
            if k == 3:
                assert (rec == [0, 0, 0, 255 * N, N, 0]).all()
            if k == 4:  # the largest value a record can hold
                assert (rec == [255 * N, 1065369600, 1065369600, 0, 0, N]).all() and 255 * 255 * N == 1065369600 < 2 ** 31


def frame_says(p, m, sigma6):
    """the records of p against (m, sigma6) on the 2 x 1 grid of a 300 x 170 frame through the host's functions, what the
    frame says through abub::lightFrame, and the same from the restatement, which must agree"""
    x0, y0, ncx, ncy = GRID
    rec, model = host.light_cells_host(p, m, x0, y0, ncx, ncy), host.light_model_host(m, sigma6, x0, y0, ncx, ncy)
    assert np.array_equal(rec, lightref.records(p, m, x0, y0, ncx, ncy))
    assert np.array_equal(model, lightref.model_records(m, sigma6, x0, y0, ncx, ncy))
    got, want = host.light_frame(rec, model), lightref.summary(rec, model)
    assert got == {k: v for k, v in want.items() if k != "changed_cells"}, (got, want)
    return got, rec


def test_known_answers():
    rs = np.random.RandomState(5)
    six = np.full((H, W), 6, np.uint8)  # sigma = 1
    right = np.zeros((H, W), bool)
    right[:, GRID[0] + C:] = True  # the right cell (and what lies beyond it)
    m = rs.randint(7, 249, (H, W)).astype(np.uint8)
    same = dict(rated=2, clipped=0)
    # p = m: nothing changed, the fit is the identity
    s, _ = frame_says(m, m, six)
    assert s == dict(same, changed=0, up=0, down=0, kind="steady", level_milli=0, ratio_min=1000, ratio_max=1000, gain_milli=1000,
                     offset_milli=0)
    # a gain of 0.9 exactly: m of multiples of 10, p = 9 m / 10
    m10 = (10 * rs.randint(1, 26, (H, W))).astype(np.uint8)
    s, _ = frame_says((m10.astype(np.int64) * 9 // 10).astype(np.uint8), m10, six)
    assert (s["gain_milli"], s["offset_milli"], s["ratio_min"], s["ratio_max"]) == (900, 0, 900, 900) and s["down"] == 2 and s["kind"] == "level"
    # an offset of 7 against a mean 6 sigma of 6: every cell changed, upward
    s, _ = frame_says(m + 7, m, six)
    assert s["kind"] == "level" and (s["changed"], s["up"], s["down"]) == (2, 2, 0)
    assert (s["gain_milli"], s["offset_milli"], s["level_milli"]) == (1000, 7000, 7000)
    s, _ = frame_says(m - 7, m, six)
    assert s["kind"] == "level" and (s["changed"], s["up"], s["down"]) == (2, 0, 2) and s["level_milli"] == -7000 and s["offset_milli"] == -7000
    # ... of 6: the comparison is strict
    s, _ = frame_says(m + 6, m, six)
    assert s["kind"] == "steady" and s["changed"] == 0 and (s["gain_milli"], s["offset_milli"], s["level_milli"]) == (1000, 6000, 6000)
    # half of the cells
    s, _ = frame_says(np.where(right, m + 7, m).astype(np.uint8), m, six)
    assert s["kind"] == "uneven" and (s["changed"], s["up"], s["down"]) == (1, 1, 0) and s["level_milli"] == 3500
    # one half up, the other down: every cell changed, but not in one direction
    s, _ = frame_says(np.where(right, m + 7, m - 7).astype(np.uint8), m, six)
    assert s["kind"] == "uneven" and (s["changed"], s["up"], s["down"]) == (2, 1, 1) and s["level_milli"] == 0
    # a saturated frame: every cell clipped, none rated
    s, _ = frame_says(np.full((H, W), 255, np.uint8), m, six)
    assert s == dict(rated=0, clipped=2, changed=0, up=0, down=0, kind="blind", level_milli=None, ratio_min=None, ratio_max=None,
                     gain_milli=None, offset_milli=None)
    # one pixel more than N / 16 at 0 or 255 clips a cell, N / 16 does not
    p = m.copy()
    p[GRID[1], GRID[0]:GRID[0] + C] = 0
    p[GRID[1] + 1:GRID[1] + 8, GRID[0]:GRID[0] + C] = 255
    assert N // 16 == 8 * C
    s, rec = frame_says(p, m, six)
    assert (s["rated"], s["clipped"]) == (2, 0) and list(rec[0, 0, 4:]) == [C, 7 * C]
    p[GRID[1] + 8, GRID[0]] = 0
    s, _ = frame_says(p, m, six)
    assert (s["rated"], s["clipped"]) == (1, 1)
    # a dark model: no cell is rated or clipped
    s, _ = frame_says(m, np.zeros((H, W), np.uint8), six)
    assert s["kind"] == "blind" and (s["rated"], s["clipped"]) == (0, 0)
    # sm = N - 1: still not rated; sm = N: rated
    dim = np.ones((H, W), np.uint8)
    dim[GRID[1], GRID[0]] = 0
    s, _ = frame_says(dim, dim, six)
    assert (s["rated"], s["clipped"], s["kind"]) == (1, 0, "steady")
    # a flat model has no contrast to fit a gain to
    flat = np.full((H, W), 100, np.uint8)
    s, _ = frame_says(flat + 9, flat, six)
    assert s["kind"] == "level" and s["gain_milli"] is None and s["offset_milli"] is None and s["level_milli"] == 9000
    assert (s["ratio_min"], s["ratio_max"]) == (1090, 1090)
    # the largest product
    full = np.full((H, W), 255, np.uint8)
    _, rec = frame_says(full, full, six)
    assert (rec[..., 2] == 1065369600).all()


# ---- runs --------------------------------------------------------------------------------------------------------------------
def make_light_run(root, untrained_cam=None, w=W, h=H):
    """5 events x 2 cameras x 5 frames of 300 x 170 (at R = 4 a grid of 2 x 1 cells, origin 22, 21): per camera a smooth
    texture, one grey level of noise per frame: a steady stack.  One frame is brighter by STEP everywhere, one only in its
    right cell, one is all 255; one file is truncated.  untrained_cam: that camera's second frame differs from its first in
    every event, so the entropy veto leaves it no training frames.  Another size: the plain frames only
    -> (run dir, {(event, cam, name): image or None (does not decode)})"""
    rs = np.random.RandomState(37)
    rd = os.path.join(root, RUN_ID)
    tex = [shiftref.displaced(smooth_texture(h + 2 * MARGIN, w + 2 * MARGIN, 80 + c), 0, 0, w, h, MARGIN) for c in range(NCAMS)]
    special = (w, h) == (W, H)
    frames = {}
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for c in range(NCAMS):
            for k in range(F):
                key = (e, c, f"cam{c}_image{30 + k}.png")
                img = tex[c].astype(np.int16) + rs.randint(-1, 2, (h, w))
                if special and key == LEVEL:
                    img += STEP
                if special and key == UNEVEN:
                    img[:, GRID[0] + C:] += STEP
                if special and key == SATURATED:
                    img[:] = 255
                if c == untrained_cam and k == 1:
                    img[:, :w // 2] += 70
                frames[key] = np.clip(img, 0, 255).astype(np.uint8)
    for (e, c, name), img in frames.items():
        open(os.path.join(rd, str(e), "Images", name), "wb").write(png_bytes(img))
    if special:
        p = os.path.join(rd, str(TRUNCATED[0]), "Images", TRUNCATED[2])
        data = open(p, "rb").read()
        open(p, "wb").write(data[:len(data) // 2])
        frames[TRUNCATED] = None
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(NEV):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd, frames


def expected_light(rd, frames, R=4, w=W, h=H):
    """-> (light.txt, {cam: the array of cam<c>_light.npy}, {cam: that of cam<c>_light_model.npy}, the models)"""
    models = trained_models(rd, w, h)
    rows = lightref.rows_of(stacks_of(frames), w, h, models, R)
    marr = {c: a.astype(np.int32) for c, a in lightref.model_arrays(models, w, h, R).items()}
    return lightref.report(models, rows, w, h, R), lightref.arrays(models, rows, w, h, R), marr, models


@pytest.fixture(scope="module")
def lit(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("light_lit"))
    rd, frames = make_light_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def half_trained(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("light_half"))
    return make_light_run(os.path.join(root, "data"), untrained_cam=0)


def read_light(d):
    """the directory DIR/<run_ID> -> (light.txt or None, {cam: records}, {cam: model records})"""
    if not os.path.isdir(d):
        return None, {}, {}
    arrays = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_light.npy")}
    marr = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_light_model.npy")}
    assert sorted(arrays) == sorted(marr)
    assert sorted(os.listdir(d)) == sorted(["light.txt"] + [f"cam{c}_light{s}.npy" for c in arrays for s in ("", "_model")])
    return open(os.path.join(d, "light.txt")).read(), arrays, marr


def same_arrays(got, want):
    return sorted(got) == sorted(want) and all(got[c].dtype == np.int32 and got[c].shape == want[c].shape and np.array_equal(got[c], want[c])
                                              for c in want)


def light_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-light stem_light -> (the process, the report, light.txt, the arrays, the models')"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-light", stem + "_light", *more, env=env)
    return (r, text) + read_light(os.path.join(stem + "_light", RUN_ID))


def check_kinds(text, R=4):
    """light.txt of the lit run with models that are the scene at sigma 1: every row says what was done to its frame"""
    lines = text.splitlines()
    assert lines[:2] == ["# abub3hs light 1", f"radius {R} cell 128 grid 2 1 origin 22 21"] and lines[2] + "\n" == lightref.HEADER
    assert len(lines) == 3 + TOTAL + NCAMS + NCAMS * 1 + 1
    per_cam = [0] * NCAMS
    for l in lines[3:3 + TOTAL]:
        r = l.split("\t")
        assert len(r) == 17
        key = (int(r[0]), int(r[1]), r[3])
        if key == TRUNCATED:
            assert r[4:] == ["undecodable"] + ["-"] * 12
            continue
        assert r[4] == "ok" and int(r[5]) == per_cam[key[1]]
        per_cam[key[1]] += 1
        if key == SATURATED:
            assert r[6:] == ["0", "2", "0", "0", "0"] + ["-"] * 5 + ["blind"], r
        elif key == LEVEL:
            assert r[6:11] == ["2", "0", "2", "2", "0"] and r[16] == "level" and abs(int(r[11]) - 1000 * STEP) < 100, r
        elif key == UNEVEN:
            assert r[6:11] == ["2", "0", "1", "1", "0"] and r[16] == "uneven" and abs(int(r[11]) - 500 * STEP) < 100, r
        else:
            assert r[6:11] == ["2", "0", "0", "0", "0"] and r[16] == "steady" and abs(int(r[11])) < 100 and abs(int(r[14]) - 1000) < 10, r
    assert lines[3 + TOTAL] == f"light cam 0 frames {F * NEV} blind 0 steady {F * NEV - 2} level 1 uneven 1 first_changed_event 1"
    assert lines[4 + TOTAL] == f"light cam 1 frames {F * NEV - 1} blind 1 steady {F * NEV - 2} level 0 uneven 0 first_changed_event -"
    assert lines[5 + TOTAL:] == ["changed cam 0 y 0 1 2", "changed cam 1 y 0 0 0",
                                 f"run frames {TOTAL - 1} blind 1 steady {TOTAL - 4} level 1 uneven 1"]


def test_the_restatement_sees_the_light_change(lit):
    """the run is what its description says, with the textures themselves as the models and sigma 1"""
    _, frames = lit
    models = [dict(mu=shiftref.displaced(smooth_texture(H + 2 * MARGIN, W + 2 * MARGIN, 80 + c), 0, 0, W, H, MARGIN),
                   sigma=np.ones((H, W), np.uint8)) for c in range(NCAMS)]
    rows = lightref.rows_of(stacks_of(frames), W, H, models, 4)
    check_kinds(lightref.report(models, rows, W, H, 4))
    arrays = lightref.arrays(models, rows, W, H, 4)
    assert arrays[0].shape == (F * NEV, 1, 2, 6) and arrays[1].shape == (F * NEV - 1, 1, 2, 6)
    text = lightref.report([None, models[1]], lightref.rows_of(stacks_of(frames), W, H, [None, models[1]], 4), W, H, 4)
    assert text.count("light cam 0 none\n") == 1 and "changed cam 0" not in text and "changed cam 1 y 0" in text


def test_cli_host_route_on_every_source_form(lit, tmp_path):
    src, frames = lit
    want, want_arrays, want_models, models = expected_light(src.rd, frames)
    files = []
    for name in src.cli:
        others = lambda tag: ["--survey-planes", str(tmp_path / f"{name}_planes_{tag}"), "--survey-shift",  # noqa: E731
                              str(tmp_path / f"{name}_shift_{tag}.txt"), "--survey-field", str(tmp_path / f"{name}_field_{tag}")]
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / (name + "_plain.txt")), *others("plain"))
        r, report, text, arrays, marr = light_cli(src.cli[name], str(tmp_path / name), *others("with"))
        assert r.returncode == plain.returncode == 1, (name, r.stdout, r.stderr)  # (the truncated file: the survey's status)
        assert report == report_plain and report is not None, name  # the report, the shift file, the planes and the field do not change
        assert open(str(tmp_path / f"{name}_shift_with.txt")).read() == open(str(tmp_path / f"{name}_shift_plain.txt")).read()
        for kind in ("planes", "field"):
            with_flag, without = (os.path.join(str(tmp_path / f"{name}_{kind}_{tag}"), RUN_ID) for tag in ("with", "plain"))
            assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without)) and os.listdir(without)
            for f in os.listdir(without):
                assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(without, f), "rb").read(), (name, f)
        assert text == want and same_arrays(arrays, want_arrays) and same_arrays(marr, want_models), name
        assert "survey-light: " in r.stdout and "survey-light" not in plain.stdout
        files.append(text)
    assert len(files) == 5 and len(set(files)) == 1
    for c, m in enumerate(models):
        assert (f"light cam {c} none" in want.splitlines()) == (m is None) and (c in want_arrays) == (m is not None)
    # the field's radius is the light's, with and without the field: another grid line, here the same cells
    want8 = expected_light(src.rd, frames, 8)
    r, report, text, arrays, marr = light_cli(src.cli["dir"], str(tmp_path / "r8"), "--survey-field-radius", "8")
    assert r.returncode == 1 and text == want8[0] and same_arrays(arrays, want8[1]) and same_arrays(marr, want8[2]) and report == report_plain
    assert want8[0].splitlines()[1] == "radius 8 cell 128 grid 2 1 origin 22 21"
    want1 = expected_light(src.rd, frames, 1)
    r, report, text, arrays, marr = light_cli(src.cli["packed"], str(tmp_path / "r1"), "--survey-field-radius=1", "--survey-field",
                                              str(tmp_path / "r1_field"))
    assert r.returncode == 1 and text == want1[0] and same_arrays(arrays, want1[1]) and same_arrays(marr, want1[2])
    assert want1[0].splitlines()[1] == "radius 1 cell 128 grid 2 1 origin 22 21"
    assert open(str(tmp_path / "r1_field" / RUN_ID / "field.txt")).read().splitlines()[1] == want1[0].splitlines()[1]


def test_a_camera_that_does_not_train_has_no_light(half_trained, tmp_path):
    rd, frames = half_trained
    want, want_arrays, want_models, models = expected_light(rd, frames)
    assert models[0] is None
    r, report, text, arrays, marr = light_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "half"))
    assert r.returncode == 1 and text == want and same_arrays(arrays, want_arrays) and same_arrays(marr, want_models), (r.stdout, r.stderr)
    assert "light cam 0 none\n" in text and "survey: a camera did not train" in r.stdout and 0 not in arrays and 0 not in marr
    assert all(l.endswith("\t-" * 12) for l in text.splitlines()[3:3 + TOTAL] if l.split("\t")[1] == "0")


def test_run_survey_agrees_with_the_cli(lit, tmp_path):
    src, frames = lit
    want, want_arrays, want_models, models = expected_light(src.rd, frames)
    for name in ("dir", "deflated"):
        run = src.open(name)
        try:
            plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
            res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, light=str(tmp_path / "l"))
            res2, _ = run.survey(nthreads=4, ncams=NCAMS, light=str(tmp_path / "l2"), field=str(tmp_path / "f2"), field_radius=2,
                                 shift=str(tmp_path / "s2.txt"))
        finally:
            run.close()
        got = read_light(str(tmp_path / "l"))
        assert text == text_plain and got[0] == want and same_arrays(got[1], want_arrays) and same_arrays(got[2], want_models)
        want2 = expected_light(src.rd, frames, 2)
        got2 = read_light(str(tmp_path / "l2"))
        assert got2[0] == want2[0] and same_arrays(got2[1], want2[1]) and same_arrays(got2[2], want2[2])
        with_model = sum(1 for (e, c, n), img in frames.items() if img is not None and models[c] is not None)
        assert res["light_frames_kernel"] == 0 and res["light_launches"] == 0 and res["light_frames_host"] == with_model
        assert res2["light_frames_host"] == with_model == res2["shift_frames_host"] == res2["field_frames_host"]
        assert "light_frames_host" not in plain and "shift_frames_host" not in res and "field_frames_host" not in res
        assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
               {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}
    run = src.open("dir")
    try:
        with pytest.raises(RuntimeError, match="radius"):
            run.survey(nthreads=4, ncams=NCAMS, light=str(tmp_path / "bad"), field_radius=9)
    finally:
        run.close()
    assert not os.path.exists(str(tmp_path / "bad"))


def test_cli_flags_and_refusals(lit, tmp_path):
    src, _ = lit
    r = cli("-h")
    assert "--survey-light = Dir" in r.stdout and "[--survey-light DIR [--survey-field-radius R]]" in r.stdout
    out, ld, sh = str(tmp_path / "s.txt"), str(tmp_path / "light"), str(tmp_path / "shift.txt")
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-light", ld)
    assert r.returncode != 0 and "--survey-light is valid only together with --survey" in r.stderr and not os.path.exists(ld)
    # the shift's radius keeps its own refusal: the light does not make it valid
    r = cli(*src.cli["dir"], "--survey", out, "--survey-light", ld, "--survey-shift-radius", "2")
    assert r.returncode != 0 and "--survey-shift-radius is valid only together with --survey-shift" in r.stderr
    for radius in ("0", "9", "-1", "four", "4x"):
        r = cli(*src.cli["dir"], "--survey", out, "--survey-light", ld, "--survey-field-radius", radius)
        assert r.returncode != 0 and "--survey-field-radius expects a radius from 1 to 8" in r.stderr, radius
    r = cli(*src.cli["dir"], "--survey", out, "--survey-light")
    assert r.returncode != 0 and "--survey-light needs the directory to write to" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-light", ld, "--repack", str(tmp_path / "X"))
    assert r.returncode != 0 and "--survey cannot be combined with --repack" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(ld) and not os.path.exists(sh)
    # the run's own directory is no place for what was derived from it
    r = cli(*src.cli["dir"], "--survey", out, "--survey-light", os.path.dirname(src.rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(out)
    assert not os.path.exists(os.path.join(src.rd, "light.txt"))


def test_a_run_without_a_whole_cell_is_refused(tmp_path):
    rd, _ = make_light_run(str(tmp_path / "data"), w=42, h=140)
    out, ld = str(tmp_path / "s.txt"), str(tmp_path / "light")
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-light", ld)
    assert r.returncode != 0 and "need frames of at least 136x136, the run's are 42x140" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(ld)
    rd, _ = make_light_run(str(tmp_path / "data2"), w=135, h=200)
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-light", ld)
    assert r.returncode != 0 and "need frames of at least 136x136, the run's are 135x200" in r.stderr, r.stderr
    r = cli(*args, "--survey", out, "--survey-light", ld, "--survey-field-radius", "3")  # 135 = 128 + 2 * 3 + 1: one cell across
    assert r.returncode == 0 and os.path.exists(out), r.stderr
    assert open(os.path.join(ld, RUN_ID, "light.txt")).read().startswith("# abub3hs light 1\nradius 3 cell 128 grid 1 1 origin 3 36\n")
