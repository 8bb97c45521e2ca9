"""abub3hs --survey-field / Run.survey(field=...) on the CPU side: abub_frame_shift_cells_dev and abub_frame_cells_grid are
declared, exported, bound and validate their arguments without a device; the grid, fieldCellsHost (the definition) and a cell's
record against the numpy restatement (tests/fieldref.py) and, cell by cell, against frameShiftHost of the cell's crops; known
answers; the CLI's host route on a small run whose camera moves rigidly, locally and warped, in five source forms, which must
all give the files fieldref gives and leave the survey's report, planes and shift file as they are; the flags and refusals.
The sizes and contents (field_sizes, field_contents, planted) and the run (make_field_run) are shared with
tests/test_gpu_frame_field.py and tests/test_gpu_field_routes.py, which put them through the kernel and the device route."""
import ctypes
import os

import numpy as np
import pytest

import fieldref
import shiftref
from autobub3hs_amd import _lib, hip, host
from test_shift_abi import smooth_texture
from test_survey_abi import ENV, NCAMS, RUN_ID, Sources, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
RADII = (1, 2, 4, 8)
C = fieldref.CELL
W, H, F, NEV = 300, 170, 5, 5
TOTAL = F * NEV * NCAMS
MARGIN = 8
RIGID_STACK, RIGID_BY = (NEV - 1, 1), (2, -1)            # every frame of the last event, camera 1
# the truncated file is the first frame of the rigid stack: the Trainer leaves an event without its frames 0 and 1 out, so
# camera 1's model is made of the events in which it had not moved
TRUNCATED = (NEV - 1, 1, "cam1_image30.png")
LOCAL, LOCAL_BY = (1, 0, "cam0_image33.png"), ((0, 0), (3, 1))      # only the right cell is displaced
WARPED, WARPED_BY = (2, 0, "cam0_image34.png"), ((-2, 1), (2, -1))  # the two cells in opposite directions
FLAT = (2, 1, "cam1_image33.png")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def field_sizes(R):
    """W x H of the definition's and the kernel's tests: one cell with no margin; 2, 4 and 6 columns more, so that with the
    next the origin takes every residue mod 4; an odd width; two cells across with odd margins; a 2 x 2 and a 3 x 1 grid"""
    s = C + 2 * R
    return [(s, s), (s + 2, s), (s + 4, s + 1), (s + 6, s), (s + 3, s + 2), (2 * C + 2 * R + 5, s + 3), (2 * C + 2 * R + 1, 2 * C + 2 * R + 2),
            (3 * C + 2 * R + 7, s)]


def field_contents(w, h, rs):
    """the jobs of one size -> [(frame, model)]: random; a random frame against itself; a flat frame on a random model; 0
    against 255"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    a = rnd()
    return [(rnd(), rnd()), (a, a.copy()), (np.full((h, w), 90, np.uint8), rnd()), (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8))]


def composed(tex, w, h, R, moves, margin=MARGIN):
    """the w x h frame whose cell (cx, cy) shows the texture displaced by moves[cy][cx] = (dx, dy): the frame is cut along the
    cells' borders (the outer cells reach to the frame's edges)"""
    ncx, ncy, x0, y0 = fieldref.grid(w, h, R)
    assert len(moves) == ncy and all(len(row) == ncx for row in moves)
    out = np.zeros((h, w), np.uint8)
    xs = [0] + [x0 + C * k for k in range(1, ncx)] + [w]
    ys = [0] + [y0 + C * k for k in range(1, ncy)] + [h]
    for cy in range(ncy):
        for cx in range(ncx):
            dx, dy = moves[cy][cx]
            out[ys[cy]:ys[cy + 1], xs[cx]:xs[cx + 1]] = shiftref.displaced(tex, dx, dy, w, h, margin)[ys[cy]:ys[cy + 1], xs[cx]:xs[cx + 1]]
    return out


def planted(R, seed=17):
    """a 2 x 2 grid of random texture, each cell given its own displacement within R -> (frame, model, moves)"""
    w, h = 2 * C + 2 * R + 3, 2 * C + 2 * R + 4
    tex = np.random.RandomState(seed + R).randint(0, 256, (h + 2 * MARGIN, w + 2 * MARGIN)).astype(np.uint8)
    moves = [[(R, -1), (-1, R)], [(0, 0), (-R, 1 - R)]]
    return composed(tex, w, h, R, moves), shiftref.displaced(tex, 0, 0, w, h, MARGIN), moves


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_field_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "#define ABUB_FIELD_CELL 128\n" in hdr
    assert "int abub_frame_cells_grid(int W, int H, int R, int *ncx, int *ncy, int *x0, int *y0);" in hdr
    assert "int abub_frame_shift_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes," in hdr
    L = ctypes.CDLL(_lib.build())
    for name in ("abub_frame_shift_cells_dev", "abub_frame_cells_grid"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert callable(hip.frame_shift_cells) and callable(hip.field_grid) and callable(host.field_cells_host) and callable(host.field_grid)
    assert hip.FIELD_CELL == C
    for name in ("abh_run_survey_field", "abh_run_survey_field_dev", "abh_field_cells_host", "abh_field_grid"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_frame_shift_cells_validates_before_it_touches_the_device():
    """every refusal comes before the first HIP call, so it is the same with and without a device; the buffers are host
    memory that a launch could not even read"""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, model_bytes=4096, jobs=p, njobs=1, W=200, H=150, R=4, status=p, sad=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_shift_cells_dev(a["frames"], a["frames_bytes"], a["mu"], a["model_bytes"], a["jobs"], a["njobs"], a["W"],
                                            a["H"], a["R"], a["status"], a["sad"], a["stream"])

    bad = [dict(frames=None), dict(mu=None), dict(jobs=None), dict(status=None), dict(sad=None), dict(njobs=-1), dict(R=0), dict(R=9),
           dict(R=-1), dict(W=135), dict(H=135), dict(W=0), dict(H=-3), dict(W=65536), dict(H=65536), dict(R=1, W=129), dict(R=8, H=143),
           dict(jobs=p + 4), dict(sad=p + 2), dict(status=p + 2), dict(sad=p + 1)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_shift_cells_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, W=65535, H=65535, R=8) == 0 and call(njobs=0, W=136, H=136) == 0 and call(njobs=0, R=1, W=130, H=130) == 0
    assert call(njobs=0, sad=p + 4) == 0  # (a u32 surface: 4-byte aligned)
    assert not any(buf)
    out = [ctypes.c_int(7) for _ in range(4)]
    refs = [ctypes.byref(v) for v in out]
    assert L.abub_frame_cells_grid(300, 170, 0, *refs) == E_INVALID and L.abub_frame_cells_grid(300, 170, 9, *refs) == E_INVALID
    assert L.abub_frame_cells_grid(-1, 170, 4, *refs) == E_INVALID and L.abub_frame_cells_grid(300, 170, 4, None, *refs[1:]) == E_INVALID
    assert [v.value for v in out] == [7] * 4


def test_the_grid():
    """the one copy of the rule (the GPU library's, and through the host library) against the restatement, and by hand"""
    assert fieldref.grid(300, 170, 4) == (2, 1, 22, 21) and fieldref.grid(1680, 1050, 4) == (13, 8, 8, 13)
    assert fieldref.grid(1680, 1050, 8) == (13, 8, 8, 13) and fieldref.grid(136, 136, 4) == (1, 1, 4, 4)
    assert fieldref.grid(135, 200, 4) == (0, 1, 67, 36)
    for R in range(1, 9):
        sizes = field_sizes(R) + [(C + 2 * R - 1, 400), (400, C + 2 * R - 1), (1, 1), (0, 0), (2 * R - 1, 5), (1680, 1050), (65535, 65535)]
        for w, h in sizes + [(w + k, h + k) for w, h in field_sizes(R) for k in (1, 127, 128)]:
            want = fieldref.grid(w, h, R)
            assert hip.field_grid(w, h, R) == want and host.field_grid(w, h, R) == want, (w, h, R)
            ncx, ncy, x0, y0 = want
            if ncx * ncy:  # whole cells with their halo inside the frame, centred to within a pixel
                assert x0 >= R and x0 + C * ncx + R <= w and y0 >= R and y0 + C * ncy + R <= h
                assert 0 <= (w - (x0 + C * ncx)) - x0 <= 1 and 0 <= (h - (y0 + C * ncy)) - y0 <= 1
    assert sorted(fieldref.grid(w, h, 4)[2] % 4 for w, h in field_sizes(4)[:4]) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        host.field_grid(300, 170, 9)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def check_against_crops(p, m, R, sad):
    """every cell's surface is frameShiftHost of the cell's two crops (existing code, another decomposition)"""
    h, w = p.shape
    for cy in range(sad.shape[0]):
        for cx in range(sad.shape[1]):
            crops = [fieldref.crop(a, w, h, R, cx, cy) for a in (p, m)]
            assert crops[0].shape == (C + 2 * R, C + 2 * R)
            assert np.array_equal(host.frame_shift_host(crops[0], crops[1], R), sad[cy, cx].astype(np.uint64)), (R, w, h, cx, cy)


@pytest.mark.parametrize("R", RADII)
def test_host_definition_against_numpy_and_against_the_frame_search_on_crops(R):
    for w, h in field_sizes(R):
        rs = np.random.RandomState(1000 * R + w)
        ncx, ncy, _, _ = fieldref.grid(w, h, R)
        for k, (p, m) in enumerate(field_contents(w, h, rs)):
            want = fieldref.surfaces(p, m, R)
            sad, rec = host.field_cells_host(p, m, R)
            assert sad.dtype == np.uint32 and sad.shape == (ncy, ncx, 2 * R + 1, 2 * R + 1) and np.array_equal(sad, want), (R, w, h, k)
            assert rec.dtype == np.int32 and np.array_equal(rec, fieldref.records(want, R)), (R, w, h, k)
            s = fieldref.summary(rec)
            if k == 0:
                check_against_crops(p, m, R, sad)
            if k == 1:  # p = m: every cell still, with sad_best 0
                assert s["kind"] == "still" and s["rated"] == ncx * ncy and (rec[..., :2] == 0).all() and (rec[..., 2:4] == 0).all()
            if k == 2:  # a flat frame: every displacement of a cell scores alike, no cell is rated
                assert s["kind"] == "blind" and (sad == sad[:, :, :1, :1]).all() and (rec[..., 3] == rec[..., 4]).all()
            if k == 3:
                assert (sad == 4177920).all() and s["kind"] == "blind" and 4177920 == 255 * C * C
    small = np.zeros((C + 2 * R - 1, C + 2 * R), np.uint8)
    with pytest.raises(ValueError):
        host.field_cells_host(small, small, R)


def test_host_definition_at_every_radius():
    rs = np.random.RandomState(56)
    for R in range(1, 9):
        w, h = 2 * C + 2 * R + 5, C + 2 * R + 3
        p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
        sad, rec = host.field_cells_host(p, m, R)
        assert np.array_equal(sad, fieldref.surfaces(p, m, R)) and np.array_equal(rec, fieldref.records(sad, R)), R


@pytest.mark.parametrize("R", (2, 4, 8))
def test_planted_displacements_cell_by_cell(R):
    """each cell of a 2 x 2 grid shows the texture displaced by its own (dx, dy).  A cell reads up to R pixels of its
    neighbours, so its best sum is not 0; the restatement finds every planted displacement, rates every cell, and calls the
    frame local (one cell stayed); the definition agrees with the restatement"""
    frame, model, moves = planted(R)
    want = fieldref.records(fieldref.surfaces(frame, model, R), R)
    for cy in range(2):
        for cx in range(2):
            assert tuple(want[cy, cx, :2]) == moves[cy][cx] and fieldref.rated(want[cy, cx]), (cx, cy, want[cy, cx])
    s = fieldref.summary(want)
    assert (s["kind"], s["rated"], s["moved"]) == ("local", 4, 3) and s["ranges"] == (-R, R, min(-1, 1 - R), R)
    assert s["modal"] == (0, 0, 1)  # four displacements, each once: the nearest
    sad, rec = host.field_cells_host(frame, model, R)
    assert np.array_equal(rec, want) and np.array_equal(sad, fieldref.surfaces(frame, model, R))


def test_kinds_and_the_modal_displacement():
    """records written down directly, one per clause of the frame's kind and of the modal tie rule"""
    def rec(*cells):  # (dx, dy, rated)
        return np.array([[[dx, dy, 50, 10 if ok else 40, 60] for dx, dy, ok in cells]], np.int32)

    assert fieldref.summary(rec((1, 1, False), (0, 0, False)))["kind"] == "blind"
    assert fieldref.summary(rec((0, 0, True), (3, 3, False)))["kind"] == "still"
    assert fieldref.summary(rec((2, -1, True), (2, -1, True), (0, 0, False)))["kind"] == "rigid"
    assert fieldref.summary(rec((2, -1, True), (2, 0, True)))["kind"] == "warped"
    assert fieldref.summary(rec((2, -1, True), (0, 0, True)))["kind"] == "local"
    s = fieldref.summary(rec((2, 0, True), (1, 1, True), (2, 0, True), (1, 1, True), (0, 0, True)))
    assert s["modal"] == (1, 1, 2) and s["ranges"] == (0, 2, 0, 1) and (s["rated"], s["moved"]) == (5, 4)  # the nearer of two pairs
    assert fieldref.summary(rec((1, 0, True), (0, -1, True)))["modal"] == (0, -1, 1)   # equal distance: the smaller dy
    assert fieldref.summary(rec((1, 0, True), (-1, 0, True)))["modal"] == (-1, 0, 1)   # ... then the smaller dx
    assert not fieldref.rated([0, 0, 0, 0, 0]) and fieldref.rated([0, 0, 0, 0, 1]) and fieldref.rated([0, 0, 9, 5, 10])
    assert not fieldref.rated([0, 0, 9, 6, 11])


# ---- runs --------------------------------------------------------------------------------------------------------------------
def make_field_run(root, untrained_cam=None, w=W, h=H, R=4):
    """5 events x 2 cameras x 5 frames of 300 x 170 (at R = 4 a grid of 2 x 1 cells, origin 22, 21): per camera a smooth
    texture seen through a window, one grey level of noise per frame.  Every frame of the last event, camera 1 is displaced
    by (+2, -1); one frame has only its right cell displaced, one has the two cells displaced in opposite directions, one is
    flat; the first file of the rigid stack is truncated.  untrained_cam: that camera's second frame differs from its first
    in every event, so the entropy veto leaves it no training frames.  Another size: the plain frames only
    -> (run dir, {(event, cam, name): image or None (does not decode)})"""
    rs = np.random.RandomState(29)
    rd = os.path.join(root, RUN_ID)
    tex = [smooth_texture(h + 2 * MARGIN, w + 2 * MARGIN, 60 + c) for c in range(NCAMS)]
    special = (w, h) == (W, H)
    frames = {}
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for c in range(NCAMS):
            for k in range(F):
                key = (e, c, f"cam{c}_image{30 + k}.png")
                if special and key in (LOCAL, WARPED):
                    img = composed(tex[c], w, h, R, [list(LOCAL_BY if key == LOCAL else WARPED_BY)])
                elif special and key == FLAT:
                    img = np.full((h, w), 128, np.uint8)
                else:
                    dx, dy = RIGID_BY if special and (e, c) == RIGID_STACK else (0, 0)
                    img = shiftref.displaced(tex[c], dx, dy, w, h, MARGIN)
                img = img.astype(np.int16) + rs.randint(-1, 2, (h, w))
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


def expected_field(rd, frames, R, w=W, h=H):
    """-> (field.txt, {cam: the array of cam<c>_field.npy}, the models)"""
    models = trained_models(rd, w, h)
    rows = fieldref.rows_of(stacks_of(frames), w, h, models, R)
    return fieldref.report(models, rows, w, h, R), fieldref.arrays(models, rows, w, h, R), models


@pytest.fixture(scope="module")
def moving(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("field_moving"))
    rd, frames = make_field_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def half_trained(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("field_half"))
    return make_field_run(os.path.join(root, "data"), untrained_cam=0)


def read_field(d):
    """the directory DIR/<run_ID> -> (field.txt or None, {cam: array})"""
    if not os.path.isdir(d):
        return None, {}
    arrays = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_field.npy")}
    assert sorted(os.listdir(d)) == sorted(["field.txt"] + [f"cam{c}_field.npy" for c in arrays])
    return open(os.path.join(d, "field.txt")).read(), arrays


def same_arrays(got, want):
    return sorted(got) == sorted(want) and all(got[c].dtype == np.int32 and got[c].shape == want[c].shape and np.array_equal(got[c], want[c])
                                              for c in want)


def field_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-field stem_field -> (the process, the report, field.txt, the arrays)"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-field", stem + "_field", *more, env=env)
    return (r, text) + read_field(os.path.join(stem + "_field", RUN_ID))


def check_kinds(text, R=4):
    """field.txt of the moving run with models that are the scene: every row says what was done to its frame"""
    lines = text.splitlines()
    assert lines[:2] == ["# abub3hs field 1", f"radius {R} cell 128 grid 2 1 origin 22 21"] and lines[2] + "\n" == fieldref.HEADER
    assert len(lines) == 3 + TOTAL + NCAMS + NCAMS * 1 + 1
    per_cam = [0] * NCAMS
    for l in lines[3:3 + TOTAL]:
        r = l.split("\t")
        key = (int(r[0]), int(r[1]), r[3])
        if key == TRUNCATED:
            assert r[4:] == ["undecodable"] + ["-"] * 11
            continue
        assert r[4] == "ok" and int(r[5]) == per_cam[key[1]]
        per_cam[key[1]] += 1
        if key == FLAT:
            assert r[6:] == ["0", "0"] + ["-"] * 7 + ["blind"], r
        elif key == LOCAL:
            assert r[6:] == ["2", "1", "0", "0", "1", "0", "3", "0", "1", "local"], r
        elif key == WARPED:
            assert r[6:] == ["2", "2", "2", "-1", "1", "-2", "2", "-1", "1", "warped"], r
        elif key[:2] == RIGID_STACK:
            assert r[6:] == ["2", "2", "2", "-1", "2", "2", "2", "-1", "-1", "rigid"], r
        else:
            assert r[6:] == ["2", "0", "0", "0", "2", "0", "0", "0", "0", "still"], r
    assert lines[3 + TOTAL] == f"field cam 0 frames {F * NEV} blind 0 still {F * NEV - 2} rigid 0 warped 1 local 1 first_moved_event 1"
    assert lines[4 + TOTAL] == (f"field cam 1 frames {F * NEV - 1} blind 1 still {F * (NEV - 1) - 1} rigid {F - 1} warped 0 local 0 "
                                f"first_moved_event {NEV - 1}")
    assert lines[5 + TOTAL:] == ["moved cam 0 y 0 1 2", f"moved cam 1 y 0 {F - 1} {F - 1}",
                                 f"run frames {TOTAL - 1} blind 1 still {TOTAL - 3 - F} rigid {F - 1} warped 1 local 1"]


def test_the_restatement_sees_the_run_move(moving):
    """the run is what its description says, with the textures themselves as the models"""
    _, frames = moving
    models = [dict(mu=shiftref.displaced(smooth_texture(H + 2 * MARGIN, W + 2 * MARGIN, 60 + c), 0, 0, W, H, MARGIN)) for c in range(NCAMS)]
    rows = fieldref.rows_of(stacks_of(frames), W, H, models, 4)
    check_kinds(fieldref.report(models, rows, W, H, 4))
    arrays = fieldref.arrays(models, rows, W, H, 4)
    assert arrays[0].shape == (F * NEV, 1, 2, 5) and arrays[1].shape == (F * NEV - 1, 1, 2, 5)
    text = fieldref.report([None, models[1]], fieldref.rows_of(stacks_of(frames), W, H, [None, models[1]], 4), W, H, 4)
    assert text.count("field cam 0 none\n") == 1 and "moved cam 0" not in text and "moved cam 1 y 0" in text


def test_cli_host_route_on_every_source_form(moving, tmp_path):
    src, frames = moving
    want, want_arrays, models = expected_field(src.rd, frames, 4)
    if all(m is not None for m in models):  # (without a GPU the host Trainer trains no camera: every row is `-`)
        check_kinds(want)
    files = []
    for name in src.cli:
        others = ["--survey-planes", str(tmp_path / (name + "_planes")), "--survey-shift", str(tmp_path / (name + "_shift.txt"))]
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / (name + "_plain.txt")), "--survey-planes",
                                         str(tmp_path / (name + "_planes_plain")), "--survey-shift", str(tmp_path / (name + "_shift_plain.txt")))
        r, report, text, arrays = field_cli(src.cli[name], str(tmp_path / name), *others)
        assert r.returncode == plain.returncode == 1, (name, r.stdout, r.stderr)  # (the truncated file: the survey's status)
        assert report == report_plain and report is not None, name  # the report, the shift file and the planes do not change
        assert open(str(tmp_path / (name + "_shift.txt"))).read() == open(str(tmp_path / (name + "_shift_plain.txt"))).read()
        with_flag, without = (os.path.join(str(tmp_path / (name + s)), RUN_ID) for s in ("_planes", "_planes_plain"))
        assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without)) and os.listdir(without)
        for f in os.listdir(without):
            assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(without, f), "rb").read(), (name, f)
        assert text == want and same_arrays(arrays, want_arrays), name
        assert "survey-field: " in r.stdout and "survey-field" not in plain.stdout
        files.append(text)
    assert len(files) == 5 and len(set(files)) == 1
    for c, m in enumerate(models):
        assert (f"field cam {c} none" in want.splitlines()) == (m is None) and (c in want_arrays) == (m is not None)
    # another radius: its own files, the same report
    want8, arrays8, _ = expected_field(src.rd, frames, 8)
    r, report, text, arrays = field_cli(src.cli["dir"], str(tmp_path / "r8"), "--survey-field-radius", "8")
    assert r.returncode == 1 and text == want8 and same_arrays(arrays, arrays8) and report == report_plain
    assert want8.splitlines()[1] == "radius 8 cell 128 grid 2 1 origin 22 21"
    r, report, text, arrays = field_cli(src.cli["packed"], str(tmp_path / "r1"), "--survey-field-radius=1")
    want1, arrays1, _ = expected_field(src.rd, frames, 1)
    assert r.returncode == 1 and text == want1 and same_arrays(arrays, arrays1)


def test_a_camera_that_does_not_train_has_no_field(half_trained, tmp_path):
    rd, frames = half_trained
    want, want_arrays, models = expected_field(rd, frames, 4)
    assert models[0] is None
    r, report, text, arrays = field_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "half"))
    assert r.returncode == 1 and text == want and same_arrays(arrays, want_arrays), (r.stdout, r.stderr)
    assert "field cam 0 none\n" in text and "survey: a camera did not train" in r.stdout and 0 not in arrays
    assert all(l.endswith("\t-" * 11) for l in text.splitlines()[3:3 + TOTAL] if l.split("\t")[1] == "0")


def test_run_survey_agrees_with_the_cli(moving, tmp_path):
    src, frames = moving
    want, want_arrays, models = expected_field(src.rd, frames, 4)
    for name in ("dir", "deflated"):
        run = src.open(name)
        try:
            plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
            res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, field=str(tmp_path / "f"))
            res2, _ = run.survey(nthreads=4, ncams=NCAMS, field=str(tmp_path / "f2"), field_radius=2, shift=str(tmp_path / "s2.txt"))
        finally:
            run.close()
        got = read_field(str(tmp_path / "f"))
        assert text == text_plain and got[0] == want and same_arrays(got[1], want_arrays)
        want2 = expected_field(src.rd, frames, 2)
        got2 = read_field(str(tmp_path / "f2"))
        assert got2[0] == want2[0] and same_arrays(got2[1], want2[1])
        with_model = sum(1 for (e, c, n), img in frames.items() if img is not None and models[c] is not None)
        assert res["field_frames_kernel"] == 0 and res["field_launches"] == 0 and res["field_frames_host"] == with_model
        assert res2["field_frames_host"] == with_model == res2["shift_frames_host"] and "field_frames_host" not in plain
        assert "shift_frames_host" not in res
        assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
               {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}
    run = src.open("dir")
    try:
        with pytest.raises(RuntimeError, match="radius"):
            run.survey(nthreads=4, ncams=NCAMS, field=str(tmp_path / "bad"), field_radius=9)
    finally:
        run.close()
    assert not os.path.exists(str(tmp_path / "bad"))


def test_cli_flags_and_refusals(moving, tmp_path):
    src, _ = moving
    r = cli("-h")
    assert "--survey-field = Dir" in r.stdout and "--survey-field-radius = R" in r.stdout
    assert "[--survey-field DIR [--survey-field-radius R]]" in r.stdout
    out, fd, sh = str(tmp_path / "s.txt"), str(tmp_path / "field"), str(tmp_path / "shift.txt")
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-field", fd)
    assert r.returncode != 0 and "--survey-field is valid only together with --survey" in r.stderr and not os.path.exists(fd)
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field-radius", "2")
    assert r.returncode != 0 and "--survey-field-radius is valid only together with --survey-field" in r.stderr
    # the shift's radius keeps its own refusal: a field does not make it valid
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field", fd, "--survey-shift-radius", "2")
    assert r.returncode != 0 and "--survey-shift-radius is valid only together with --survey-shift" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-shift", sh, "--survey-field-radius", "2")
    assert r.returncode != 0 and "--survey-field-radius is valid only together with --survey-field" in r.stderr
    for radius in ("0", "9", "-1", "four", "4x"):
        r = cli(*src.cli["dir"], "--survey", out, "--survey-field", fd, "--survey-field-radius", radius)
        assert r.returncode != 0 and "--survey-field-radius expects a radius from 1 to 8" in r.stderr, radius
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field")
    assert r.returncode != 0 and "--survey-field needs the directory to write to" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field", fd, "--repack", str(tmp_path / "X"))
    assert r.returncode != 0 and "--survey cannot be combined with --repack" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(fd) and not os.path.exists(sh)
    # the run's own directory is no place for what was derived from it
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field", os.path.dirname(src.rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(out)
    assert not os.path.exists(os.path.join(src.rd, "field.txt"))


def test_a_run_without_a_whole_cell_is_refused(tmp_path):
    rd, _ = make_field_run(str(tmp_path / "data"), w=135, h=200)
    out, fd = str(tmp_path / "s.txt"), str(tmp_path / "field")
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-field", fd)
    assert r.returncode != 0 and "needs frames of at least 136x136, the run's are 135x200" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(fd)
    r = cli(*args, "--survey", out, "--survey-field", fd, "--survey-field-radius", "3")  # 135 = 128 + 2 * 3 + 1: one cell across
    assert r.returncode == 0 and os.path.exists(out), r.stderr
    assert open(os.path.join(fd, RUN_ID, "field.txt")).read().startswith("# abub3hs field 1\nradius 3 cell 128 grid 1 1 origin 3 36\n")
