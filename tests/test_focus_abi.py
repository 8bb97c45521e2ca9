"""abub3hs --survey-focus / Run.survey(focus=...) on the CPU side: abub_frame_focus_cells_dev is declared, exported, bound and
validates its arguments without a device; focusCellsHost and focusModelHost (the definition) against the numpy restatement
(tests/focusref.py); what a cell and a frame say (abub::focusCell, abub::focusFrame) against the restatement and against
known answers, every one exact; the CLI's host route on a small run that holds a blurred frame, a half-blurred one, a
saturated frame and a truncated file, in five source forms, which must all give the files focusref gives and leave the
survey's report, planes, shift file, field and light as they are; the flags and refusals; the sample frame, blurred once.
The sizes and contents (focus_sizes, focus_contents) and the run (make_focus_run) are shared with
tests/test_gpu_frame_focus.py and tests/test_gpu_focus_routes.py, which put them through the kernel and the device route."""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

import fieldref
import focusref
import shiftref
from autobub3hs_amd import _lib, hip, host
from test_shift_abi import smooth_texture
from test_survey_abi import ENV, NCAMS, RUN_ID, Sources, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E_INVALID = -1
C = focusref.CELL
N = C * C
W, H, F, NEV = 300, 170, 5, 5
TOTAL = F * NEV * NCAMS
GRID = (22, 21, 2, 1)  # x0, y0, ncx, ncy of 300 x 170 at R = 4
MARGIN = 8
SOFT = (1, 0, "cam0_image33.png")       # the whole frame blurred once
UNEVEN = (2, 0, "cam0_image34.png")     # only the right cell blurred, but for its first column: the left cell's ring
SATURATED = (2, 1, "cam1_image33.png")  # all 255
TRUNCATED = (NEV - 1, 1, "cam1_image30.png")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def focus_sizes():
    """(w, h, x0, y0, ncx, ncy) of the definition's and the kernel's tests, each on the field's grid: 130 x 130 at R = 1, where
    the ring is the frame's first and last row and column; 131 x 130; one cell at R = 4 with the origin at every residue
    mod 4; grids of 2 x 1, 1 x 2 (R = 1: the ring at the frame's edge) and 2 x 2 (R = 4), where neighbouring cells share ring
    pixels"""
    out = []
    for w, h, R in ((130, 130, 1), (131, 130, 1), (136, 136, 4), (138, 136, 4), (140, 137, 4), (142, 136, 4), (2 * C + 3, 131, 1),
                    (131, 2 * C + 3, 1), (2 * C + 9, 2 * C + 10, 4)):
        ncx, ncy, x0, y0 = fieldref.grid(w, h, R)
        out.append((w, h, x0, y0, ncx, ncy))
    return out


def stripes(w, h):
    """columns in the pattern 0 0 255 255: every horizontal central difference is 255 or -255, every vertical one 0"""
    return np.ascontiguousarray(np.broadcast_to(np.where(np.arange(w) % 4 >= 2, 255, 0).astype(np.uint8), (h, w)))


def focus_contents(w, h, rs):
    """the jobs of one size -> [(frame, model)]: random; a random frame against itself; a frame against its negative; the
    stripes against themselves; the stripes transposed; a random frame on a flat model; a frame of many 0 and 255 against a
    random model"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    a, b = rnd(), rnd()
    ends = rs.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (h, w))
    sx, sy = stripes(w, h), np.ascontiguousarray(stripes(h, w).T)
    return [(rnd(), rnd()), (a, a.copy()), ((255 - b).astype(np.uint8), b), (sx, sx.copy()), (sy, sy.copy()),
            (rnd(), np.full((h, w), 90, np.uint8)), (ends, rnd())]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_focus_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "int abub_frame_focus_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes," in hdr
    assert "uint32_t *status /*[njobs]*/, int32_t *rec /*[njobs * ncy * ncx * 5]*/, void *stream);" in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_focus_cells_dev") and "abub_frame_focus_cells_dev" in _lib.SIGNATURES
    assert callable(hip.frame_focus_cells) and callable(host.focus_cells_host) and callable(host.focus_model_host)
    assert callable(host.focus_cell) and callable(host.focus_frame)
    for name in ("abh_run_survey_focus", "abh_run_survey_focus_dev", "abh_focus_cells_host", "abh_focus_model_host", "abh_focus_cell",
                 "abh_focus_frame"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES


def test_frame_focus_cells_validates_before_it_touches_the_device():
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
        return L.abub_frame_focus_cells_dev(a["frames"], a["frames_bytes"], a["mu"], a["model_bytes"], a["jobs"], a["njobs"], a["W"],
                                            a["H"], a["x0"], a["y0"], a["ncx"], a["ncy"], a["status"], a["rec"], a["stream"])

    bad = [dict(frames=None), dict(mu=None), dict(jobs=None), dict(status=None), dict(rec=None), dict(njobs=-1),
           dict(W=129, ncx=1, x0=1), dict(H=129, y0=1), dict(W=0), dict(H=-3), dict(W=65536), dict(H=65536), dict(ncx=0), dict(ncy=0),
           dict(ncx=-1), dict(ncy=-2), dict(x0=0), dict(y0=0), dict(x0=-1), dict(y0=-1), dict(x0=44), dict(y0=42), dict(ncx=3),
           dict(ncy=2), dict(ncx=1 << 24), dict(ncy=1 << 24), dict(x0=(1 << 31) - 1), dict(y0=(1 << 31) - 1), dict(jobs=p + 4),
           dict(rec=p + 2), dict(status=p + 2), dict(rec=p + 1)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_focus_cells_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, x0=43, y0=41) == 0 and call(njobs=0, x0=1, y0=1) == 0 and call(njobs=0, W=130, H=130, x0=1, y0=1, ncx=1) == 0
    assert call(njobs=0, W=65535, H=65535, x0=126, y0=126, ncx=511, ncy=511) == 0
    assert call(njobs=0, rec=p + 4, status=p + 4) == 0  # (32-bit words: 4-byte aligned)
    assert not any(buf)
    for fn in (host.focus_cells_host, host.focus_model_host):  # the host entries refuse a grid without its ring too
        a = np.zeros((170, 300), np.uint8)
        for x0, y0, ncx, ncy in ((44, 21, 2, 1), (22, 42, 2, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 3, 1), (1, 1, 1, 2)):
            with pytest.raises(ValueError):
                fn(a, a, x0, y0, ncx, ncy)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_host_definition_against_numpy():
    sizes = focus_sizes()
    assert sizes[0] == (130, 130, 1, 1, 1, 1) and sizes[1][:2] == (131, 130)
    assert sorted({s[2] % 4 for s in sizes}) == [0, 1, 2, 3] and {(s[4], s[5]) for s in sizes} == {(1, 1), (2, 1), (1, 2), (2, 2)}
    for w, h, x0, y0, ncx, ncy in sizes:
        rs = np.random.RandomState(5000 + w)
        s6 = rs.randint(0, 256, (h, w)).astype(np.uint8)
        for k, (p, m) in enumerate(focus_contents(w, h, rs)):
            want = focusref.records(p, m, x0, y0, ncx, ncy)
            rec = host.focus_cells_host(p, m, x0, y0, ncx, ncy)
            assert rec.dtype == np.int32 and rec.shape == (ncy, ncx, 5) and np.array_equal(rec, want), (w, h, k)
            want_model = focusref.model_records(m, s6, x0, y0, ncx, ncy)
            model = host.focus_model_host(m, s6, x0, y0, ncx, ncy)
            assert model.dtype == np.int64 and model.shape == (ncy, ncx, 3) and np.array_equal(model, want_model), (w, h, k)
            G, M = rec[..., 2].astype(np.int64) + rec[..., 3], model[..., 0] + model[..., 1]
            # the identity that gives nv its meaning: G - M = sum over the cell and its ring of (p - m) c
            for cy in range(ncy):
                for cx in range(ncx):
                    xa, ya = x0 + C * cx, y0 + C * cy
                    d = p[ya - 1:ya + C + 1, xa - 1:xa + C + 1].astype(np.int64) - m[ya - 1:ya + C + 1, xa - 1:xa + C + 1]
                    assert int((d * focusref.coefficient(m, xa, ya)).sum()) == int(G[cy, cx] - M[cy, cx]), (w, h, k, cx, cy)
            if k == 1:  # p = m: the agreement is the model's own energy, and so is the frame's
                assert np.array_equal(G, M) and np.array_equal(rec[..., 0].astype(np.int64) + rec[..., 1], M)
            if k == 2:  # p = 255 - m
                assert np.array_equal(G, -M) and (G < 0).all()
            if k == 3:  # the largest value a record can hold
                assert (rec[..., :4] == [1065369600, 0, 1065369600, 0]).all() and (rec[..., 4] == N).all() and 255 * 255 * N == 1065369600
                assert (model[..., :2] == [1065369600, 0]).all()
            if k == 4:
                assert (rec[..., :4] == [0, 1065369600, 0, 1065369600]).all()
            if k == 5:  # a flat model has no edges
                assert not model.any() and not rec[..., 2:4].any()
                f = host.focus_frame(rec, model)
                assert (f["rated"], f["kind"]) == (0, "blind")


def frame_says(p, m, sigma6):
    """the records of p against (m, sigma6) on the 2 x 1 grid of a 300 x 170 frame through the host's functions, what the
    frame and every cell say through abub::focusFrame and abub::focusCell, and the same from the restatement, which must
    agree"""
    x0, y0, ncx, ncy = GRID
    rec, model = host.focus_cells_host(p, m, x0, y0, ncx, ncy), host.focus_model_host(m, sigma6, x0, y0, ncx, ncy)
    assert np.array_equal(rec, focusref.records(p, m, x0, y0, ncx, ncy))
    assert np.array_equal(model, focusref.model_records(m, sigma6, x0, y0, ncx, ncy))
    got, want = host.focus_frame(rec, model), focusref.summary(rec, model)
    assert got == {k: v for k, v in want.items() if k != "changed_cells"}, (got, want)
    for r, q in zip(rec.reshape(-1, 5), model.reshape(-1, 3)):
        assert host.focus_cell(r, q) == focusref.cell(r, q)
    return got, rec, model


def edged_texture(h, w, seed):
    """a smooth texture under a checkerboard of 6 x 6 squares: edges that one pass of a blur takes down"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (smooth_texture(h, w, seed) // 2 + 20 + 70 * ((xx // 6 + yy // 6) % 2)).astype(np.uint8)


def test_rdiv_floors_toward_minus_infinity():
    assert [focusref.rdiv(a, 2) for a in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]
    assert focusref.rdiv(-7, 3) == -2 and focusref.rdiv(7, 3) == 2 and focusref.rdiv(-15, 10) == -1 and focusref.rdiv(15, 10) == 2


def test_known_answers():
    rs = np.random.RandomState(6)
    six = np.full((H, W), 6, np.uint8)  # sigma = 1
    zero = np.zeros((H, W), np.uint8)
    right = np.zeros((H, W), bool)
    right[:, GRID[0] + C + 1:] = True  # the right cell (and what lies beyond it) but for its first column: the left cell's ring
    m = edged_texture(H, W, 3)
    assert m.min() > 0 and m.max() < 255
    none = dict(rated=2, clipped=0, changed=0, softer=0, harder=0)
    # p = m: G = M, nothing changed
    s, rec, model = frame_says(m, m, six)
    assert s == dict(none, kind="steady", keep_milli=1000, keep_min=1000, keep_max=1000, energy_milli=1000)
    # p = 255 - m: G = -M, every cell changed and softer
    s, _, _ = frame_says((255 - m).astype(np.uint8), m, six)
    assert s == dict(rated=2, clipped=0, changed=2, softer=2, harder=0, kind="soft", keep_milli=-1000, keep_min=-1000, keep_max=-1000,
                     energy_milli=1000)
    # one grey level of noise: steady under sigma = 1
    s, _, _ = frame_says((m.astype(np.int16) + rs.randint(-1, 2, (H, W))).astype(np.uint8), m, six)
    assert s["kind"] == "steady" and abs(s["keep_milli"] - 1000) < 10
    # blurred once: every cell softer, the energy falls below the agreement
    b = focusref.blur(m)
    s, _, _ = frame_says(b, m, six)
    assert (s["changed"], s["softer"], s["harder"], s["kind"]) == (2, 2, 0, "soft") and s["energy_milli"] < s["keep_milli"] < 900
    # half of the cells blurred
    s, _, _ = frame_says(np.where(right, b, m).astype(np.uint8), m, six)
    assert (s["changed"], s["softer"], s["harder"], s["kind"]) == (1, 1, 0, "uneven") and s["keep_max"] == 1000
    # twice the contrast about the mean: harder
    hard = np.clip(2 * m.astype(np.int16) - 100, 1, 254).astype(np.uint8)
    s, _, _ = frame_says(hard, m, six)
    assert (s["changed"], s["softer"], s["harder"], s["kind"]) == (2, 0, 2, "uneven") and s["keep_milli"] > 1500
    # a flat model: M = 0, no cell is rated, none clipped
    s, _, _ = frame_says(m, np.full((H, W), 100, np.uint8), six)
    assert s == dict(rated=0, clipped=0, changed=0, softer=0, harder=0, kind="blind", keep_milli=None, keep_min=None, keep_max=None,
                     energy_milli=None)
    # a saturated frame: every cell clipped
    s, _, _ = frame_says(np.full((H, W), 255, np.uint8), m, six)
    assert (s["rated"], s["clipped"], s["kind"]) == (0, 2, "blind")
    # N / 16 pixels at 0 or 255 do not clip a cell, one more does
    p = m.copy()
    p[GRID[1], GRID[0]:GRID[0] + C] = 0
    p[GRID[1] + 1:GRID[1] + 8, GRID[0]:GRID[0] + C] = 255
    assert N // 16 == 8 * C
    s, rec, _ = frame_says(p, m, six)
    assert (s["rated"], s["clipped"]) == (2, 0) and list(rec[0, :, 4]) == [8 * C, 0]
    p[GRID[1] + 8, GRID[0]] = 0
    s, rec, _ = frame_says(p, m, six)
    assert (s["rated"], s["clipped"]) == (1, 1) and rec[0, 0, 4] == 8 * C + 1
    # sigma = 0: nv = 0, any change of the agreement counts
    s, rec, model = frame_says(m, m, zero)
    assert not model[..., 2].any() and s["kind"] == "steady" and s["rated"] == 2
    p = m.copy()
    y, x = GRID[1] + 40, GRID[0] + 40
    assert focusref.coefficient(m, GRID[0], GRID[1])[41, 41] != 0
    p[y, x] += 1
    s, _, _ = frame_says(p, m, zero)
    assert (s["changed"], s["kind"]) == (1, "uneven")
    assert frame_says(p, m, six)[0]["kind"] == "steady"  # (and under sigma = 1 it does not)


def test_the_comparisons_are_strict():
    """(M - G)^2 = nv is not a change, nv + 1 is; M^2 = nv is not rated, nv + 1 is; records at the ends of their range"""
    cell = lambda G, mxx, myy, nv, clip=0, e=0: host.focus_cell([e, 0, G, 0, clip], [mxx, myy, nv])  # noqa: E731
    for G, M, nv in ((990, 1000, 100), (1010, 1000, 100), (2000000000, 2130739200, 130739200 ** 2)):
        rec = [0, 0, G - G // 2, G // 2, 0]
        for d, changed in ((0, False), (-1, True)):
            got = host.focus_cell(rec, [M, 0, nv + d])
            assert got == focusref.cell(rec, [M, 0, nv + d]) and got["rated"] and got["changed"] is changed, (G, M, nv, d)
            assert got["softer"] is (changed and G < M)
    assert cell(0, 10, 0, 100)["rated"] is False and cell(0, 10, 0, 99)["rated"] is True and cell(0, 6, 4, 100)["rated"] is False
    assert cell(0, 0, 0, 0) == dict(rated=False, clipped=False, changed=False, softer=False, keep=None, energy=None)
    assert cell(5, 10, 0, 0, clip=N // 16)["rated"] is True and cell(5, 10, 0, 0, clip=N // 16 + 1) == dict(
        rated=False, clipped=True, changed=False, softer=False, keep=None, energy=None)
    # keep and energy round to the nearest, a half upward, toward minus infinity below zero
    assert cell(1, 2000, 0, 0)["keep"] == 1 and cell(-1, 2000, 0, 0)["keep"] == 0 and cell(-3, 2000, 0, 0)["keep"] == -1
    assert cell(0, 3, 0, 0, e=1)["energy"] == 333 and cell(0, 3, 0, 0, e=2)["energy"] == 667
    # the largest sums: M and nv at their bounds do not overflow the 128-bit arithmetic
    big = [1065369600, 1065369600, 16900 * (255 * 1020) ** 2]
    rec = [1065369600, 1065369600, -1065369600, -1065369600, 0]
    assert host.focus_cell(rec, big) == focusref.cell(rec, big) and host.focus_cell(rec, big)["keep"] == -1000


# ---- runs --------------------------------------------------------------------------------------------------------------------
def make_focus_run(root, untrained_cam=None, w=W, h=H):
    """5 events x 2 cameras x 5 frames of 300 x 170 (at R = 4 a grid of 2 x 1 cells, origin 22, 21): per camera an edged
    texture, one grey level of noise per frame: a steady stack.  One frame is blurred once everywhere, one only in its
    right cell, one is all 255; one file is truncated.  untrained_cam: that camera's second frame differs from its first in
    every event, so the entropy veto leaves it no training frames.  Another size: the plain frames only
    -> (run dir, {(event, cam, name): image or None (does not decode)})"""
    rs = np.random.RandomState(41)
    rd = os.path.join(root, RUN_ID)
    tex = [shiftref.displaced(edged_texture(h + 2 * MARGIN, w + 2 * MARGIN, 90 + c), 0, 0, w, h, MARGIN) for c in range(NCAMS)]
    special = (w, h) == (W, H)
    frames = {}
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for c in range(NCAMS):
            for k in range(F):
                key = (e, c, f"cam{c}_image{30 + k}.png")
                img = tex[c].astype(np.int16) + rs.randint(-1, 2, (h, w))
                if special and key == SOFT:
                    img = focusref.blur(np.clip(img, 0, 255)).astype(np.int16)
                if special and key == UNEVEN:
                    img[:, GRID[0] + C + 1:] = focusref.blur(np.clip(img, 0, 255))[:, GRID[0] + C + 1:]
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


def expected_focus(rd, frames, R=4, w=W, h=H):
    """-> (focus.txt, {cam: the array of cam<c>_focus.npy}, {cam: that of cam<c>_focus_model.npy}, the models)"""
    models = trained_models(rd, w, h)
    rows = focusref.rows_of(stacks_of(frames), w, h, models, R)
    return focusref.report(models, rows, w, h, R), focusref.arrays(models, rows, w, h, R), focusref.model_arrays(models, w, h, R), models


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("focus_soft"))
    rd, frames = make_focus_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def half_trained(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("focus_half"))
    return make_focus_run(os.path.join(root, "data"), untrained_cam=0)


def read_focus(d):
    """the directory DIR/<run_ID> -> (focus.txt or None, {cam: records}, {cam: model records})"""
    if not os.path.isdir(d):
        return None, {}, {}
    arrays = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_focus.npy")}
    marr = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_focus_model.npy")}
    assert sorted(arrays) == sorted(marr)
    assert sorted(os.listdir(d)) == sorted(["focus.txt"] + [f"cam{c}_focus{s}.npy" for c in arrays for s in ("", "_model")])
    return open(os.path.join(d, "focus.txt")).read(), arrays, marr


def same_arrays(got, want, dtype=np.int32):
    return sorted(got) == sorted(want) and all(got[c].dtype == dtype and got[c].shape == want[c].shape and np.array_equal(got[c], want[c])
                                              for c in want)


def same_focus(got, want):
    """(text, arrays, model arrays) against expected_focus' first three"""
    return got[0] == want[0] and same_arrays(got[1], want[1]) and same_arrays(got[2], want[2], np.int64)


def focus_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-focus stem_focus -> (the process, the report, (focus.txt, the arrays, the models'))"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-focus", stem + "_focus", *more, env=env)
    return r, text, read_focus(os.path.join(stem + "_focus", RUN_ID))


def check_kinds(text, R=4):
    """focus.txt of the run with models that are the scene at sigma 1: every row says what was done to its frame"""
    lines = text.splitlines()
    assert lines[:2] == ["# abub3hs focus 1", f"radius {R} cell 128 grid 2 1 origin 22 21"] and lines[2] + "\n" == focusref.HEADER
    assert len(lines) == 3 + TOTAL + NCAMS + NCAMS * 1 + 1
    per_cam = [0] * NCAMS
    for l in lines[3:3 + TOTAL]:
        r = l.split("\t")
        assert len(r) == 16
        key = (int(r[0]), int(r[1]), r[3])
        if key == TRUNCATED:
            assert r[4:] == ["undecodable"] + ["-"] * 11
            continue
        assert r[4] == "ok" and int(r[5]) == per_cam[key[1]]
        per_cam[key[1]] += 1
        if key == SATURATED:
            assert r[6:] == ["0", "2", "0", "0", "0"] + ["-"] * 4 + ["blind"], r
        elif key == SOFT:
            assert r[6:11] == ["2", "0", "2", "2", "0"] and r[15] == "soft" and int(r[14]) < int(r[11]) < 900, r
        elif key == UNEVEN:
            assert r[6:11] == ["2", "0", "1", "1", "0"] and r[15] == "uneven" and int(r[12]) < 900 < int(r[13]), r
        else:
            assert r[6:11] == ["2", "0", "0", "0", "0"] and r[15] == "steady" and abs(int(r[11]) - 1000) < 10, r
    assert lines[3 + TOTAL] == f"focus cam 0 frames {F * NEV} blind 0 steady {F * NEV - 2} soft 1 uneven 1 first_changed_event 1"
    assert lines[4 + TOTAL] == f"focus cam 1 frames {F * NEV - 1} blind 1 steady {F * NEV - 2} soft 0 uneven 0 first_changed_event -"
    assert lines[5 + TOTAL:] == ["changed cam 0 y 0 1 2", "changed cam 1 y 0 0 0",
                                 f"run frames {TOTAL - 1} blind 1 steady {TOTAL - 4} soft 1 uneven 1"]


def test_the_restatement_sees_the_blur(soft):
    """the run is what its description says, with the textures themselves as the models and sigma 1"""
    _, frames = soft
    models = [dict(mu=shiftref.displaced(edged_texture(H + 2 * MARGIN, W + 2 * MARGIN, 90 + c), 0, 0, W, H, MARGIN),
                   sigma=np.ones((H, W), np.uint8)) for c in range(NCAMS)]
    rows = focusref.rows_of(stacks_of(frames), W, H, models, 4)
    check_kinds(focusref.report(models, rows, W, H, 4))
    arrays = focusref.arrays(models, rows, W, H, 4)
    assert arrays[0].shape == (F * NEV, 1, 2, 5) and arrays[1].shape == (F * NEV - 1, 1, 2, 5)
    text = focusref.report([None, models[1]], focusref.rows_of(stacks_of(frames), W, H, [None, models[1]], 4), W, H, 4)
    assert text.count("focus cam 0 none\n") == 1 and "changed cam 0" not in text and "changed cam 1 y 0" in text


def others(tmp_path, name, tag):
    """the other four outputs of a survey, into files of their own"""
    return ["--survey-planes", str(tmp_path / f"{name}_planes_{tag}"), "--survey-shift", str(tmp_path / f"{name}_shift_{tag}.txt"),
            "--survey-field", str(tmp_path / f"{name}_field_{tag}"), "--survey-light", str(tmp_path / f"{name}_light_{tag}")]


def same_others(tmp_path, name):
    """the shift file, the planes, the field and the light of the run with the flag against those without"""
    if open(str(tmp_path / f"{name}_shift_with.txt")).read() != open(str(tmp_path / f"{name}_shift_plain.txt")).read():
        return False
    for kind in ("planes", "field", "light"):
        with_flag, without = (os.path.join(str(tmp_path / f"{name}_{kind}_{tag}"), RUN_ID) for tag in ("with", "plain"))
        if sorted(os.listdir(with_flag)) != sorted(os.listdir(without)) or not os.listdir(without):
            return False
        for f in os.listdir(without):
            if open(os.path.join(with_flag, f), "rb").read() != open(os.path.join(without, f), "rb").read():
                return False
    return True


def test_cli_host_route_on_every_source_form(soft, tmp_path):
    src, frames = soft
    want = expected_focus(src.rd, frames)
    models = want[3]
    files = []
    for name in src.cli:
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / (name + "_plain.txt")), *others(tmp_path, name, "plain"))
        r, report, got = focus_cli(src.cli[name], str(tmp_path / name), *others(tmp_path, name, "with"))
        assert r.returncode == plain.returncode == 1, (name, r.stdout, r.stderr)  # (the truncated file: the survey's status)
        assert report == report_plain and report is not None, name  # the report and the other four outputs do not change
        assert same_others(tmp_path, name), name
        assert same_focus(got, want), name
        assert "survey-focus: " in r.stdout and "survey-focus" not in plain.stdout
        files.append(got[0])
    assert len(files) == 5 and len(set(files)) == 1
    for c, m in enumerate(models):
        assert (f"focus cam {c} none" in want[0].splitlines()) == (m is None) and (c in want[1]) == (m is not None)
    # the field's radius is the focus', with and without the field: another grid line, here the same cells
    want8 = expected_focus(src.rd, frames, 8)
    r, report, got = focus_cli(src.cli["dir"], str(tmp_path / "r8"), "--survey-field-radius", "8")
    assert r.returncode == 1 and same_focus(got, want8) and report == report_plain
    assert want8[0].splitlines()[1] == "radius 8 cell 128 grid 2 1 origin 22 21"
    want1 = expected_focus(src.rd, frames, 1)
    r, report, got = focus_cli(src.cli["packed"], str(tmp_path / "r1"), "--survey-field-radius=1", "--survey-field", str(tmp_path / "r1_field"))
    assert r.returncode == 1 and same_focus(got, want1)
    assert want1[0].splitlines()[1] == "radius 1 cell 128 grid 2 1 origin 22 21"
    assert open(str(tmp_path / "r1_field" / RUN_ID / "field.txt")).read().splitlines()[1] == want1[0].splitlines()[1]


def test_a_camera_that_does_not_train_has_no_focus(half_trained, tmp_path):
    rd, frames = half_trained
    want = expected_focus(rd, frames)
    assert want[3][0] is None
    r, report, got = focus_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "half"))
    assert r.returncode == 1 and same_focus(got, want), (r.stdout, r.stderr)
    assert "focus cam 0 none\n" in got[0] and "survey: a camera did not train" in r.stdout and 0 not in got[1] and 0 not in got[2]
    assert all(l.endswith("\t-" * 11) for l in got[0].splitlines()[3:3 + TOTAL] if l.split("\t")[1] == "0")


def test_run_survey_agrees_with_the_cli(soft, tmp_path):
    src, frames = soft
    want = expected_focus(src.rd, frames)
    models = want[3]
    for name in ("dir", "deflated"):
        run = src.open(name)
        try:
            plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
            res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, focus=str(tmp_path / "o"))
            res2, _ = run.survey(nthreads=4, ncams=NCAMS, focus=str(tmp_path / "o2"), light=str(tmp_path / "l2"), field=str(tmp_path / "f2"),
                                 field_radius=2, shift=str(tmp_path / "s2.txt"))
        finally:
            run.close()
        assert text == text_plain and same_focus(read_focus(str(tmp_path / "o")), want)
        assert same_focus(read_focus(str(tmp_path / "o2")), expected_focus(src.rd, frames, 2))
        with_model = sum(1 for (e, c, n), img in frames.items() if img is not None and models[c] is not None)
        assert res["focus_frames_kernel"] == 0 and res["focus_launches"] == 0 and res["focus_frames_host"] == with_model
        assert res2["focus_frames_host"] == with_model == res2["shift_frames_host"] == res2["field_frames_host"] == res2["light_frames_host"]
        assert "focus_frames_host" not in plain and "light_frames_host" not in res and "field_frames_host" not in res
        assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
               {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}
    run = src.open("dir")
    try:
        with pytest.raises(RuntimeError, match="radius"):
            run.survey(nthreads=4, ncams=NCAMS, focus=str(tmp_path / "bad"), field_radius=9)
    finally:
        run.close()
    assert not os.path.exists(str(tmp_path / "bad"))


def test_cli_flags_and_refusals(soft, tmp_path):
    src, _ = soft
    r = cli("-h")
    assert "--survey-focus = Dir" in r.stdout and "[--survey-focus DIR [--survey-field-radius R]]" in r.stdout
    out, od, sh = str(tmp_path / "s.txt"), str(tmp_path / "focus"), str(tmp_path / "shift.txt")
    r = cli(*src.cli["dir"], "-o", str(tmp_path), "--survey-focus", od)
    assert r.returncode != 0 and "--survey-focus is valid only together with --survey" in r.stderr and not os.path.exists(od)
    # the shift's radius keeps its own refusal: the focus does not make it valid
    r = cli(*src.cli["dir"], "--survey", out, "--survey-focus", od, "--survey-shift-radius", "2")
    assert r.returncode != 0 and "--survey-shift-radius is valid only together with --survey-shift" in r.stderr
    for radius in ("0", "9", "-1", "four", "4x"):
        r = cli(*src.cli["dir"], "--survey", out, "--survey-focus", od, "--survey-field-radius", radius)
        assert r.returncode != 0 and "--survey-field-radius expects a radius from 1 to 8" in r.stderr, radius
    r = cli(*src.cli["dir"], "--survey", out, "--survey-field-radius", "2")  # (and without any of the three it stays refused)
    assert r.returncode != 0 and "--survey-field-radius is valid only together with --survey-field" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-focus")
    assert r.returncode != 0 and "--survey-focus needs the directory to write to" in r.stderr
    r = cli(*src.cli["dir"], "--survey", out, "--survey-focus", od, "--repack", str(tmp_path / "X"))
    assert r.returncode != 0 and "--survey cannot be combined with --repack" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(od) and not os.path.exists(sh)
    # the run's own directory is no place for what was derived from it
    r = cli(*src.cli["dir"], "--survey", out, "--survey-focus", os.path.dirname(src.rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(out)
    assert not os.path.exists(os.path.join(src.rd, "focus.txt"))


def test_a_run_without_a_whole_cell_is_refused(tmp_path):
    rd, _ = make_focus_run(str(tmp_path / "data"), w=42, h=140)
    out, od = str(tmp_path / "s.txt"), str(tmp_path / "focus")
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-focus", od)
    assert r.returncode != 0 and "need frames of at least 136x136, the run's are 42x140" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(od)
    rd, _ = make_focus_run(str(tmp_path / "data2"), w=135, h=200)
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-focus", od)
    assert r.returncode != 0 and "need frames of at least 136x136, the run's are 135x200" in r.stderr, r.stderr
    r = cli(*args, "--survey", out, "--survey-focus", od, "--survey-field-radius", "3")  # 135 = 128 + 2 * 3 + 1: one cell across
    assert r.returncode == 0 and os.path.exists(out), r.stderr
    assert open(os.path.join(od, RUN_ID, "focus.txt")).read().startswith("# abub3hs focus 1\nradius 3 cell 128 grid 1 1 origin 3 36\n")


# ---- the sample frame ----------------------------------------------------------------------------------------------------------
SAMPLE = dict(rated=95, clipped=9, changed=95, softer=95, harder=0, kind="soft", keep_milli=597, keep_min=429, keep_max=834,
              energy_milli=454)  # (the line DESIGN quotes)


def test_the_sample_frame_blurred_once_is_soft(tmp_path):
    """the sample frame through one pass of the 3 x 3 binomial, against itself as the model at sigma 1: every rated cell is
    softer, and the frame's line is the one DESIGN quotes.  Then as a two-event run whose last frame is the blurred one: its
    files are the restatement's, and where the camera trains (on a GPU) that frame's row says `soft` and the others `steady`"""
    sample = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    h, w = sample.shape
    soft_frame = focusref.blur(sample)
    ncx, ncy, x0, y0 = fieldref.grid(w, h, 4)
    assert (w, h, ncx, ncy) == (1680, 1050, 13, 8)
    six = np.full((h, w), 6, np.uint8)
    rec, model = host.focus_cells_host(soft_frame, sample, x0, y0, ncx, ncy), host.focus_model_host(sample, six, x0, y0, ncx, ncy)
    assert np.array_equal(rec, focusref.records(soft_frame, sample, x0, y0, ncx, ncy))
    assert np.array_equal(model, focusref.model_records(sample, six, x0, y0, ncx, ncy))
    got, want = host.focus_frame(rec, model), focusref.summary(rec, model)
    assert got == {k: v for k, v in want.items() if k != "changed_cells"}
    assert got["kind"] == "soft" and got["changed"] == got["softer"] == got["rated"] > 0 and got["energy_milli"] < got["keep_milli"] < 1000
    assert got == SAMPLE, got
    rd = os.path.join(str(tmp_path), "data", RUN_ID)
    frames = {}
    for e in range(2):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for k in range(3):
            frames[(e, 0, f"cam0_image{30 + k}.png")] = soft_frame if (e, k) == (1, 2) else sample
    for (e, c, name), img in frames.items():
        open(os.path.join(rd, str(e), "Images", name), "wb").write(png_bytes(img))
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(2):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    r, report, got = focus_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "sample"), env=dict(ENV, ABUB_NUM_CAMS="1"))
    run = host.Run("raw", rd + "/", "Images")
    try:
        st, tss, mu, sg = run.train(0, shape=(h, w))
    except RuntimeError:  # (no device: the Trainer does not run, the camera has no model)
        st = -7
    finally:
        run.close()
    models = [None if st else dict(trained=tss, mu=mu, sigma=sg)]
    rows = focusref.rows_of(stacks_of(frames), w, h, models, 4)
    assert got[0] == focusref.report(models, rows, w, h, 4), (r.stdout, r.stderr)
    assert same_arrays(got[1], focusref.arrays(models, rows, w, h, 4))
    assert same_arrays(got[2], focusref.model_arrays(models, w, h, 4), np.int64)
    lines = got[0].splitlines()
    assert lines[1] == "radius 4 cell 128 grid 13 8 origin 8 13" and len(lines) == 3 + 6 + 1 + (0 if st else 8) + 1
    if st == 0:
        row = lines[3 + 5].split("\t")
        assert row[:5] == ["1", "0", "2", "cam0_image32.png", "ok"] and row[15] == "soft", row
        assert row[8] == row[9] == row[6] != "0" and row[10] == "0" and int(row[14]) < int(row[11]) < 1000, row
        assert all(l.split("\t")[15] == "steady" for l in lines[3:3 + 5])
        assert lines[-1] == "run frames 6 blind 0 steady 5 soft 1 uneven 0"
