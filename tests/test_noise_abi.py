"""abub3hs --survey-noise / Run.survey(noise=...) on the CPU side: abub_frame_noise_cells_dev is declared, exported, bound and
validates its arguments without a device; noiseCellsHost and noiseModelHost (the definition) against the numpy restatement
(tests/noiseref.py) at the sizes and contents of the issue; what a cell and a frame say (abub::noiseCell, abub::noiseFrame)
on hand-made records, one per state and kind; the CLI's host route on a small run with planted cases, whose files must be the
restatement's byte for byte and which must leave every other product of the survey as it is; the flags and refusals.  The
sizes and contents (noise_sizes, noise_contents) and the run (make_noise_run) are shared with tests/test_gpu_frame_noise.py
and tests/test_gpu_noise_routes.py, which put them through the kernel and the device route."""
import ctypes
import os

import numpy as np
import pytest

import noiseref
from autobub3hs_amd import _lib, hip, host
from test_light_abi import light_sizes
from test_survey_abi import ENV, NCAMS, RUN_ID, cli, png_bytes, stacks_of, survey_cli, trained_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
C = noiseref.CELL
N = C * C
R = 4
W, H, F, NEV = 2 * C + 2 * R + 3, C + 2 * R + 1, 8, 8
GRID = (5, 4, 2, 1)  # x0, y0, ncx, ncy of 267 x 137 at R = 4
SIGMA = 3
NOISY_EVENT, NOISY_FROM = 2, 4          # its frames from 4 on have noise of 2 SIGMA
DISC_EVENT, DISC_FROM = 3, 5            # a bright disc in the left cell from frame 5 on
DISC = (GRID[0] + 64, GRID[1] + 64, 30)  # x, y, radius: 2821 pixels, 17 % of its cell
TRUNCATED = (4, 1, "cam1_image33.png")
REMOVED = (5, 1, "cam1_image34.png")
WIDER = (6, 1, "cam1_image31.png")      # stack position 1: out of the baseline, and frame 3 of its stack has no reference
UNTRAINED = 0
TOTAL = F * NEV * NCAMS


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def noise_sizes():
    """(w, h, x0, y0, ncx, ncy): the light's sizes (128 x 128 at the origin; the field's sizes at R = 4, with grids of 2 x 1,
    2 x 2 and 3 x 1) and x0 at every residue mod 4 on the odd width 128 + 19"""
    return light_sizes() + [(C + 19, C + 2, x0, 1, 1, 1) for x0 in (16, 17, 18, 19)]


def noise_contents(w, h, rs):
    """the jobs of one size -> [(frame, reference frame, sigma6)]: random; 255 against 0 and the reverse under s = 255 (the
    largest record, both signs of s1_in); random under s = 0 everywhere and under s = 255 everywhere; |d| = s exactly in the
    even columns and s + 1 in the odd ones, d of both signs, and the reverse, so that with the origins every byte of a dword
    has both; the reference the same array as the frame"""
    rnd = lambda: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    full, none = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    a = rnd()
    out = [(rnd(), rnd(), rnd()), (full, none, full), (none, full, full), (rnd(), rnd(), none), (rnd(), rnd(), full)]
    for odd in (0, 1):
        p = rs.randint(60, 190, (h, w))
        s = rs.randint(0, 41, (h, w))
        over = (np.arange(w)[None, :] + np.zeros((h, 1), np.int64)) % 2 == odd
        r = p + np.where(rs.randint(0, 2, (h, w)) == 1, 1, -1) * (s + over)
        out.append((p.astype(np.uint8), r.astype(np.uint8), s.astype(np.uint8)))
    out.append((a, a, rnd()))
    return out


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_noise_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    assert "#define ABUB_NOISE_WORDS 6" in hdr
    assert "int abub_frame_noise_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *sigma6, size_t model_bytes," in hdr
    assert "const abub_stat_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy," in hdr
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "abub_frame_noise_cells_dev") and "abub_frame_noise_cells_dev" in _lib.SIGNATURES
    assert callable(hip.frame_noise_cells) and callable(host.noise_cells_host) and callable(host.noise_model_host) and callable(host.noise_cell)
    for name in ("abh_run_survey_noise", "abh_run_survey_noise_dev", "abh_noise_cells_host", "abh_noise_model_host", "abh_noise_cell",
                 "abh_noise_frame"):
        assert hasattr(host.lib(), name) and name in host.SIGNATURES
    assert hip.NOISE_WORDS == 6


def test_frame_noise_cells_validates_before_it_touches_the_device():
    """every refusal comes before the first HIP call, so it is the same with and without a device; the buffers are host
    memory that a launch could not even read"""
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    ok = dict(frames=p, frames_bytes=4096, sigma6=p, model_bytes=4096, jobs=p, njobs=1, W=300, H=170, x0=22, y0=21, ncx=2, ncy=1, status=p,
              rec=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_noise_cells_dev(a["frames"], a["frames_bytes"], a["sigma6"], a["model_bytes"], a["jobs"], a["njobs"], a["W"],
                                            a["H"], a["x0"], a["y0"], a["ncx"], a["ncy"], a["status"], a["rec"], a["stream"])

    bad = [dict(frames=None), dict(sigma6=None), dict(jobs=None), dict(status=None), dict(rec=None), dict(njobs=-1), dict(W=127, ncx=1, x0=0),
           dict(H=127, y0=0), dict(W=0), dict(H=-3), dict(W=65536), dict(H=65536), dict(ncx=0), dict(ncy=0), dict(ncx=-1), dict(ncy=-2),
           dict(x0=-1), dict(y0=-1), dict(x0=45), dict(y0=43), dict(ncx=3), dict(ncy=2), dict(ncx=1 << 24), dict(ncy=1 << 24),
           dict(x0=(1 << 31) - 1), dict(y0=(1 << 31) - 1), dict(jobs=p + 4), dict(rec=p + 2), dict(status=p + 2), dict(rec=p + 1)]
    for kw in bad:
        assert L.abub_k2_set_option(None, 0) == -1  # (another text first: a refusal must write its own)
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_noise_cells_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0  # nothing to do, nothing touched
    assert call(njobs=0, x0=44, y0=42) == 0 and call(njobs=0, x0=0, y0=0) == 0 and call(njobs=0, W=128, H=128, x0=0, y0=0, ncx=1) == 0
    assert call(njobs=0, W=65535, H=65535, x0=127, y0=127, ncx=511, ncy=511) == 0
    assert call(njobs=0, rec=p + 4, status=p + 4) == 0  # (i32 words: 4-byte aligned)
    assert not any(buf)
    a = np.zeros((170, 300), np.uint8)  # the host entries refuse a grid outside the frame too
    for x0, y0, ncx, ncy in ((45, 21, 2, 1), (22, 43, 2, 1), (-1, 0, 1, 1), (0, 0, 0, 1), (0, 0, 3, 1), (0, 0, 1, 2)):
        with pytest.raises(ValueError):
            host.noise_cells_host(a, a, a, x0, y0, ncx, ncy)
        with pytest.raises(ValueError):
            host.noise_model_host(a, np.zeros((0, max(ncy, 0), max(ncx, 0), 6), np.int32), x0, y0, ncx, ncy)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_host_definition_against_numpy():
    sizes = noise_sizes()
    assert sorted({s[2] % 4 for s in sizes if s[0] == C + 19}) == [0, 1, 2, 3] and (C + 19) % 2
    assert {(s[4], s[5]) for s in sizes} == {(1, 1), (2, 1), (2, 2), (3, 1)} and sizes[0] == (C, C, 0, 0, 1, 1)
    for w, h, x0, y0, ncx, ncy in sizes:
        rs = np.random.RandomState(5000 + w + x0)
        recs = []
        for k, (p, r, s) in enumerate(noise_contents(w, h, rs)):
            rec = host.noise_cells_host(p, r, s, x0, y0, ncx, ncy)
            assert rec.dtype == np.int32 and rec.shape == (ncy, ncx, 6), (w, h, k)
            assert np.array_equal(rec, noiseref.records(p, r, s, x0, y0, ncx, ncy)), (w, h, x0, k)
            recs.append(rec)
            if k == 1:  # the largest record, s1_in at its largest
                assert (rec == [0, N, 255 * N, 1065369600, 255 * N, 1065369600]).all() and 255 * 255 * N == 1065369600 < 2 ** 31
            if k == 2:
                assert (rec == [0, N, -255 * N, 1065369600, 255 * N, 1065369600]).all()
            if k == 3:  # s = 0: only d = 0 is inside, and adds nothing
                assert not rec[..., 2:4].any() and (rec[..., 0] > N - 200).all()
            if k == 4:  # s = 255: nothing is over
                assert not rec[..., 0].any() and np.array_equal(rec[..., 3], rec[..., 5])
            if k in (5, 6):  # half of every cell is over by one grey level, whichever column the cell begins in
                assert (rec[..., 0] == N // 2).all() and not rec[..., 1].any()
            if k == 7:  # the reference is the frame itself
                assert not rec[..., [0, 2, 3, 4, 5]].any()
        s6 = noise_contents(w, h, rs)[0][2]
        model = host.noise_model_host(s6, np.stack(recs), x0, y0, ncx, ncy)
        assert model.dtype == np.int64 and np.array_equal(model, noiseref.model_records(s6, recs, x0, y0, ncx, ncy)), (w, h)
        assert (model[..., 2] >= 2).all() and (model[..., 2] < len(recs)).all()  # some of the records are busy or clipped, some not
        none = host.noise_model_host(s6, np.zeros((0, ncy, ncx, 6), np.int32), x0, y0, ncx, ncy)
        assert not none[..., :3].any() and np.array_equal(none, noiseref.model_records(s6, [], x0, y0, ncx, ncy))


BASE = [100 * N, N, 1, 1800 * N, 0]  # a baseline of 100 = 2 sigma^2 per pixel from one row; (6 sigma)^2 = 1800 agrees with it


def rec_of(q_milli=1000, n_over=0, n_clip=0, s1=0):
    """a record whose E is q_milli thousandths of BASE's share of its inside pixels (s1 adds its square over n_in to s2_in)"""
    n = N - n_over
    s2 = -(-100 * n * q_milli // 1000) + (s1 * s1 + n - 1) // n  # (rounded up: q_milli floors)
    return [n_over, n_clip, s1, s2, 0, s2 + 400 * n_over]


def says(rec, model):
    got, want = host.noise_cell(rec, model), noiseref.cell(rec, model)
    assert {k: got[k] for k in want} == want and got["model_milli"] == noiseref.model_milli(model), (got, want)
    return got


def test_what_a_cell_says_on_hand_made_records():
    assert says(rec_of(), BASE) == dict(state="same", q_milli=1000, all_milli=1000, model_milli=1000)
    assert says(rec_of(1500), BASE)["state"] == "same" and says(rec_of(1501), BASE)["state"] == "noisy"  # the comparisons are strict
    assert says(rec_of(667), BASE)["state"] == "same" and says(rec_of(666), BASE)["state"] == "quiet"
    # the inside mean is taken out: a level step between the two frames is no noise
    assert says(rec_of(1000, s1=5 * N), BASE)["q_milli"] in (999, 1000) and rec_of(1000, s1=5 * N)[3] == 125 * N
    # the states in their order: clipped before busy before nobase
    assert N // 8 == 2048 and N // 4 == 4096
    assert says(rec_of(n_clip=2048), BASE)["state"] == "same" and says(rec_of(n_clip=2049), BASE)["state"] == "clipped"
    assert says(rec_of(n_over=4096), BASE)["state"] == "same" and says(rec_of(n_over=4097), BASE)["state"] == "busy"
    assert says(rec_of(n_over=4097, n_clip=2049), BASE)["state"] == "clipped"
    for nobase in ([0, N, 1, 5, 0], [100 * N, N, 0, 5, 0], [0, 0, 0, 0, N]):
        assert says(rec_of(), nobase) == dict(state="nobase", q_milli=None, all_milli=0, model_milli=noiseref.model_milli(nobase))
        assert says(rec_of(n_over=4097), nobase)["state"] == "busy" and says(rec_of(n_clip=2049), nobase)["state"] == "clipped"
    # a busy cell is not rated, but all_milli says what fills it: here the over pixels carry 400 each
    busy = says(rec_of(n_over=8192), BASE)
    assert busy["state"] == "busy" and busy["q_milli"] is None and busy["all_milli"] == 1000 * (50 * N + 200 * N) // (100 * N)
    # a product beyond 64 bits: the largest E against the baseline of a million rows
    big = [1065369600 * 10 ** 6, N * 10 ** 6, 10 ** 6, 255 * 255 * N, 0]
    assert 1000 * 1065369600 * big[1] > 2 ** 64
    assert says([0, 0, 0, 1065369600, 255 * N, 1065369600], big) == dict(state="same", q_milli=1000, all_milli=1000, model_milli=18000)
    assert says([0, 0, 0, 1065369600, 255 * N, 1065369600], [big[0] // 2] + big[1:])["q_milli"] == 2000
    # sigma6 all zero: no model_milli
    assert says(rec_of(), BASE[:3] + [0, N])["model_milli"] == 0


def frame_says(recs, models=None):
    recs = np.array(recs, np.int32)
    models = np.array(models if models is not None else [BASE] * len(recs), np.int64)
    got, want = host.noise_frame(recs, models), noiseref.summary(recs, models)
    assert got == {k: v for k, v in want.items() if k != "changed_cells"}, (got, want)
    return got


def test_what_a_frame_says_one_per_kind():
    same, noisy, quiet, clipped, busy = rec_of(), rec_of(2000), rec_of(500), rec_of(n_clip=N), rec_of(n_over=N // 2)
    s = frame_says([same] * 4)
    assert s == dict(rated=4, clipped=0, busy=0, noisy=0, quiet=0, kind="steady", q_milli=1000, q_min=1000, q_max=1000, all_milli=1000)
    assert frame_says([clipped] * 4) == dict(rated=0, clipped=4, busy=0, noisy=0, quiet=0, kind="blind", q_milli=None, q_min=None, q_max=None,
                                             all_milli=0)
    assert frame_says([clipped] * 7 + [same])["kind"] == "blind" and frame_says([clipped] * 6 + [same, busy])["kind"] == "steady"
    assert frame_says([same] * 4, [[0, 0, 0, 9, 0]] * 4)["kind"] == "blind"  # no baseline: nothing is rated
    assert frame_says([busy] * 3 + [same])["kind"] == "busy" and frame_says([busy, busy, same, same])["kind"] == "steady"
    assert frame_says([busy, clipped, clipped, same])["kind"] == "steady" and frame_says([busy, busy, clipped, same])["kind"] == "busy"
    s = frame_says([noisy, noisy, same, same])
    assert (s["kind"], s["noisy"], s["q_milli"], s["q_min"], s["q_max"]) == ("noisy", 2, 1500, 1000, 2000)
    assert frame_says([noisy, same, same, same])["kind"] == "uneven" and frame_says([noisy] * 4)["kind"] == "noisy"
    s = frame_says([quiet, quiet, same, same])
    assert (s["kind"], s["quiet"], s["q_milli"], s["q_min"], s["q_max"]) == ("quiet", 2, 750, 500, 1000)
    assert frame_says([quiet, same, same, same])["kind"] == "uneven" and frame_says([noisy, quiet, same, same])["kind"] == "uneven"
    assert frame_says([noisy, noisy, noisy, quiet])["kind"] == "uneven"
    # cells with baselines of their own: the pooled ratio weighs each by its baseline
    s = frame_says([rec_of(1000), [0, 0, 0, 400 * N, 0, 400 * N]], [BASE, [200 * N, N, 1, 5, 0]])
    assert (s["q_min"], s["q_max"], s["q_milli"], s["kind"]) == (1000, 2000, 1000 * 500 // 300, "noisy")


# ---- runs --------------------------------------------------------------------------------------------------------------------
def make_noise_run(root, w=W, h=H, plain=False):
    """8 events x 2 cameras x 8 frames of 267 x 137 (at R = 4 a grid of 2 x 1 cells, origin 5, 4): per camera a smooth
    background with Gaussian noise of sigma 3, rounded: a steady run.  Camera 0 does not train (its second frame differs from
    its first in every event, so the entropy veto leaves it no training frames).  Planted in camera 1: one event whose frames
    from 4 on have noise of sigma 6; one with a bright disc in the left cell from frame 5 on; one truncated file; one removed
    file; one wider frame at stack position 1.  plain: none of them.  The Trainer keeps an event only if the 16-bin histogram
    of frame 1 - frame 0 has all but nothing in its first bin, which two or three pixels at 16 or more already spoil, and at
    sigma 3 about five of a pair's 36,579 pixels are: in frame 1 those pixels' noise is drawn again, so that the events train
    -> (run dir, {(event, cam, name): image, None (does not decode) or "missing"})"""
    rs = np.random.RandomState(53)
    rd = os.path.join(root, RUN_ID)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = {}
    for e in range(NEV):
        os.makedirs(os.path.join(rd, str(e), "Images"))
        for c in range(NCAMS):
            back = 120 + 30 * np.sin(xx / 37.0 + c) + 20 * np.cos(yy / 29.0)
            for k in range(F):
                sd = 2 * SIGMA if not plain and (e, c) == (NOISY_EVENT, 1) and k >= NOISY_FROM else SIGMA
                img = back + sd * rs.standard_normal((h, w))
                if k == 1:
                    first = frames[(e, c, f"cam{c}_image30.png")].astype(np.int64)
                    while True:
                        high = np.rint(img) - first >= 16
                        if not high.any():
                            break
                        img[high] = back[high] + sd * rs.standard_normal(int(high.sum()))
                if not plain and (e, c) == (DISC_EVENT, 1) and k >= DISC_FROM:
                    img[(xx - DISC[0]) ** 2 + (yy - DISC[1]) ** 2 <= DISC[2] ** 2] += 80
                if c == UNTRAINED and k == 1:
                    img[:, :w // 2] += 70
                frames[(e, c, f"cam{c}_image{30 + k}.png")] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if not plain:
        frames[WIDER] = np.ascontiguousarray(np.pad(frames[WIDER], ((0, 0), (0, 4)), mode="edge"))
    for (e, c, name), img in frames.items():
        open(os.path.join(rd, str(e), "Images", name), "wb").write(png_bytes(img))
    if not plain:
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


def expected_noise(rd, frames, radius=R, w=W, h=H, models=None):
    """-> (noise.txt, {cam: the array of cam<c>_noise.npy}, {cam: that of cam<c>_noise_model.npy}, the models)"""
    models = trained_models(rd, w, h) if models is None else models
    rows = noiseref.rows_of(stacks_of(frames), w, h, models, radius)
    return (noiseref.report(models, rows, w, h, radius), noiseref.arrays(models, rows, w, h, radius),
            noiseref.model_arrays(models, rows, w, h, radius), models)


def welford_models(frames):
    """the models the Trainer would make of the run, without one: mean and truncated standard deviation of frames 0 and 1 of
    every event of camera 1 (what the issue's trial did); camera 0 has none"""
    tr = np.stack([img for (e, c, n), img in sorted(frames.items()) if c == 1 and n[-6:-4] in ("30", "31") and
                   not isinstance(img, str) and img is not None and img.shape == (H, W)]).astype(np.float64)
    return [None, dict(mu=np.rint(tr.mean(axis=0)).astype(np.uint8), sigma=np.floor(tr.std(axis=0)).astype(np.uint8))]


@pytest.fixture(scope="module")
def noise_run(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("noise_run"))
    return make_noise_run(os.path.join(root, "data"))


def read_noise(d):
    """the directory DIR/<run_ID> -> (noise.txt or None, {cam: records}, {cam: model records})"""
    if not os.path.isdir(d):
        return None, {}, {}
    arrays = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_noise.npy")}
    marr = {int(f[3:f.index("_")]): np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith("_noise_model.npy")}
    assert sorted(arrays) == sorted(marr)
    assert sorted(os.listdir(d)) == sorted(["noise.txt"] + [f"cam{c}_noise{s}.npy" for c in arrays for s in ("", "_model")])
    return open(os.path.join(d, "noise.txt")).read(), arrays, marr


def same_arrays(got, want, dtype=np.int32):
    return sorted(got) == sorted(want) and all(got[c].dtype == dtype and got[c].shape == want[c].shape and np.array_equal(got[c], want[c])
                                              for c in want)


def same_noise(got, want):
    return got[0] == want[0] and same_arrays(got[1], want[1]) and same_arrays(got[2], want[2], np.int64)


def noise_cli(src_args, stem, *more, env=ENV):
    """abub3hs --survey stem.txt --survey-noise stem_noise -> (the process, the report, (noise.txt, the arrays, the models'))"""
    r, text = survey_cli(src_args, stem + ".txt", "--survey-noise", stem + "_noise", *more, env=env)
    return r, text, read_noise(os.path.join(stem + "_noise", RUN_ID))


def check_kinds(text, arrays, marr, origin=GRID[:2]):
    """noise.txt of the run with a model of camera 1: every row says what was planted in its frame"""
    lines = text.splitlines()
    assert lines[:2] == ["# abub3hs noise 1", f"radius {R} cell 128 grid 2 1 origin {origin[0]} {origin[1]}"] and lines[2] + "\n" == noiseref.HEADER
    assert len(lines) == 3 + TOTAL + NCAMS + 1 + 1
    index, kinds = 0, {k: 0 for k in noiseref.KINDS}
    for l in lines[3:3 + TOTAL]:
        r = l.split("\t")
        assert len(r) == 16
        e, c, k, name = int(r[0]), int(r[1]), int(r[2]), r[3]
        ref = (e, c, f"cam{c}_image{30 + max(k - 2, 0)}.png")
        if c == UNTRAINED or k < 1 or (e, c, name) in (TRUNCATED, REMOVED, WIDER) or ref in (TRUNCATED, REMOVED, WIDER):
            assert r[5:] == ["-"] * 11, r
            continue
        assert r[4] == "ok" and int(r[5]) == index, r
        index += 1
        kinds[r[15]] += 1
        over = arrays[1][int(r[5]), 0, :, 0]
        if e == NOISY_EVENT and k >= NOISY_FROM:  # doubled noise: a variance 2.5 times (one frame of the pair) or 4 times the baseline
            assert r[6:11] == ["2", "0", "0", "2", "0"] and r[15] == "noisy" and 1800 < int(r[12]) and int(r[13]) < 4800, r
            assert (over * 4 < N * 0.8).all(), over  # (well below the busy share)
        elif e == DISC_EVENT and k in (DISC_FROM, DISC_FROM + 1):  # the disc against a frame without it: over pixels, not noise
            assert r[6:11] == ["2", "0", "0", "0", "0"] and r[15] == "steady" and int(r[14]) > 10000, r
            assert 2700 < over[0] < 3100 and over[1] < 200, over
        else:  # steady, the disc against itself (frame 7 of its event) included
            assert r[6:11] == ["2", "0", "0", "0", "0"] and r[15] == "steady" and 800 < int(r[12]) <= int(r[13]) < 1200, r
            assert (over < 250).all(), over
    steady = index - (F - NOISY_FROM)
    assert kinds == dict(blind=0, busy=0, steady=steady, noisy=F - NOISY_FROM, quiet=0, uneven=0)
    assert index == NEV * (F - 1) - 3 * 2  # the truncated, the removed and the wider frame and the frames they are the reference of
    assert lines[3 + TOTAL] == f"noise cam {UNTRAINED} none"
    cam = lines[4 + TOTAL].split(" ")
    assert cam[:17] == f"noise cam 1 frames {index} blind 0 busy 0 steady {steady} noisy {F - NOISY_FROM} quiet 0 uneven 0".split(" ")
    assert cam[17:20] == ["first_changed_event", str(NOISY_EVENT), "model_milli"] and len(cam) == 22
    assert all(400 < int(v) < 2500 for v in cam[20:])  # the u8 sigma plane is truncated: of the order of 1000, not near it
    assert lines[5 + TOTAL:] == [f"changed cam 1 y 0 {F - NOISY_FROM} {F - NOISY_FROM}",
                                 f"run frames {index} blind 0 busy 0 steady {steady} noisy {F - NOISY_FROM} quiet 0 uneven 0"]
    assert (marr[1][..., 2] == NEV - 1).all()  # the baseline: every event's frame 1 but the wider one
    assert arrays[1].shape == (index, 1, 2, 6) and marr[1].shape == (1, 2, 5)


def test_the_restatement_sees_what_was_planted(noise_run):
    """the run is what its description says, with the mean and the truncated standard deviation of the training frames as
    the model; no figure comes within 20 % of a threshold of the rule"""
    _, frames = noise_run
    models = welford_models(frames)
    assert GRID == tuple(np.roll(noiseref.grid(W, H, R), 2)) and np.median(models[1]["sigma"]) == 2  # (truncated: 6 sigma is 12, not 18)
    text, arrays, marr, _ = expected_noise(None, frames, models=models)
    check_kinds(text, arrays, marr)
    q = [int(l.split("\t")[k]) for l in text.splitlines()[3:3 + TOTAL] if l.split("\t")[12] != "-" for k in (12, 13)]
    assert all(v > 1.2 * noiseref.NOISY_MILLI or 1.2 * noiseref.QUIET_MILLI < v < 0.8 * noiseref.NOISY_MILLI for v in q), sorted(q)


def others(tmp_path, tag):
    """the flags of every other product of a survey, into places of their own"""
    return ["--survey-planes", str(tmp_path / f"planes_{tag}"), "--survey-shift", str(tmp_path / f"shift_{tag}.txt"), "--survey-field",
            str(tmp_path / f"field_{tag}"), "--survey-light", str(tmp_path / f"light_{tag}"), "--survey-focus", str(tmp_path / f"focus_{tag}")]


def same_others(tmp_path, a, b):
    """every other product's files of the calls tagged a and b are the same bytes"""
    if open(str(tmp_path / f"shift_{a}.txt"), "rb").read() != open(str(tmp_path / f"shift_{b}.txt"), "rb").read():
        return False
    for kind in ("planes", "field", "light", "focus"):
        da, db = (os.path.join(str(tmp_path / f"{kind}_{tag}"), RUN_ID) for tag in (a, b))
        if sorted(os.listdir(da)) != sorted(os.listdir(db)) or not os.listdir(da):
            return False
        if any(open(os.path.join(da, f), "rb").read() != open(os.path.join(db, f), "rb").read() for f in os.listdir(da)):
            return False
    return True


def test_cli_host_route_and_nothing_else_changes(noise_run, tmp_path):
    """the files against the restatement, byte for byte; the report and every other product's files are the same bytes with
    the flag and without it; alone, the noise is the same again"""
    rd, frames = noise_run
    src = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    want = expected_noise(rd, frames)
    plain, report_plain = survey_cli(src, str(tmp_path / "plain.txt"), *others(tmp_path, "plain"))
    r, report, got = noise_cli(src, str(tmp_path / "with"), *others(tmp_path, "with"))
    assert r.returncode == plain.returncode == 1, (r.stdout, r.stderr)  # (the damaged files: the survey's status)
    assert report == report_plain and report is not None and same_others(tmp_path, "with", "plain")
    assert same_noise(got, want), got[0]
    assert "survey-noise: " in r.stdout and "survey-noise" not in plain.stdout
    r, report, alone = noise_cli(src, str(tmp_path / "alone"))
    assert r.returncode == 1 and report == report_plain and same_noise(alone, want)
    models = want[3]
    assert models[UNTRAINED] is None and f"noise cam {UNTRAINED} none\n" in want[0]
    if models[1] is not None:  # (the host Trainer needs a device: without one no camera has a model, and the files say so)
        check_kinds(*got)
    else:
        assert "noise cam 1 none\n" in want[0] and not got[1] and not got[2]
    want2 = expected_noise(rd, frames, 2, models=models)  # the field's radius places the noise's cells
    r, report, got = noise_cli(src, str(tmp_path / "r2"), "--survey-field-radius", "2")
    assert r.returncode == 1 and same_noise(got, want2) and report == report_plain
    assert want2[0].splitlines()[1] == "radius 2 cell 128 grid 2 1 origin 5 4"


def test_run_survey_agrees_with_the_cli(noise_run, tmp_path):
    rd, frames = noise_run
    want = expected_noise(rd, frames)
    run = host.Run("raw", rd + "/", "Images")
    try:
        plain, text_plain = run.survey(nthreads=4, ncams=NCAMS)
        res, text = run.survey(str(tmp_path / "r.txt"), nthreads=4, ncams=NCAMS, noise=str(tmp_path / "n"))
        with pytest.raises(RuntimeError, match="radius"):
            run.survey(nthreads=4, ncams=NCAMS, noise=str(tmp_path / "bad"), field_radius=9)
    finally:
        run.close()
    assert text == text_plain and same_noise(read_noise(str(tmp_path / "n")), want) and not os.path.exists(str(tmp_path / "bad"))
    records = sum(len(a) for a in want[1].values())
    assert res["noise_frames_kernel"] == 0 and res["noise_launches"] == 0 and res["noise_frames_host"] == records
    assert "noise_frames_host" not in plain and "light_frames_host" not in res
    assert {k: v for k, v in res.items() if k in plain and not k.endswith("_s") and k != "seconds"} == \
           {k: v for k, v in plain.items() if not k.endswith("_s") and k != "seconds"}


def test_cli_flags_and_refusals(noise_run, tmp_path):
    rd, _ = noise_run
    src = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli("-h")
    assert "--survey-noise = Dir" in r.stdout and "[--survey-noise DIR [--survey-field-radius R]]" in r.stdout
    out, nd = str(tmp_path / "s.txt"), str(tmp_path / "noise")
    r = cli(*src, "-o", str(tmp_path), "--survey-noise", nd)
    assert r.returncode != 0 and "--survey-noise is valid only together with --survey" in r.stderr and not os.path.exists(nd)
    r = cli(*src, "--survey", out, "--survey-noise", nd, "--survey-shift-radius", "2")
    assert r.returncode != 0 and "--survey-shift-radius is valid only together with --survey-shift" in r.stderr
    for radius in ("0", "9", "four"):
        r = cli(*src, "--survey", out, "--survey-noise", nd, "--survey-field-radius", radius)
        assert r.returncode != 0 and "--survey-field-radius expects a radius from 1 to 8" in r.stderr, radius
    r = cli(*src, "--survey", out, "--survey-noise")
    assert r.returncode != 0 and "--survey-noise needs the directory to write to" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(nd)
    r = cli(*src, "--survey", out, "--survey-noise", os.path.dirname(rd))
    assert r.returncode != 0 and "is the run that is being read" in r.stderr and not os.path.exists(out)
    assert not os.path.exists(os.path.join(rd, "noise.txt"))


def test_a_run_without_a_whole_cell_is_refused(tmp_path):
    """the existing message, with the noise's name for what it cannot make"""
    rd, _ = make_noise_run(str(tmp_path / "data"), w=135, h=200, plain=True)
    out, nd = str(tmp_path / "s.txt"), str(tmp_path / "noise")
    args = ["-d", os.path.dirname(rd), "-r", RUN_ID]
    r = cli(*args, "--survey", out, "--survey-noise", nd)
    assert r.returncode != 0 and "survey: the noise records at radius 4 need frames of at least 136x136, the run's are 135x200" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(nd)
    r = cli(*args, "--survey", out, "--survey-noise", nd, "--survey-field-radius", "3")  # 135 = 128 + 2 * 3 + 1: one cell across
    assert r.returncode == 0 and os.path.exists(out), r.stderr
    assert open(os.path.join(nd, RUN_ID, "noise.txt")).read().startswith("# abub3hs noise 1\nradius 3 cell 128 grid 1 1 origin 3 36\n")
