"""Bellows-movement veto inside the batched pipeline (L3Localizer.cpp:292-390, TrackAFeature :473-510): the batched exact
template matcher (abub_match_ccorr_batch_dev), the best match computed on the device (abub_match_best_batch_dev) against
the host's bestMatchFromTerms, and the pipeline's veto round against the oracle."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest
from PIL import Image

from matchref import match_geometry, same_xy

from autobub3hs_amd import _lib, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("abub_match_ccorr_batch_dev", "abub_match_best_batch_dev", "abub_match_best_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def test_new_exports_declared_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "abub_hip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.build())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert hasattr(C.CDLL(os.path.join(ROOT, "autobub3hs_amd", "libabub_host.so")), "abh_pipe_bellows")


def test_argument_validation_before_the_device():
    L = _lib.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below must be refused up front
    s = L.abub_match_best_scratch_bytes(64, 32, 8, 4, 3)
    assert s > 0 and L.abub_match_best_scratch_bytes(64, 32, 65, 4, 3) == 0
    assert L.abub_match_best_scratch_bytes(64, 32, 8, 4, 0) == 0
    cases = [
        (64, 32, 65, 4, 3),  # template wider than the frame
        (64, 32, 8, 33, 3),  # taller
        (64, 32, 8, 4, 0),   # no jobs
        (64, 32, 8, 4, -1),
        (64, 32, 0, 4, 3),
    ]
    for W, H, tw, th, nj in cases:
        assert L.abub_match_ccorr_batch_dev(fake, W, H, fake, nj, fake, tw, th, fake, fake, None) == -1  # ABUB_E_INVALID
        assert L.abub_match_best_batch_dev(fake, W, H, fake, nj, fake, tw, th, fake, fake, 1 << 30, None) == -1
    # scratch one byte too small, null pointers
    assert L.abub_match_best_batch_dev(fake, 64, 32, fake, 3, fake, 8, 4, fake, fake, s - 1, None) == -1
    assert L.abub_match_best_batch_dev(fake, 64, 32, fake, 3, fake, 8, 4, fake, None, s, None) == -1
    assert L.abub_match_ccorr_batch_dev(None, 64, 32, fake, 3, fake, 8, 4, fake, fake, None) == -1
    assert b"bad arguments" in L.abub_last_error()


def exact_terms(img, tmpl):
    """num = sum(T*I), wsum2 = sum(I*I) per placement, in u64 (vectorised over the template taps)."""
    I = img.astype(np.uint64)
    T = tmpl.astype(np.uint64)
    th, tw = tmpl.shape
    rh, rw = img.shape[0] - th + 1, img.shape[1] - tw + 1
    num = np.zeros((rh, rw), np.uint64)
    w2 = np.zeros((rh, rw), np.uint64)
    for r in range(th):
        for c in range(tw):
            win = I[r:r + rh, c:c + rw]
            num += T[r, c] * win
            w2 += win * win
    return num, w2


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
def test_batch_terms_exact_small_shapes():
    import torch

    from autobub3hs_amd import hip

    dev = "cuda:0"
    rng = np.random.RandomState(5)
    for (H, W, th, tw) in [(20, 30, 5, 1), (40, 37, 9, 3), (33, 70, 33, 7), (50, 71, 11, 13), (36, 333, 7, 300),
                           (17, 19, 1, 1), (45, 130, 24, 6)]:
        frames = rng.randint(0, 256, (5, H, W)).astype(np.uint8)
        frames[2] = 255  # saturated frame: the largest products
        tmpl = rng.randint(0, 256, (th, tw)).astype(np.uint8)
        idx = np.array([3, 0, 2, 4, 2], np.int32)
        num, w2 = hip.match_terms(torch.from_numpy(frames).to(dev), torch.from_numpy(idx).to(dev),
                                  torch.from_numpy(tmpl).to(dev))
        num, w2 = _u64(num), _u64(w2)
        for k, f in enumerate(idx):
            en, ew = exact_terms(frames[f], tmpl)
            assert np.array_equal(num[k], en), (H, W, th, tw, k)
            assert np.array_equal(w2[k], ew), (H, W, th, tw, k)


def _old_terms(img_d, tmpl_d, W, H, tw, th):
    import torch

    rh, rw = H - th + 1, W - tw + 1
    num = torch.zeros((rh, rw), dtype=torch.int64, device=img_d.device)
    w2 = torch.zeros_like(num)
    _lib.check(_lib.lib().abub_match_ccorr_dev(img_d.data_ptr(), W, H, tmpl_d.data_ptr(), tw, th, num.data_ptr(),
                                               w2.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return num, w2


def _real_frame_and_template():
    """A 1680 x 1050 frame tiled from the committed 40l-19 camera-1 sample and the committed template crop, stretched to
    the real cam1 template size (178 x 557)."""
    img = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    reps = (1050 // img.shape[0] + 1, 1680 // img.shape[1] + 1)
    frame = np.tile(img, reps)[:1050, :1680].copy()
    t = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_bellows_template.png")).convert("L"))
    tmpl = np.array(Image.fromarray(t).resize((178, 557), Image.NEAREST))
    return frame, tmpl


@pytest.mark.gpu
def test_batch_terms_equal_per_event_kernel_at_full_size():
    import torch

    from autobub3hs_amd import hip

    dev = "cuda:0"
    frame, tmpl = _real_frame_and_template()
    H, W = frame.shape
    th, tw = tmpl.shape
    bright = np.full_like(frame, 250)
    frames = torch.from_numpy(np.stack([frame, bright])).to(dev)
    t_d = torch.from_numpy(tmpl).to(dev)
    num, w2 = hip.match_terms(frames, torch.tensor([0, 1, 0], dtype=torch.int32, device=dev), t_d)
    for k, f in enumerate((0, 1, 0)):
        on, ow = _old_terms(frames[f].contiguous(), t_d, W, H, tw, th)
        assert torch.equal(num[k], on) and torch.equal(w2[k], ow), k


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,tw,th,njobs", [(1680, 1050, 178, 557, 12), (4096, 60, 4000, 40, 2)])
def test_batch_terms_u64_flush(W, H, tw, th, njobs):
    """Shapes where one workgroup walks more image rows than fit in the u32 sums: the flush to u64 must run (the
    geometry is asserted), on a saturated frame (closed form) and on the camera sample (the per-event kernel)."""
    import torch

    from autobub3hs_amd import hip

    nsplit, rsplit, flush = match_geometry(W, H, tw, th, njobs)
    assert nsplit == 1 and rsplit > flush, (nsplit, rsplit, flush)
    dev = "cuda:0"
    img = np.array(Image.open(os.path.join(GOLDEN, "sample_40l19_cam1_image30.png")).convert("L"))
    sample = np.tile(img, (H // img.shape[0] + 1, W // img.shape[1] + 1))[:H, :W]
    frames = torch.from_numpy(np.stack([sample, np.full((H, W), 255, np.uint8)])).to(dev)
    rng = np.random.RandomState(8)
    for tmpl in (np.full((th, tw), 255, np.uint8), rng.randint(0, 256, (th, tw)).astype(np.uint8)):
        t_d = torch.from_numpy(tmpl).to(dev)
        idx = torch.tensor([1, 0] * (njobs // 2), dtype=torch.int32, device=dev)
        num, w2 = hip.match_terms(frames, idx, t_d)
        if tmpl.min() == 255:
            assert int(num[0].min()) == int(num[0].max()) == 255 * 255 * tw * th > (1 << 32)
            assert int(w2[0].min()) == int(w2[0].max()) == 255 * 255 * tw * th
        for k in (0, 1):
            on, ow = _old_terms(frames[k].contiguous(), t_d, W, H, tw, th)
            j = 1 - k
            assert torch.equal(num[j], on) and torch.equal(w2[j], ow), k
            assert torch.equal(num[j + 2 * (njobs // 2 - 1)], on), k


def _device_best(frames_np, idx, tmpl):
    import torch

    from autobub3hs_amd import hip

    dev = "cuda:0"
    out = hip.match_best(torch.from_numpy(np.ascontiguousarray(frames_np)).to(dev),
                         torch.tensor(idx, dtype=torch.int32, device=dev), torch.from_numpy(tmpl).to(dev))
    return out.cpu().numpy()


@pytest.mark.gpu
def test_best_match_on_device_equals_host_bit_for_bit(oracle):
    rng = np.random.RandomState(11)
    for trial in range(7):
        H, W, th, tw = 40 + trial, 64 + 3 * trial, 9 + trial, 12 - trial
        img = rng.randint(0, 256, (H, W)).astype(np.uint8)
        y0, x0 = rng.randint(0, H - th), rng.randint(0, W - tw)
        tmpl = np.clip(img[y0:y0 + th, x0:x0 + tw].astype(int) + rng.randint(-6, 7, (th, tw)), 0, 255).astype(np.uint8)
        if trial == 5:  # maximum in a corner: neighbours outside the plane
            tmpl = img[:th, :tw].copy()
        if trial == 6:  # last corner
            tmpl = img[H - th:, W - tw:].copy()
        other = rng.randint(0, 256, (H, W)).astype(np.uint8)
        flat = np.full((H, W), 77, np.uint8)  # flat plane: smax - smin <= DBL_EPSILON
        frames = np.stack([img, other, flat])
        got = _device_best(frames, [0, 1, 2, 0], tmpl)
        for k, f in enumerate((0, 1, 2, 0)):
            num, w2 = exact_terms(frames[f], tmpl)
            hx, hy = host.best_match(num, w2, tmpl)
            assert same_xy(got[k], (hx, hy)), (trial, k, got[k], hx, hy)
            ox, oy = oracle.track_feature(frames[f], tmpl)
            assert same_xy(got[k], (ox, oy)), (trial, k, got[k], ox, oy)


@pytest.mark.gpu
def test_best_match_on_device_equals_host_on_the_real_frame():
    import torch

    frame, tmpl = _real_frame_and_template()
    shifted = np.roll(frame, (3, -5), axis=(0, 1))
    frames = np.stack([frame, shifted])
    got = _device_best(frames, [0, 1], tmpl)
    dev = "cuda:0"
    t_d = torch.from_numpy(tmpl).to(dev)
    H, W = frame.shape
    for k in range(2):
        num, w2 = _old_terms(torch.from_numpy(frames[k]).to(dev), t_d, W, H, tmpl.shape[1], tmpl.shape[0])
        hx, hy = host.best_match(_u64(num), _u64(w2), tmpl)
        assert same_xy(got[k], (hx, hy)), (k, got[k], hx, hy)


# ---- the pipeline's veto round ---------------------------------------------------------------------------------------

def write_bmp8(path, img):
    H, W = img.shape
    stride = (W + 3) // 4 * 4
    pal = b"".join(struct.pack("<BBBB", i, i, i, 0) for i in range(256))
    data = b"".join(img[y].tobytes() + b"\0" * (stride - W) for y in range(H - 1, -1, -1))
    off = 14 + 40 + len(pal)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", off + len(data), 0, 0, off))
        f.write(struct.pack("<IiiHHIIiiII", 40, W, H, 1, 8, 0, len(data), 2835, 2835, 256, 0))
        f.write(pal + data)


def bellows_event(W, H, F, t0, shift):
    """A textured 'bellows' block that creeps one pixel per frame from t0 (for 8 frames): the trigger fires and every
    genesis contour lies inside the bellows mask."""
    spec = synth.EventSpec(F)
    fr = synth.render_event(W, H, spec, 77, 0).astype(int)
    yy, xx = np.mgrid[:50, :30]
    tex = (60 + 50 * ((yy // 5 + xx // 5) % 2) + 25 * np.sin(xx / 2.0) + 20 * np.cos(yy / 3.0)).astype(int)
    bx0, by0 = 140, 40
    for f in range(F):
        x = bx0 + (min(f - t0 + 1, 8) if f >= t0 else 0) * (1 if shift > 0 else -1)
        fr[f, by0:by0 + 50, x:x + 30] = tex
    return np.clip(fr, 0, 255).astype(np.uint8), np.clip(tex, 0, 255).astype(np.uint8), (bx0, by0)


def _scene(tmp_path, oracle):
    W, H, F, t0 = 200, 120, 24, 12
    fr, tex, (bx0, by0) = bellows_event(W, H, F, t0, shift=2)
    tr = synth.training_pairs(W, H, 8, 0, F)
    for k in range(len(tr)):
        tr[k, by0:by0 + 50, bx0:bx0 + 30] = tex
    mu, sg = oracle.welford(tr)
    bel = np.zeros((H, W), np.uint8)
    bel[by0 - 10:by0 + 60, bx0 - 10:bx0 + 45] = 255
    write_bmp8(os.path.join(tmp_path, "cam0_bellows_mask.bmp"), bel)
    Image.fromarray(tex).save(os.path.join(tmp_path, "cam0_bellows_template.png"))
    plain = synth.render_event(W, H, synth.EventSpec(F, t0=10, bubbles=[(60, 60, 40)]), 5, 0)
    return (W, H, F), [fr, plain], tex, bel, mu, sg, len(tr)


def _run_pipeline(tmp_path, oracle, with_sigma, env=None):
    import torch

    from autobub3hs_amd import hip

    dev = "cuda:0"
    (W, H, F), stacks, tex, bel, mu, sg, tss = _scene(tmp_path, oracle)
    slab = np.stack(stacks)[:, None]  # [E=2][C=1][F][H][W]
    d_slab = torch.from_numpy(np.ascontiguousarray(slab)).to(dev)
    d_mu = torch.from_numpy(mu[None]).to(dev)
    d_sg = torch.from_numpy(sg[None]).to(dev)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        pipe = host.Pipeline(0, W, H, F, 2, 1, [tss], nthreads=2, maskdir=str(tmp_path))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pipe.run(d_slab, d_mu, hip.sigma6(d_sg), torch.cuda.current_stream().cuda_stream, sigma=d_sg if with_sigma else None)
    for s, stack in enumerate(stacks):
        staged, state, bubbles, err = pipe.result(s)
        a = oracle.Analyzer(stack, mu, sg, tss, bel_mask=bel, bel_template=tex)
        ref = a.any_cam_analysis()
        a.close()
        assert (staged, state) == (ref[0], ref[1]), (s, staged, state, ref[0], ref[1], err)
        assert [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in bubbles] == \
               [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in ref[2]]
    return pipe


@pytest.mark.gpu
def test_pipeline_runs_the_veto_in_the_batch(tmp_path, oracle):
    pipe = _run_pipeline(tmp_path, oracle, with_sigma=True)
    assert pipe.timing()["dropin_stacks"] == 0
    st = pipe.bellows_stats()
    assert st["vetoed"] == 1 and st["match_jobs"] == 2 and st["match_launches"] == 1 and st["residual_images"] == 1, st
    pipe.close()


@pytest.mark.gpu
def test_pipeline_veto_list_grows_on_overflow(tmp_path, oracle):
    """ABUB_PIPE_PAIRCAP also seeds the veto's candidate list: the residual's candidates overflow it, the list grows and
    the veto's K4 is redone -- the same results and veto counts as with the default capacity."""
    pipe = _run_pipeline(tmp_path, oracle, with_sigma=True, env={"ABUB_PIPE_PAIRCAP": "16"})
    assert pipe.timing()["dropin_stacks"] == 0
    st = pipe.bellows_stats()
    assert st["vetoed"] == 1 and st["match_jobs"] == 2 and st["match_launches"] == 1 and st["residual_images"] == 1, st
    pipe.close()


@pytest.mark.gpu
def test_pipeline_veto_without_raw_sigma(tmp_path, oracle):
    pipe = _run_pipeline(tmp_path, oracle, with_sigma=False)
    assert pipe.timing()["dropin_stacks"] == 0 and pipe.bellows_stats()["vetoed"] == 1
    pipe.close()


@pytest.mark.gpu
def test_pipeline_dropin_knob_keeps_the_old_route(tmp_path, oracle):
    pipe = _run_pipeline(tmp_path, oracle, with_sigma=True, env={"ABUB_PIPE_BELLOWS": "dropin"})
    assert pipe.timing()["dropin_stacks"] == 1 and pipe.bellows_stats()["vetoed"] == 0
    pipe.close()


# ---- real 40l-19 geometry: full-size masks and templates (tests/golden/bellows40l19.npz) -----------------------------

def _real_scene():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bellows40l19_scene", os.path.join(GOLDEN, "bellows40l19_scene.py"))
    sc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sc)
    return sc


def _rows(staged, state, bubbles):
    return staged, {k: state[k] for k in ("trig", "status", "ok", "loc_thres")}, \
        [[[d[k] for k in "xywh"] for d in b["desc"]] for b in bubbles]


@pytest.mark.gpu
def test_real_geometry_three_routes_equal_the_oracle(tmp_path):
    import torch

    from autobub3hs_amd import hip

    sc = _real_scene()
    fx = sc.fixture()
    exp = json.load(open(os.path.join(GOLDEN, "bellows40l19_expected.json")))
    sc.write_masks(fx, str(tmp_path))
    E, C = len(sc.KINDS), sc.C
    want = {(r["event"], r["cam"]): (r["staged"], r["state"], r["bubbles"]) for r in exp["stacks"]}
    trs = [sc.training(fx, c) for c in range(C)]
    run = host.Run()
    models = []
    for c in range(C):
        for e in range(sc.NTRAIN):  # (the Trainer takes frames 0 and 1 of each training event)
            pair = trs[c][2 * e:2 * e + 2]
            run.add_event(1000 + e, c, np.concatenate([pair, pair, pair]))
    for c in range(C):
        st, tss, mu, sg = run.train(c)
        assert st == 0 and tss == 2 * sc.NTRAIN
        models.append((mu, sg))
    stacks = [[sc.stack(fx, e, c) for c in range(C)] for e in range(E)]
    # route 1: the per-event path (EventOnDevice, abub_match_ccorr_dev + host normalisation)
    for e in range(E):
        for c in range(C):
            run.add_event(e, c, stacks[e][c])
            staged, state, bubbles, err = run.analyze(e, c, maskdir=str(tmp_path))
            assert _rows(staged, state, bubbles) == want[(e, c)], ("per-event", e, c, err)
    run.close()
    # routes 2 and 3: the batched pipeline, veto in the batch and through the drop-in path
    dev = "cuda:0"
    d_slab = torch.from_numpy(np.ascontiguousarray(np.stack([np.stack(s) for s in stacks]))).to(dev)
    del stacks
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(dev)
    d_sg = torch.from_numpy(np.stack([m[1] for m in models])).to(dev)
    s6 = hip.sigma6(d_sg)
    for mode in ("batched", "dropin"):
        if mode == "dropin":
            os.environ["ABUB_PIPE_BELLOWS"] = "dropin"
        try:
            pipe = host.Pipeline(0, sc.W, sc.H, sc.F, E, C, [2 * sc.NTRAIN] * C, nthreads=4, maskdir=str(tmp_path))
        finally:
            os.environ.pop("ABUB_PIPE_BELLOWS", None)
        pipe.run(d_slab, d_mu, s6, torch.cuda.current_stream().cuda_stream, sigma=d_sg if mode == "dropin" else None)
        for e in range(E):
            for c in range(C):
                staged, state, bubbles, err = pipe.result(e * C + c)
                assert _rows(staged, state, bubbles) == want[(e, c)], (mode, e, c, err)
        st = pipe.bellows_stats()
        if mode == "batched":
            assert pipe.timing()["dropin_stacks"] == 0 and st["vetoed"] >= 1, st
        else:
            assert st["vetoed"] == 0 and pipe.timing()["dropin_stacks"] >= 1
        pipe.close()
