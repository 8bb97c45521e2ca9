"""K5 (abub_contours.hip) against the host's contour finder and the oracle: count, order and vertices of every contour,
exactly; the limits and the declined slots; the overflow convention; the production call chain; the pipeline's "contours"
knob against the oracle and against the host route."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import blobscenes as bs  # noqa: E402
import contourscenes as cs  # noqa: E402
from autobub3hs_amd import _lib, host, synth  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def limits():
    from autobub3hs_amd import hip

    return hip.trace_contours_limits()


def _check_traced(out, s, frame, what=""):
    assert out["status"][s] == 0, (what, s)
    got, ref = cs.contours_of(out, s), cs.host_contours(frame)
    assert cs.same(got, ref), (what, s, [g.tolist() for g in got][:3], [r.tolist() for r in ref][:3])
    return got


def _check_stats(out):
    st, n = out["stats"], len(out["status"])
    declined = int((out["status"] != 0).sum())
    assert (st[0], st[1], st[2], st[3]) == (n - declined, declined, out["cont_off"][-1], out["pt_off"][-1])
    assert out["cont_off"][0] == 0 and np.array_equal(np.diff(out["cont_off"]), out["ncont"])


# ---- 1. random masks ------------------------------------------------------------------------------------------------------

def test_random_masks_equal_host_and_oracle(oracle):
    H = W = 44
    rs = np.random.RandomState(11)
    masks = cs.masks(rs)
    assert len(masks) >= 200
    frames = [cs.place(m, H, W, rs.randint(0, 2)) for m in masks]  # (a row or column longer than the frame is cut to it)
    out = cs.launch(frames, W, H)
    assert (out["status"] == 0).all()
    for s, f in enumerate(frames):
        got = _check_traced(out, s, f)
        ref = [xy for xy, _ in oracle.find_contours(f.astype(np.uint8) * 255)]
        assert cs.same(got, ref), s
    _check_stats(out)
    # deterministic: a second launch writes the same arrays
    out2 = cs.launch(frames, W, H)
    for k in ("status", "ncont", "cont_off", "pt_off", "stats"):
        assert np.array_equal(out[k], out2[k]), k
    assert np.array_equal(out["pts"][:out["pt_off"][-1]], out2["pts"][:out2["pt_off"][-1]])
    assert np.array_equal(out["cont_npts"][:out["cont_off"][-1]], out2["cont_npts"][:out2["cont_off"][-1]])


# ---- 2. adversarial shapes --------------------------------------------------------------------------------------------------

def _ring_box_frames(H, W):
    """each rectangle of blobscenes.ring_boxes as a frame of its own, filled and as an outline"""
    out = []
    for x0, y0, x1, y1 in bs.ring_boxes(H, W):
        f = np.zeros((H, W), bool)
        f[y0:y1 + 1, x0:x1 + 1] = True
        out.append(("ring_box_filled", f))
        o = f.copy()
        o[y0 + 1:y1, x0 + 1:x1] = False
        out.append(("ring_box_outline", o))
    return out


@pytest.mark.parametrize("H,W", [(24, 40), (37, 322)])
def test_adversarial_shapes(limits, H, W):
    max_pixels, max_chain = limits
    named = [(n, getattr(bs, n)(H, W) > 0) for n in ("serpentine", "checkerboard", "diagonals", "antidiagonals", "rings", "comb",
                                                     "corners", "hlines", "vlines", "wrap_pair")]
    named += _ring_box_frames(H, W)[:6]
    frames = [f for _, f in named]
    out = cs.launch(frames, W, H)
    traced = 0
    for s, (name, f) in enumerate(named):
        if out["status"][s] == 0:
            got = _check_traced(out, s, f, name)
            traced += 1
            if name == "wrap_pair":  # (W-1, 0) and (0, 1): adjacent raster indices, no neighbours
                assert [g.tolist() for g in got] == [[[0, 1]], [[W - 1, 0]]]
        else:
            assert out["status"][s] == 1 and out["ncont"][s] == 0, name
            assert out["pt_off"][s] == out["pt_off"][s + 1], name
            chains = cs.chain_lengths(f)
            assert int(f.sum()) > max_pixels or max(chains) > max_chain, (name, int(f.sum()), max(chains))
    assert out["status"][[n for n, _ in named].index("wrap_pair")] == 0
    # at 24 x 40 every shape is inside the limits; at 37 x 322 most exceed the pixel limit and are declined
    assert traced == len(named) if (H, W) == (24, 40) else 3 <= traced < len(named)
    _check_stats(out)


# ---- 3. limits ----------------------------------------------------------------------------------------------------------------

def test_pixel_limit(limits):
    max_pixels, _ = limits
    H = W = 96
    frames, want = [], []
    for n in (max_pixels - 1, max_pixels, max_pixels + 1):
        frames += [bs.compact(H, W, n) > 0, bs.lattice(H, W, n, seed=n) > 0]
        want += [int(n > max_pixels)] * 2
    assert [int(f.sum()) for f in frames] == [max_pixels - 1] * 2 + [max_pixels] * 2 + [max_pixels + 1] * 2
    out = cs.launch(frames, W, H)
    assert out["status"].tolist() == want
    for s, f in enumerate(frames):
        if want[s] == 0:
            _check_traced(out, s, f)
        else:
            assert out["ncont"][s] == 0 and out["pt_off"][s] == out["pt_off"][s + 1]
    _check_stats(out)


def test_chain_limit_and_a_traced_slot_next_to_a_declined_one(limits):
    _, max_chain = limits
    n0 = max_chain // 2 + 1  # a 1-pixel-wide line of n pixels has a chain of 2 (n - 1) codes
    H, W = 3, n0 + 3
    frames = []
    for n in (n0, n0 + 1):
        f = np.zeros((H, W), bool)
        f[1, 1:1 + n] = True
        frames.append(f)
    blob = np.zeros((H, W), bool)
    blob[0:3, 2:7] = True
    blob[1, 4] = False
    frames = [blob, frames[0], blob, frames[1], blob]
    assert [max(cs.chain_lengths(f)) for f in frames[1::2]] == [max_chain, max_chain + 2]
    out = cs.launch(frames, W, H)
    assert out["status"].tolist() == [0, 0, 0, 1, 0]
    for s in (0, 1, 2, 4):
        _check_traced(out, s, frames[s])
    assert out["ncont"][3] == 0 and out["pt_off"][3] == out["pt_off"][4] and out["cont_off"][3] == out["cont_off"][4]
    _check_stats(out)


# ---- 4. overflow convention -----------------------------------------------------------------------------------------------------

def test_overflow_convention():
    from autobub3hs_amd import hip  # noqa: F401

    H = W = 44
    rs = np.random.RandomState(5)
    frames = [cs.place(m, H, W, rs.randint(0, 2)) for m in cs.masks(rs)[:80]]
    full = cs.launch(frames, W, H)
    nc, nv = int(full["cont_off"][-1]), int(full["pt_off"][-1])
    cont_cap, pts_cap = nc // 2, nv // 3
    assert cont_cap > 4 and pts_cap > 4
    offs, idx = cs.kept_list(frames)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)  # noqa: E731
    n = len(frames)
    d_off, d_idx = t(offs), t(idx)
    new = lambda k, fill=0: torch.full((k,), fill, dtype=torch.int32, device=DEV)  # noqa: E731
    status, ncont, cont_off, pt_off, stats = new(n), new(n), new(n + 1), new(n + 1), new(4)
    cont_npts, pts = new(cont_cap + 64, -7), new(pts_cap + 64, -7)
    L = _lib.lib()
    scratch = torch.empty((int(L.abub_trace_contours_scratch_bytes(n, len(idx))),), dtype=torch.uint8, device=DEV)
    _lib.check(L.abub_trace_contours_dev(d_off.data_ptr(), d_idx.data_ptr(), len(idx), n, W, H, status.data_ptr(),
                                         ncont.data_ptr(), cont_off.data_ptr(), cont_npts.data_ptr(), cont_cap,
                                         pt_off.data_ptr(), pts.data_ptr(), pts_cap, stats.data_ptr(), scratch.data_ptr(),
                                         scratch.numel(), torch.cuda.current_stream().cuda_stream), "abub_trace_contours_dev")
    torch.cuda.synchronize()
    # the true counts are reported
    for k, v in (("status", status), ("ncont", ncont), ("cont_off", cont_off), ("pt_off", pt_off), ("stats", stats)):
        assert np.array_equal(v.cpu().numpy(), full[k]), k
    # what fits is written, nothing at or past the capacities
    c, p = cont_npts.cpu().numpy(), pts.cpu().numpy()
    assert np.array_equal(c[:cont_cap], full["cont_npts"][:cont_cap]) and (c[cont_cap:] == -7).all()
    assert np.array_equal(p[:pts_cap], full["pts"][:pts_cap]) and (p[pts_cap:] == -7).all()


# ---- 5. the production chain ------------------------------------------------------------------------------------------------------

def test_production_chain_1280x96():
    """K4 pairs with the per-image TOZERO cut -> group by slot -> device Otsu -> K4b (comp = NULL) -> K5: the calls the
    batched pipeline makes with the contours knob on.  Per image the contours equal the host route's on the image's kept
    pixels, and K4b's kept pixels are the thresholded image's components that pass the box filter."""
    from autobub3hs_amd import hip

    W, H, n = 1280, 96, 96
    rs = np.random.RandomState(1280)
    img = np.zeros((n, H, W), np.uint8)
    noise = rs.rand(n, H, W) < 0.002
    img[noise] = rs.randint(1, 40, int(noise.sum()))
    yy, xx = np.mgrid[0:H, 0:W]
    for s in range(n):
        for _ in range(rs.randint(0, 5)):  # bubbles: discs of radius 1 .. 14, some over the border, some overlapping
            cy, cx, r = rs.randint(-3, H + 3), rs.randint(-3, W + 3), rs.randint(1, 15)
            d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            img[s][d] = np.maximum(img[s][d], rs.randint(60, 256, int(d.sum())))
    img[7] = 0  # a blank image
    tozero = rs.choice([3, 5, 10, 30], n).astype(np.int32)
    mb = np.where(np.arange(n) % 5 == 0, -1, 10).astype(np.int32)
    hist = np.stack([np.bincount(im.ravel(), minlength=256) for im in img])
    cap = int((img > tozero[:, None, None]).sum()) + 64
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    d_img, d_tz = torch.from_numpy(img).to(DEV), torch.from_numpy(tozero).to(DEV)
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    _lib.check(L.abub_fg_compact_pairs_dev(d_img.data_ptr(), n, W, H, d_tz.data_ptr(), pairs.data_ptr(), cap, count.data_ptr(),
                                           st), "abub_fg_compact_pairs_dev")
    gscratch = torch.zeros((2 * n,), dtype=torch.int32, device=DEV)
    offs = torch.empty((n + 1,), dtype=torch.int32, device=DEV)
    idx = torch.empty((cap,), dtype=torch.int32, device=DEV)
    val = torch.empty((cap,), dtype=torch.uint8, device=DEV)
    _lib.check(L.abub_pairs_group_dev(pairs.data_ptr(), count.data_ptr(), cap, n, gscratch.data_ptr(), offs.data_ptr(),
                                      idx.data_ptr(), val.data_ptr(), st), "abub_pairs_group_dev")
    otsu = hip.binarize_thr(torch.from_numpy(hist.astype(np.int32)).to(DEV), d_tz, W, H)
    lab = hip.label_blobs(offs, idx, val, otsu, torch.from_numpy(mb).to(DEV), W, H, comp=False)
    out = hip.trace_contours(lab["kept_off"], lab["kept_idx"], W, H)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    ko, ki, thr = lab["kept_off"].cpu().numpy(), lab["kept_idx"].cpu().numpy(), otsu.cpu().numpy()
    assert (out["status"] == 0).all()
    total = 0
    for s in range(n):
        kept = ki[ko[s]:ko[s + 1]]
        assert np.array_equal(kept, bs._reference(img[s], thr[s], mb[s])[2])
        f = np.zeros(H * W, bool)
        f[kept] = True
        total += len(_check_traced(out, s, f.reshape(H, W)))
    assert total > n and out["ncont"][7] == 0
    _check_stats(out)


# ---- 6. the pipeline's "contours" knob ------------------------------------------------------------------------------------------

def _oracle_event(oracle, fr, mu, sg, tss):
    a = oracle.Analyzer(fr, mu, sg, tss)
    out = a.any_cam_analysis()
    a.close()
    return out


def _boxes(bubbles):
    return [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in bubbles]


def _both_settings(pipe, run, S):
    """run with contours = 0, then 1, on the same pipeline object: per-stack results are identical, every slot of the
    second run was traced on the device -> (results of the second run, its contour_stats)"""
    res = []
    for v in (0, 1):
        pipe.set_option("contours", v)
        run()
        res.append([pipe.result(s) for s in range(S)])
        st = pipe.contour_stats()
        if v == 0:
            assert (st["traced"], st["host_route"], st["contours"], st["vertices"]) == (0, 0, 0, 0), st
    assert repr(res[0]) == repr(res[1])
    for r in res[1]:
        assert "Otsu" not in r[3] and "contoursKept" not in r[3], r[3]
    assert st["host_route"] == 0 and st["traced"] > 0 and 0 < st["contours"] <= st["vertices"], st
    assert st["k5_ms"] > 0
    return res[1], st


@pytest.mark.parametrize("W,H", [(1280, 128), (322, 120)])  # fused lists / K4 pairs on stored images (non-fast-path width)
def test_pipeline_contours_equals_oracle(oracle, W, H):
    from autobub3hs_amd import hip

    F, E, C_ = 41, 7, 2
    slab = np.zeros((E, C_, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C_):
            spec = synth.random_spec(W, H, F, 500 + e, c, p_second=0.4, p_none=0.2, p_flicker=0.3, margin=25)
            slab[e, c] = synth.render_event(W, H, spec, 500 + e, c)
    quiet = synth.render_event(W, H, synth.EventSpec(F), 900, 0)
    quiet[12:] = np.clip(quiet[12:].astype(int) + 1, 0, 255)
    slab[E - 1, 0] = quiet
    tr0, tr1 = synth.training_pairs(W, H, 10, 0, F), synth.training_pairs(W, H, 2, 1, F)
    models = [oracle.welford(tr0), oracle.welford(tr1)]
    tss = [len(tr0), len(tr1)]
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res, _ = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c])
            assert (staged, state) == (ref[0], ref[1]), (e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])
    pipe.close()


@pytest.mark.parametrize("regime", ["default", "post_trigger_dense", "noisy"])
def test_pipeline_contours_in_every_regime(oracle, regime):
    from autobub3hs_amd import hip

    W, H, F, E, C_ = 1280, 96, 41, 6, 2
    slab = np.zeros((E, C_, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C_):
            spec = synth.random_spec(W, H, F, 700 + e, c, p_second=0.3, p_none=0.15, p_flicker=0.3, margin=25, regime=regime)
            slab[e, c] = synth.render_event(W, H, spec, 700 + e, c)
    models, tss = [], []
    for c in range(C_):
        tr = np.concatenate([slab[e, c, :2] for e in range(E)])
        models.append(oracle.welford(tr))
        tss.append(len(tr))
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res, _ = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c])
            assert (staged, state) == (ref[0], ref[1]), (regime, e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])
    pipe.close()


def test_pipeline_contours_regrow_and_env_seed(oracle, monkeypatch):
    """ABUB_PIPE_PAIRCAP=64: the candidate list, and with it the contour and vertex lists, grow and the batch is redone;
    ABUB_PIPE_CONTOURS=1 seeds the knob"""
    from autobub3hs_amd import hip

    W, H, F, E = 1280, 96, 41, 4
    slab = np.zeros((E, 1, F, H, W), np.uint8)
    for e in range(E):
        spec = synth.random_spec(W, H, F, 300 + e, 0, p_second=0.5, margin=25)
        slab[e, 0] = synth.render_event(W, H, spec, 300 + e, 0)
    mu, sg = oracle.welford(synth.training_pairs(W, H, 8, 0, F))
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(mu[None]).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(sg[None]).to(DEV))
    st_ = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("ABUB_PIPE_PAIRCAP", "64")
    monkeypatch.setenv("ABUB_PIPE_CONTOURS", "1")
    pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    monkeypatch.delenv("ABUB_PIPE_PAIRCAP")
    monkeypatch.delenv("ABUB_PIPE_CONTOURS")
    pipe.run(d_slab, d_mu, d_s6, st_)
    assert pipe.timing()["pairs"] > 64
    st = pipe.contour_stats()  # the environment switched it on
    assert st["traced"] > 0 and st["host_route"] == 0 and st["vertices"] > 64 // 4 + 64, st  # more than the first lists held
    grown = [pipe.result(s) for s in range(E)]
    pipe.close()
    ref_pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    ref_pipe.run(d_slab, d_mu, d_s6, st_)
    assert ref_pipe.contour_stats()["traced"] == 0  # default: off
    assert repr(grown) == repr([ref_pipe.result(s) for s in range(E)])
    ref_pipe.close()
    ref = _oracle_event(oracle, slab[0, 0], mu, sg, 16)
    assert (grown[0][0], grown[0][1]) == (ref[0], ref[1])


def test_pipeline_contours_on_the_bellows_fixture(tmp_path):
    """the committed full-size 40l-19 scenes (bellows veto in the batch: residual images stay on the host route; the
    scenes' own images are above K5's pixel limit, so this is also the declined-slot route through the pipeline)"""
    from autobub3hs_amd import hip

    spec = importlib.util.spec_from_file_location("bellows40l19_scene", os.path.join(GOLDEN, "bellows40l19_scene.py"))
    sc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sc)
    fx = sc.fixture()
    exp = json.load(open(os.path.join(GOLDEN, "bellows40l19_expected.json")))
    sc.write_masks(fx, str(tmp_path))
    E, C_ = len(sc.KINDS), sc.C
    want = {(r["event"], r["cam"]): (r["staged"], r["state"], r["bubbles"]) for r in exp["stacks"]}
    run = host.Run()
    models = []
    for c in range(C_):
        tr = sc.training(fx, c)
        for e in range(sc.NTRAIN):
            pair = tr[2 * e:2 * e + 2]
            run.add_event(1000 + e, c, np.concatenate([pair, pair, pair]))
        st, tss, mu, sg = run.train(c)
        assert st == 0 and tss == 2 * sc.NTRAIN
        models.append((mu, sg))
    run.close()
    d_slab = torch.from_numpy(np.ascontiguousarray(np.stack([np.stack([sc.stack(fx, e, c) for c in range(C_)])
                                                             for e in range(E)]))).to(DEV)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    pipe = host.Pipeline(0, sc.W, sc.H, sc.F, E, C_, [2 * sc.NTRAIN] * C_, nthreads=4, maskdir=str(tmp_path))
    pipe.set_option("contours", 1)
    pipe.run(d_slab, d_mu, s6, torch.cuda.current_stream().cuda_stream)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = pipe.result(e * C_ + c)
            row = (staged, {k: state[k] for k in ("trig", "status", "ok", "loc_thres")},
                   [[[d[k] for k in "xywh"] for d in b["desc"]] for b in bubbles])
            assert row == want[(e, c)], (e, c, err)
    assert pipe.bellows_stats()["vetoed"] >= 1 and pipe.timing()["dropin_stacks"] == 0
    # The creep scenes light up the bellows strip: every image of this fixture has 5871 .. 6160 kept pixels (recounted on
    # the CPU with scipy on the oracle's post-trigger images), above K5's limit of 2048, so its slots are declined and take
    # the host route from the kept pixels the batch ships for them.  A slot declined for its pixel count is one K4b
    # labelled on its global-memory path (kept <= foreground).
    st, bst = pipe.contour_stats(), pipe.blob_stats()
    print(st, bst)
    assert st["traced"] + st["host_route"] > 0, st
    assert st["host_route"] <= bst["large_slots"], (st, bst)
    assert bst["kept"] > 2048 * st["host_route"], (st, bst)
    with pytest.raises(ValueError):
        pipe.set_option("contours", 2)
    pipe.close()
