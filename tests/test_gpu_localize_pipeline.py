"""The pipeline's "localize" knob (K7, abub_localize.hip): the same Pipeline object run with the knob off and on gives
identical per-stack results, equal to the oracle's; in the synthetic regimes every stack is localised on the device; masks
come from files; the lists regrow; the knob works with "trigger"; the 40l-19 bellows fixture keeps its vetoed and over-limit
stacks on the host route; a RunBatched run writes the same text."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import locscenes as ls  # noqa: E402
from autobub3hs_amd import hip, host, synth  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = 41


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _oracle_event(oracle, fr, mu, sg, tss, **kw):
    a = oracle.Analyzer(fr, mu, sg, tss, **kw)
    out = a.any_cam_analysis()
    a.close()
    return out


def _boxes(bubbles):
    return [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in bubbles]


def _both_settings(pipe, run, S, all_on_device=True):
    """run with localize = 0, then 1, on the same pipeline object: per-stack results are identical -> (results of the
    second run, its localize_stats)"""
    res = []
    for v in (0, 1):
        pipe.set_option("localize", v)
        run()
        res.append([pipe.result(s) for s in range(S)])
        st = pipe.localize_stats()
        if v == 0:
            assert all(st[k] == 0 for k in st if k != "list_bytes"), st
    assert repr(res[0]) == repr(res[1])
    for r in res[1]:
        assert "Otsu" not in r[3] and "contoursKept" not in r[3] and "localis" not in r[3], r[3]
    assert st["device"] > 0 and st["k7_ms"] > 0 and st["bubbles"] > 0 and st["descriptors"] >= st["bubbles"], st
    if all_on_device:
        assert st["host_route"] == 0, st
    return res[1], st


def _against_oracle(oracle, res, slab, models, tss, masks=None, what=""):
    E, C_ = slab.shape[:2]
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            kw = {} if masks is None else {"fid_mask": masks[c][0], "bel_mask": masks[c][1]}
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c], **kw)
            assert (staged, state) == (ref[0], ref[1]), (what, e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])
            for b, r in zip(bubbles, ref[2]):  # centroids and radii: the existing 1e-4
                for d, q in zip(b["desc"], r["desc"]):
                    for k in ("area", "radius", "m00", "m10", "m01", "cx", "cy"):
                        assert (np.isnan(d[k]) and np.isnan(q[k])) or abs(d[k] - q[k]) <= 1e-4 * max(1.0, abs(q[k])), (k, d[k], q[k])


def _device(slab, models):
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    return d_slab, d_mu, d_s6


@pytest.mark.parametrize("W,H", [(1280, 128), (322, 120)])
def test_pipeline_localize_equals_oracle(oracle, W, H):
    E, C_ = 7, 2
    slab = np.zeros((E, C_, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C_):
            spec = synth.random_spec(W, H, F, 500 + e, c, p_second=0.4, p_none=0.2, p_flicker=0.3, margin=25)
            slab[e, c] = synth.render_event(W, H, spec, 500 + e, c)
    quiet = synth.render_event(W, H, synth.EventSpec(F), 900, 0)
    quiet[12:] = np.clip(quiet[12:].astype(int) + 1, 0, 255)  # a persistent step without a blob: retried to the end
    slab[E - 1, 0] = quiet
    tr0, tr1 = synth.training_pairs(W, H, 10, 0, F), synth.training_pairs(W, H, 2, 1, F)
    models = [oracle.welford(tr0), oracle.welford(tr1)]
    tss = [len(tr0), len(tr1)]
    d_slab, d_mu, d_s6 = _device(slab, models)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss)
    assert pipe.contour_stats()["traced"] > 0  # the knob implies the contour tracing
    pipe.close()


@pytest.mark.parametrize("regime", ["default", "post_trigger_dense", "noisy"])
def test_pipeline_localize_in_every_regime(oracle, regime):
    W, H, E, C_ = 1280, 96, 6, 2
    slab, models, tss = ls.regime_run(oracle, regime)
    d_slab, d_mu, d_s6 = _device(slab, models)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss, what=regime)
    pipe.close()


def test_pipeline_localize_masks_from_files(oracle, tmp_path):
    """cam<N>_mask.bmp for both cameras, cam1_bellows_mask.bmp for the odd one only: camera 0 has no bellows mask"""
    W, H, E, C_ = 1280, 96, 6, 2
    maskdir = str(tmp_path / "masks")
    accept_for = synth.write_masks(maskdir, W, H, C_)
    assert not os.path.exists(os.path.join(maskdir, "cam0_bellows_mask.bmp"))
    masks = [synth.camera_masks(W, H, c) for c in range(C_)]
    slab, models, tss = ls.regime_run(oracle, "default", seed=780, accept_for=accept_for)
    # two bubbles the masks reject: outside the fiducial ellipse (camera 0), inside the bellows strip (camera 1)
    slab[0, 0] = synth.render_event(W, H, synth.EventSpec(F, 14, [(30, 10, 40), (600, 48, -40)]), 780, 0)
    slab[1, 1] = synth.render_event(W, H, synth.EventSpec(F, 15, [(640, 84, 40), (400, 40, -40)]), 781, 1)
    d_slab, d_mu, d_s6 = _device(slab, models)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4, maskdir=maskdir)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_, all_on_device=False)
    assert st["host_limits"] == 0 and st["host_slot"] == 0 and st["host_other"] == 0, st
    _against_oracle(oracle, res, slab, models, tss, masks=masks, what="masks")
    pipe.close()


def test_pipeline_localize_regrow_and_env_seed(oracle, monkeypatch):
    """ABUB_PIPE_PAIRCAP=64: the candidate list and the lists behind it grow and the batch is redone; ABUB_PIPE_LOCALIZE=1
    seeds the knob"""
    W, H, E = 1280, 96, 4
    slab = np.zeros((E, 1, F, H, W), np.uint8)
    for e in range(E):
        spec = synth.random_spec(W, H, F, 300 + e, 0, p_second=0.5, margin=25)
        slab[e, 0] = synth.render_event(W, H, spec, 300 + e, 0)
    mu, sg = oracle.welford(synth.training_pairs(W, H, 8, 0, F))
    d_slab, d_mu, d_s6 = _device(slab, [(mu, sg)])
    st_ = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("ABUB_PIPE_PAIRCAP", "64")
    monkeypatch.setenv("ABUB_PIPE_LOCALIZE", "1")
    pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    monkeypatch.delenv("ABUB_PIPE_PAIRCAP")
    monkeypatch.delenv("ABUB_PIPE_LOCALIZE")
    pipe.run(d_slab, d_mu, d_s6, st_)
    assert pipe.timing()["pairs"] > 64
    st = pipe.localize_stats()  # the environment switched it on
    assert st["device"] > 0 and st["host_route"] == 0, st
    assert pipe.contour_stats()["vertices"] > 64 // 4 + 64
    grown = [pipe.result(s) for s in range(E)]
    pipe.close()
    ref_pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    ref_pipe.run(d_slab, d_mu, d_s6, st_)
    assert ref_pipe.localize_stats()["device"] == 0 and ref_pipe.contour_stats()["traced"] == 0  # default: off
    assert repr(grown) == repr([ref_pipe.result(s) for s in range(E)])
    ref_pipe.close()
    ref = _oracle_event(oracle, slab[0, 0], mu, sg, 16)
    assert (grown[0][0], grown[0][1]) == (ref[0], ref[1])


@pytest.mark.parametrize("paircap", [None, "64"])
def test_pipeline_localize_lists_regrow(oracle, monkeypatch, paircap):
    """ABUB_PIPE_LOCCAP=1: the record, box and track lists start with one entry each.  The first pass overflows the record
    list, so K7b declines the stacks behind it and its totals are lower bounds: the records grow alone and the batch is
    redone; the boxes and tracks grow from the totals of that second pass, and a third pass fits -- two regrows per batch
    that localises, no stack on the host route, and the results of a pipeline with roomy lists.  With ABUB_PIPE_PAIRCAP=64
    the candidate and contour lists grow in front of them, in the same batch"""
    W, H, E, C_ = 1280, 96, 6, 2
    slab, models, tss = ls.regime_run(oracle, "post_trigger_dense")  # (the seeds the CPU test holds against the limits)
    d_slab, d_mu, d_s6 = _device(slab, models)
    st_ = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("ABUB_PIPE_LOCCAP", "1")
    if paircap:
        monkeypatch.setenv("ABUB_PIPE_PAIRCAP", paircap)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    monkeypatch.delenv("ABUB_PIPE_LOCCAP")
    if paircap:
        monkeypatch.delenv("ABUB_PIPE_PAIRCAP")
    pipe.set_option("localize", 1)
    pipe.run(d_slab, d_mu, d_s6, st_)
    st = pipe.localize_stats()
    print(st, pipe.contour_stats())
    assert st["regrows"] >= 2, st  # (a later round of the run finds the lists large enough, or grows them again)
    assert st["device"] > 0 and st["host_route"] == 0 and st["bubbles"] > 1 and st["descriptors"] > st["bubbles"], st
    small = [pipe.result(s) for s in range(E * C_)]
    pipe.run(d_slab, d_mu, d_s6, st_)  # the lists are large enough now
    assert pipe.localize_stats()["regrows"] == 0
    assert repr([pipe.result(s) for s in range(E * C_)]) == repr(small)
    pipe.close()
    roomy = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    for v in (1, 0):
        roomy.set_option("localize", v)
        roomy.run(d_slab, d_mu, d_s6, st_)
        assert roomy.localize_stats()["regrows"] == 0
        assert repr([roomy.result(s) for s in range(E * C_)]) == repr(small), v
    roomy.close()
    _against_oracle(oracle, small, slab, models, tss, what="lists regrow")


@pytest.mark.parametrize("paircap,loccap", [(None, None), ("64", "1")])
@pytest.mark.parametrize("groups", [None, "2"])
def test_pipeline_knob_ladder_on_one_object(oracle, monkeypatch, groups, paircap, loccap):
    """One Pipeline object through localize, contours, blobs, nothing, localize + trigger, nothing: the first batch makes
    every stage's buffers at once (with the small capacities, while every list is growing) and the later settings reuse
    them.  Every run gives the same per-stack results, the oracle's; the stats of a stage that did not run are zero."""
    W, H, E, C_ = 1280, 96, 6, 2
    slab, models, tss = ls.regime_run(oracle, "post_trigger_dense")
    d_slab, d_mu, d_s6 = _device(slab, models)
    st_ = torch.cuda.current_stream().cuda_stream
    env = {"ABUB_PIPE_GROUPS": groups, "ABUB_PIPE_PAIRCAP": paircap, "ABUB_PIPE_LOCCAP": loccap}
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    for k, v in env.items():
        if v:
            monkeypatch.delenv(k)
    ladder = [{"localize": 1}, {"contours": 1}, {"blobs": 1}, {}, {"localize": 1, "trigger": 1}, {}]
    res, regrows = [], []
    for on in ladder:
        for name in ("blobs", "contours", "trigger", "localize"):
            pipe.set_option(name, on.get(name, 0))
        pipe.run(d_slab, d_mu, d_s6, st_)
        res.append([pipe.result(s) for s in range(E * C_)])
        lst = pipe.localize_stats()
        regrows.append(lst["regrows"])
        # a stage runs when its knob, or one that implies it, is on: localize -> contours -> blobs
        ran = {"localize": "localize" in on, "trigger": "trigger" in on}
        ran["contours"] = ran["localize"] or "contours" in on
        ran["blobs"] = ran["contours"] or "blobs" in on
        stats = {"localize": {k: v for k, v in lst.items() if k != "list_bytes"}, "trigger": pipe.trigger_stats(),
                 "contours": pipe.contour_stats(), "blobs": pipe.blob_stats()}
        for name, st in stats.items():
            if not ran[name]:
                assert all(v == 0 for v in st.values()), (on, name, st)
        if ran["localize"]:
            assert lst["device"] > 0 and lst["host_route"] == 0, (on, lst)
    pipe.close()
    for r in res[1:]:
        assert repr(r) == repr(res[0])
    if loccap:
        assert regrows[0] >= 2 and regrows[4] == 0, regrows
    _against_oracle(oracle, res[0], slab, models, tss, what="knob ladder")


def test_pipeline_localize_with_trigger(oracle):
    W, H, E, C_ = 1280, 96, 6, 2
    slab, models, tss = ls.regime_run(oracle, "default", seed=740)
    d_slab, d_mu, d_s6 = _device(slab, models)
    st_ = torch.cuda.current_stream().cuda_stream
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    pipe.set_option("trigger", 1)
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    assert pipe.trigger_stats()["device"] == E * C_
    _against_oracle(oracle, res, slab, models, tss, what="trigger")
    with pytest.raises(ValueError):
        pipe.set_option("localize", 2)
    pipe.close()


def test_pipeline_localize_on_the_bellows_fixture(tmp_path):
    """the committed full-size 40l-19 scenes: the vetoed stacks (every genesis contour in the bellows mask) and the ones
    whose slots the tracer declines take the host route, which the stats show; the results are the expected ones"""
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
    pipe.set_option("localize", 1)
    pipe.run(d_slab, d_mu, s6, torch.cuda.current_stream().cuda_stream)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = pipe.result(e * C_ + c)
            row = (staged, {k: state[k] for k in ("trig", "status", "ok", "loc_thres")},
                   [[[d[k] for k in "xywh"] for d in b["desc"]] for b in bubbles])
            assert row == want[(e, c)], (e, c, err)
    st, cst, vst = pipe.localize_stats(), pipe.contour_stats(), pipe.bellows_stats()
    print(st, cst, vst)
    assert vst["vetoed"] >= 1 and pipe.timing()["dropin_stacks"] == 0
    assert st["host_other"] == 0 and st["host_route"] > 0, st
    # a vetoed stack either reached K7b, which found every genesis contour in the bellows mask, or had a slot declined
    assert st["host_bellows"] + st["host_slot"] + st["host_limits"] >= vst["vetoed"], (st, vst)
    assert (st["host_slot"] > 0) == (cst["host_route"] > 0), (st, cst)
    pipe.close()


def test_run_batched_text_is_the_same_with_the_knob(tmp_path, monkeypatch):
    """RunBatched from a directory with a short stack (20 frames) and undecodable frames: the output text with
    ABUB_PIPE_LOCALIZE=1 is the text with the knob off, byte for byte"""
    from PIL import Image

    W, H, nev, ncams = 320, 128, 5, 2
    rd = os.path.join(str(tmp_path), "data", "r")
    for e in range(nev):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d)
        for c in range(ncams):
            spec = synth.random_spec(W, H, F, 900 + e, c, p_none=0.2, margin=20)
            st = synth.render_event(W, H, spec, 900 + e, c)
            if (e, c) == (4, 0):
                st = st[:20]
            for k in range(len(st)):
                path = os.path.join(d, f"cam{c}_image{30 + k}.png")
                Image.fromarray(st[k]).save(path)
                if (e, c, k) in ((3, 1, 7), (2, 0, 33)):
                    raw = open(path, "rb").read()
                    open(path, "wb").write(raw[: len(raw) // 2])

    def go(tag, knob):
        if knob:
            monkeypatch.setenv("ABUB_PIPE_LOCALIZE", "1")
        outdir = os.path.join(str(tmp_path), tag)
        os.makedirs(outdir)
        run = host.Run("raw", rd + "/", "Images")
        before = host.localize_totals()
        try:
            for c in range(ncams):
                assert run.train(c, shape=(H, W))[0] == 0
            run.run_batched(ncams, outdir + "/", "r", 30, nthreads=4, decode_threads=4, batch_mb=64)
        finally:
            run.close()
            if knob:
                monkeypatch.delenv("ABUB_PIPE_LOCALIZE")
        after = host.localize_totals()
        return open(os.path.join(outdir, "abub3hs_r.txt")).read(), (after[0] - before[0], after[1] - before[1])

    ref, n0 = go("off", False)
    txt, n1 = go("on", True)
    assert n0 == (0, 0)
    assert n1[0] >= 4, n1
    assert txt == ref
    assert len(ref.splitlines()) >= nev * ncams
