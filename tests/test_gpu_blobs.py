"""Device Otsu and K4b (abub_blobs.hip) against the host and scipy, and the pipeline's "blobs" knob against the oracle
and the host route."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib, host, synth  # noqa: E402
from blobscenes import _assert_same_outputs, _check, _grouped, _launch, _slot_image  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- device Otsu --------------------------------------------------------------------------------------------------------

def _adversarial_hists(P, rs):
    eps = float(np.finfo(np.float32).eps)
    out = []
    for b in (0, 1, 3, 4, 128, 254, 255):  # all mass in one bin
        h = np.zeros(256, np.int64)
        h[b] = P
        out.append(h)
    for a, b in ((0, 255), (3, 200), (10, 11), (100, 156)):  # two equal spikes: ties in the between-class variance
        h = np.zeros(256, np.int64)
        h[a] = h[b] = P // 2
        h[0] += P - h.sum()
        out.append(h)
    h = np.zeros(256, np.int64)  # symmetric three spikes
    h[[20, 120, 220]] = P // 3
    h[120] += P - h.sum()
    out.append(h)
    for k in (-2, -1, 0, 1, 2):  # q1 / q2 right at the FLT_EPSILON edges
        for lo in (True, False):
            m = int(round(eps * P)) + k
            h = np.zeros(256, np.int64)
            if lo:
                h[5], h[200] = m, P - m
            else:
                h[5], h[200] = P - m, m
            out.append(h)
    for _ in range(20):  # sparse tails, like real post-trigger images
        h = np.zeros(256, np.int64)
        nz = rs.randint(1, 40)
        h[rs.randint(0, 256, nz)] += rs.randint(1, 50, nz)
        h[0] += P - h.sum()
        out.append(h)
    return out


@pytest.mark.parametrize("W,H", [(1280, 1024), (1680, 1050), (64, 48)])
def test_device_otsu_equals_host(W, H):
    from autobub3hs_amd import hip

    P = W * H
    rs = np.random.RandomState(W)
    hists, tz = [], []
    for h in _adversarial_hists(P, rs):
        for t in (0, 3, 254, 255, -1, 7):
            hists.append(h)
            tz.append(t)
    for _ in range(3000):
        k = rs.randint(1, 256)
        h = rs.multinomial(P, rs.dirichlet(np.ones(k) * rs.choice([0.05, 0.5, 5.0])))
        hh = np.zeros(256, np.int64)
        hh[np.sort(rs.choice(256, k, replace=False))] = h
        hists.append(hh)
        tz.append(int(rs.choice([0, 1, 3, 10, 50, 254, 255, rs.randint(0, 256)])))
    hists = np.array(hists, np.uint32)
    tz = np.array(tz, np.int32)
    got = hip.binarize_thr(torch.from_numpy(hists.view(np.int32)).to(DEV), torch.from_numpy(tz).to(DEV), W, H).cpu().numpy()
    ref = np.array([host.binarize_threshold(h, P, t) for h, t in zip(hists, tz)])
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, [(int(i), int(tz[i]), int(got[i]), int(ref[i])) for i in bad[:10]]


# ---- K4b -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1280, 96), (1280, 1024), (1680, 1050)])
def test_label_blobs_equals_scipy(W, H):
    rs = np.random.RandomState(H)
    kinds = ["small"] * 12 + ["empty"]
    imgs = [_slot_image(rs, W, H, k) for k in kinds]
    thr = rs.randint(0, 200, len(imgs))
    thr[0] = 0
    mb = rs.choice([-1, 0, 10], len(imgs))
    out, _ = _launch(imgs, thr, mb, W, H, rs)
    st = _check(imgs, thr, mb, out)
    assert st[0] == 0  # no slot above the LDS limit
    out2, _ = _launch(imgs, thr, mb, W, H, np.random.RandomState(H))  # another launch (other list order): byte-identical
    _assert_same_outputs(out, out2)


def test_label_blobs_large_and_small_slots_in_one_launch():
    W, H = 1280, 1024
    rs = np.random.RandomState(5)
    kinds = ["small"] * 40 + ["large", "empty", "small", "large"]
    imgs = [_slot_image(rs, W, H, k) for k in kinds]
    thr = np.array([rs.randint(0, 100) for _ in kinds])
    thr[40] = 0  # ~460k foreground pixels in one slot
    thr[43] = 150
    mb = np.array([[-1, 0, 10][k % 3] for k in range(len(kinds))])
    out, _ = _launch(imgs, thr, mb, W, H, rs)
    st = _check(imgs, thr, mb, out)
    assert (imgs[40] > 0).sum() >= 200_000
    assert st[0] == 2  # both dense slots took the global-memory path
    out2, _ = _launch(imgs, thr, mb, W, H, np.random.RandomState(5 + 1000))  # another list order: same result
    _assert_same_outputs(out, out2)


def test_label_blobs_whole_frame_slot():
    W, H = 1680, 1050
    rs = np.random.RandomState(8)
    v = rs.randint(1, 256, (H, W)).astype(np.uint8)  # every pixel a candidate: a list of W*H entries
    imgs = [v, _slot_image(rs, W, H, "small")]
    out, _ = _launch(imgs, np.array([0, 50]), np.array([10, 10]), W, H, rs, comp=True)
    _check(imgs, np.array([0, 50]), np.array([10, 10]), out)
    assert out["ncomp"][0] == 1 and out["kept_off"][1] == W * H


def test_label_blobs_overflow_convention():
    """kept_off / comp_off hold the true counts; nothing is written at or past cap"""
    W, H = 640, 480
    rs = np.random.RandomState(2)
    imgs = [_slot_image(rs, W, H, "small") for _ in range(6)]
    thr, mb = np.zeros(6, np.int64), np.full(6, -1)
    full, _ = _launch(imgs, thr, mb, W, H, rs)
    total = int(full["kept_off"][-1])
    ctotal = int(full["comp_off"][-1])
    assert total > 100
    offs, idx, val = _grouped(imgs, np.random.RandomState(3))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)  # noqa: E731
    cap, ccap, guard = total // 3, ctotal // 3, 4096
    kidx = torch.full((cap + guard,), -7, dtype=torch.int32, device=DEV)
    comp = torch.full((ccap + guard, 6), -7, dtype=torch.int32, device=DEV)
    ko, nc, nk, co, stats = (torch.empty((n,), dtype=torch.int32, device=DEV) for n in (7, 6, 6, 7, 4))
    L = _lib.lib()
    need = L.abub_label_blobs_scratch_bytes(6, W, H, len(idx), 1)
    scratch = torch.empty((need,), dtype=torch.uint8, device=DEV)
    d_offs, d_idx, d_val = t(offs, np.int32), t(idx, np.int32), t(val, np.uint8)
    d_thr, d_mb = t(thr, np.int32), t(mb, np.int32)
    _lib.check(L.abub_label_blobs_dev(d_offs.data_ptr(), d_idx.data_ptr(), d_val.data_ptr(), len(idx), 6, W, H,
                                      d_thr.data_ptr(), d_mb.data_ptr(), ko.data_ptr(), kidx.data_ptr(), cap, nc.data_ptr(),
                                      nk.data_ptr(), co.data_ptr(), comp.data_ptr(), ccap, stats.data_ptr(), scratch.data_ptr(),
                                      need, torch.cuda.current_stream().cuda_stream), "abub_label_blobs_dev")
    torch.cuda.synchronize()
    assert np.array_equal(ko.cpu().numpy(), full["kept_off"]) and np.array_equal(co.cpu().numpy(), full["comp_off"])
    k = kidx.cpu().numpy()
    assert np.array_equal(k[:cap], full["kept_idx"][:cap]) and (k[cap:] == -7).all()
    c = comp.cpu().numpy()
    assert np.array_equal(c[:ccap], full["comp"][:ccap]) and (c[ccap:] == -7).all()


# ---- the pipeline's "blobs" knob ------------------------------------------------------------------------------------------

def _oracle_event(oracle, fr, mu, sg, tss):
    a = oracle.Analyzer(fr, mu, sg, tss)
    out = a.any_cam_analysis()
    a.close()
    return out


def _boxes(bubbles):
    return [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in bubbles]


def _both_settings(pipe, run, S):
    """run with blobs = 0, then 1, on the same pipeline object: -> (results 0, results 1, blob_stats of the second)"""
    res = []
    for v in (0, 1):
        pipe.set_option("blobs", v)
        run()
        res.append([pipe.result(s) for s in range(S)])
    st = pipe.blob_stats()
    assert repr([r[:3] for r in res[0]]) == repr([r[:3] for r in res[1]])
    for r in res[1]:
        assert "Otsu" not in r[3], r[3]
    return res[0], res[1], st


def _stats_sane(st):
    assert 0 < st["kept"] <= st["foreground"] <= st["candidates"], st
    assert 0 < st["kept_components"] <= st["components"], st


@pytest.mark.parametrize("W,H", [(1280, 128), (322, 120)])  # fused lists / K4 pairs on stored images (non-fast-path width)
def test_pipeline_blobs_equals_oracle(oracle, W, H):
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
    _, res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _stats_sane(st)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c])
            assert (staged, state) == (ref[0], ref[1]), (e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])
    pipe.close()


@pytest.mark.parametrize("regime", ["default", "post_trigger_dense", "noisy"])
def test_pipeline_blobs_in_every_regime(oracle, regime):
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
    _, res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _stats_sane(st)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c])
            assert (staged, state) == (ref[0], ref[1]), (regime, e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])
    pipe.close()


def _small_run(oracle, E=4, C_=1, W=1280, H=96, F=41, seed=300):
    slab = np.zeros((E, C_, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C_):
            spec = synth.random_spec(W, H, F, seed + e, c, p_second=0.5, margin=25)
            slab[e, c] = synth.render_event(W, H, spec, seed + e, c)
    models = [oracle.welford(synth.training_pairs(W, H, 8, c, F)) for c in range(C_)]
    return slab, models


def test_pipeline_blobs_regrow_and_env_seed(oracle, monkeypatch):
    """ABUB_PIPE_PAIRCAP=64: the lists (the kept list too) grow and the batch is redone; ABUB_PIPE_BLOBS=1 seeds the knob"""
    from autobub3hs_amd import hip

    W, H, F, E = 1280, 96, 41, 4
    slab, models = _small_run(oracle, E=E)
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(models[0][0][None]).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(models[0][1][None]).to(DEV))
    st_ = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("ABUB_PIPE_PAIRCAP", "64")
    monkeypatch.setenv("ABUB_PIPE_BLOBS", "1")
    pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    monkeypatch.delenv("ABUB_PIPE_PAIRCAP")
    monkeypatch.delenv("ABUB_PIPE_BLOBS")
    pipe.run(d_slab, d_mu, d_s6, st_)
    assert pipe.timing()["pairs"] > 64
    st = pipe.blob_stats()
    _stats_sane(st)  # the environment switched it on
    grown = [pipe.result(s)[:3] for s in range(E)]
    pipe.close()
    ref_pipe = host.Pipeline(0, W, H, F, E, 1, [16], nthreads=2)
    ref_pipe.run(d_slab, d_mu, d_s6, st_)
    assert ref_pipe.blob_stats()["candidates"] == 0  # default: off
    assert repr(grown) == repr([ref_pipe.result(s)[:3] for s in range(E)])
    ref_pipe.close()
    ref = _oracle_event(oracle, slab[0, 0], models[0][0], models[0][1], 16)
    assert (grown[0][0], grown[0][1]) == (ref[0], ref[1])


def test_pipeline_blobs_streamed(oracle, monkeypatch):
    from autobub3hs_amd import hip

    W, H, F, E, C_ = 1280, 96, 41, 8, 2
    slab, models = _small_run(oracle, E=E, C_=C_, seed=800)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    h_slab = torch.from_numpy(slab).pin_memory()
    monkeypatch.setenv("ABUB_PIPE_GROUPS", "4")
    pipe = host.Pipeline(0, W, H, F, E, C_, [16, 16], nthreads=4)
    monkeypatch.delenv("ABUB_PIPE_GROUPS")
    _, res, st = _both_settings(pipe, lambda: pipe.run_host(h_slab, d_mu, d_s6), E * C_)
    _stats_sane(st)
    for s in (0, 5, 11):
        ref = _oracle_event(oracle, slab[s // C_, s % C_], models[s % C_][0], models[s % C_][1], 16)
        assert (res[s][0], res[s][1]) == (ref[0], ref[1])
    pipe.close()


def test_pipeline_blobs_on_the_bellows_fixture(tmp_path):
    """the committed full-size 40l-19 scenes (bellows veto in the batch: residual images stay on the host route)"""
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
    pipe.set_option("blobs", 1)
    pipe.run(d_slab, d_mu, s6, torch.cuda.current_stream().cuda_stream)
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = pipe.result(e * C_ + c)
            row = (staged, {k: state[k] for k in ("trig", "status", "ok", "loc_thres")},
                   [[[d[k] for k in "xywh"] for d in b["desc"]] for b in bubbles])
            assert row == want[(e, c)], (e, c, err)
    assert pipe.bellows_stats()["vetoed"] >= 1 and pipe.timing()["dropin_stacks"] == 0
    _stats_sane(pipe.blob_stats())
    with pytest.raises(ValueError):
        pipe.set_option("blobs", 2)
    pipe.close()
