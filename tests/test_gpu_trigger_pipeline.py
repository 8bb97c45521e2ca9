"""The pipeline's "trigger" knob (K6, abub_trigger.hip): the same Pipeline object run with the knob off and on gives identical
per-stack results, equal to the oracle's AnyCamAnalysis; every stack is searched on the device; lazy blocks and deferred
pieces are asked for through NEED_FRAMES / NEED_FINAL answers."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import hip, host, synth  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _oracle_event(oracle, fr, mu, sg, tss):
    a = oracle.Analyzer(fr, mu, sg, tss)
    out = a.any_cam_analysis()
    a.close()
    return out


def _boxes(bubbles):
    return [[tuple(d[k] for k in "xywh") for d in b["desc"]] for b in bubbles]


def _both_settings(pipe, run, S):
    """run with trigger = 0, then 1, on the same pipeline object: per-stack results are identical, every stack of the
    second run was searched on the device and asked for the same blocks and the same deferred pieces as the host search
    -> (results of the second run, its trigger_stats)"""
    res, tm = [], []
    for v in (0, 1):
        pipe.set_option("trigger", v)
        run()
        res.append([pipe.result(s) for s in range(S)])
        tm.append(pipe.timing())
        st = pipe.trigger_stats()
        if v == 0:
            assert (st["device"], st["host_route"], st["launches"], st["need_frames"], st["need_final"]) == (0, 0, 0, 0, 0), st
    assert repr(res[0]) == repr(res[1])
    assert st["host_route"] == 0 and st["device"] == S and st["launches"] >= 1, st
    assert st["k6_ms"] > 0
    print(st, tm[1])
    for k in ("trigger_jobs", "jobs_completed_on_demand", "dropin_stacks", "rounds"):
        assert tm[0][k] == tm[1][k], (k, tm)
    assert (tm[1]["jobs_completed_on_demand"] > 0) == (st["need_final"] > 0), (st, tm[1])
    return res[1], st


def _against_oracle(oracle, res, slab, models, tss, what=""):
    E, C_ = slab.shape[:2]
    for e in range(E):
        for c in range(C_):
            staged, state, bubbles, err = res[e * C_ + c]
            ref = _oracle_event(oracle, slab[e, c], models[c][0], models[c][1], tss[c])
            assert (staged, state) == (ref[0], ref[1]), (what, e, c, staged, state, ref[0], ref[1], err)
            assert _boxes(bubbles) == _boxes(ref[2])


def _device(slab, models):
    d_slab = torch.from_numpy(slab).to(DEV)
    d_mu = torch.from_numpy(np.stack([m[0] for m in models])).to(DEV)
    d_s6 = hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV))
    return d_slab, d_mu, d_s6


@pytest.mark.parametrize("W,H", [(1280, 128), (322, 120)])  # deferred pieces / the generic width (no deferral)
def test_pipeline_trigger_equals_oracle(oracle, W, H):
    F, E, C_ = 41, 7, 2
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
    assert st["need_frames"] > 0, st  # the quiet stack's search runs through every lazy block
    pipe.close()


def _regime_run(oracle, regime, E=6, C_=2, seed=700):
    W, H, F = 1280, 96, 41
    slab = np.zeros((E, C_, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C_):
            spec = synth.random_spec(W, H, F, seed + e, c, p_second=0.3, p_none=0.15, p_flicker=0.3, margin=25, regime=regime)
            slab[e, c] = synth.render_event(W, H, spec, seed + e, c)
    models, tss = [], []
    for c in range(C_):
        tr = np.concatenate([slab[e, c, :2] for e in range(E)])
        models.append(oracle.welford(tr))
        tss.append(len(tr))
    return slab, models, tss


@pytest.mark.parametrize("regime", ["default", "post_trigger_dense", "noisy"])
def test_pipeline_trigger_in_every_regime(oracle, regime):
    W, H, F, E, C_ = 1280, 96, 41, 6, 2
    slab, models, tss = _regime_run(oracle, regime)
    d_slab, d_mu, d_s6 = _device(slab, models)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss, regime)
    # (dense frames behind the bubble are deferred pieces: a search that goes on behind its trigger asks for them with
    # NEED_FINAL; _both_settings holds the count against the pieces the host search completed)
    pipe.close()


@pytest.mark.parametrize("env", [{"ABUB_PIPE_BLOCK0": "12", "ABUB_PIPE_BLOCK": "4"}, {"ABUB_PIPE_DEFER": "0"}])
def test_pipeline_trigger_small_blocks_and_no_deferral(oracle, monkeypatch, env):
    W, H, F, E, C_ = 1280, 96, 41, 6, 2
    slab, models, tss = _regime_run(oracle, "post_trigger_dense", seed=720)
    d_slab, d_mu, d_s6 = _device(slab, models)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    for k in env:
        monkeypatch.delenv(k)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss, str(env))
    if "ABUB_PIPE_BLOCK" in env:
        assert st["need_frames"] > 0 and st["launches"] >= 3, st  # a bubble behind frame 16 takes two more blocks
    else:
        assert st["need_final"] == 0, st  # nothing is deferred: every histogram is final when it arrives
    pipe.close()


@pytest.mark.parametrize("ordered", ["1", "0"])
def test_pipeline_trigger_ordered_and_unordered_groups(oracle, monkeypatch, ordered):
    """three groups on small blocks: with ABUB_PIPE_ORDERED=0 a group's later blocks, searches and localisation kernels go
    to the group's own stream, not to the one trigger-search stream"""
    W, H, F, E, C_ = 1280, 96, 41, 6, 2
    slab, models, tss = _regime_run(oracle, "post_trigger_dense", seed=720)
    d_slab, d_mu, d_s6 = _device(slab, models)
    env = {"ABUB_PIPE_ORDERED": ordered, "ABUB_PIPE_GROUPS": "3", "ABUB_PIPE_BLOCK0": "12", "ABUB_PIPE_BLOCK": "4"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    for k in env:
        monkeypatch.delenv(k)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss, str(env))
    assert st["need_frames"] > 0, st
    pipe.close()


def test_pipeline_trigger_env_seed_and_contours(oracle, monkeypatch):
    """ABUB_PIPE_TRIGGER=1 seeds the knob; trigger = 1 together with contours = 1"""
    W, H, F, E, C_ = 1280, 96, 41, 6, 2
    slab, models, tss = _regime_run(oracle, "default", seed=740)
    d_slab, d_mu, d_s6 = _device(slab, models)
    st_ = torch.cuda.current_stream().cuda_stream
    ref_pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    ref_pipe.run(d_slab, d_mu, d_s6, st_)
    assert ref_pipe.trigger_stats()["device"] == 0  # default: off
    ref = [ref_pipe.result(s) for s in range(E * C_)]
    ref_pipe.close()
    monkeypatch.setenv("ABUB_PIPE_TRIGGER", "1")
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    monkeypatch.delenv("ABUB_PIPE_TRIGGER")
    pipe.run(d_slab, d_mu, d_s6, st_)
    st = pipe.trigger_stats()  # the environment switched it on
    assert st["device"] == E * C_ and st["host_route"] == 0, st
    assert repr([pipe.result(s) for s in range(E * C_)]) == repr(ref)
    pipe.set_option("contours", 1)
    pipe.run(d_slab, d_mu, d_s6, st_)
    st, cst = pipe.trigger_stats(), pipe.contour_stats()
    assert st["device"] == E * C_ and st["host_route"] == 0 and cst["traced"] > 0, (st, cst)
    res = [pipe.result(s) for s in range(E * C_)]
    assert repr(res) == repr(ref)
    _against_oracle(oracle, res, slab, models, tss)
    with pytest.raises(ValueError):
        pipe.set_option("trigger", 2)
    pipe.close()


def test_pipeline_trigger_streamed(oracle, monkeypatch):
    W, H, F, E, C_ = 1280, 96, 41, 8, 2
    slab, models, tss = _regime_run(oracle, "default", E=E, seed=760)
    _, d_mu, d_s6 = _device(slab[:1], models)
    h_slab = torch.from_numpy(slab).pin_memory()
    monkeypatch.setenv("ABUB_PIPE_GROUPS", "4")
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    monkeypatch.delenv("ABUB_PIPE_GROUPS")
    res, st = _both_settings(pipe, lambda: pipe.run_host(h_slab, d_mu, d_s6), E * C_)
    assert st["launches"] >= 4, st  # one per group behind its block 0
    _against_oracle(oracle, res, slab, models, tss, "streamed")
    pipe.close()


def test_run_batched_text_is_the_same_with_the_knob(tmp_path, monkeypatch):
    """RunBatched from a directory with a short stack (20 frames) and an undecodable frame (first_bad from the parser's
    decode flags): the output text with ABUB_PIPE_TRIGGER=1 is the text with the knob off, and every stack was searched
    on the device"""
    from PIL import Image

    W, H, F, nev, ncams = 320, 128, 41, 5, 2
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
                if (e, c, k) in ((3, 1, 7), (2, 0, 33)):  # before any bubble: -9; behind one: never reached, or a look-ahead
                    raw = open(path, "rb").read()
                    open(path, "wb").write(raw[: len(raw) // 2])

    def go(tag, knob):
        if knob:
            monkeypatch.setenv("ABUB_PIPE_TRIGGER", "1")
        outdir = os.path.join(str(tmp_path), tag)
        os.makedirs(outdir)
        run = host.Run("raw", rd + "/", "Images")
        before = host.trigger_totals()
        try:
            for c in range(ncams):
                assert run.train(c, shape=(H, W))[0] == 0
            run.run_batched(ncams, outdir + "/", "r", 30, nthreads=4, decode_threads=4, batch_mb=64)
        finally:
            run.close()
            if knob:
                monkeypatch.delenv("ABUB_PIPE_TRIGGER")
        after = host.trigger_totals()
        return open(os.path.join(outdir, "abub3hs_r.txt")).read(), (after[0] - before[0], after[1] - before[1])

    ref, n0 = go("off", False)
    txt, n1 = go("on", True)
    assert n0 == (0, 0)
    assert n1[0] >= nev * ncams and n1[1] == 0, n1
    assert txt == ref
    assert "  -9  " in ref and len(ref.splitlines()) >= nev * ncams


def _triggers_where_built(oracle, slab, models, tss, specs):
    """the oracle alone, before any device result is looked at: every designed bubble triggers at its t0"""
    E, C_ = slab.shape[:2]
    for e in range(E):
        for c in range(C_):
            a = oracle.Analyzer(slab[e, c], models[c][0], models[c][1], tss[c])
            st = a.find_trigger(1)
            a.close()
            t0 = specs[e * C_ + c].t0
            assert (st["status"], st["trig"] if t0 is not None else None) == ((0, t0) if t0 is not None else (-3, None)), (e, c, t0, st)


def test_pipeline_trigger_across_a_tile_seam(oracle, monkeypatch):
    """70 frames: K6 walks a stack in tiles of 64 frames from frame 1, and the bubbles start at 62 .. 65, around its first
    seam (64 | 65); block 0 ends at frame 60 and the lazy blocks have 4 frames, so the searches stop and go on around it"""
    W, H, F, E, C_ = 1280, 96, 70, 4, 2
    B = [(600, 48, 40)]
    specs = [synth.EventSpec(F, 62, B), synth.EventSpec(F, 63, B), synth.EventSpec(F, 64, B), synth.EventSpec(F, 64, [(200, 30, 40)]),
             synth.EventSpec(F, 65, B), synth.EventSpec(F, flicker=63, flicker_adu=12), synth.EventSpec(F, 63, [(900, 50, -40)]),
             synth.EventSpec(F)]
    slab = np.stack([synth.render_event(W, H, sp, 300 + k // C_, k % C_) for k, sp in enumerate(specs)]).reshape(E, C_, F, H, W)
    tr0, tr1 = synth.training_pairs(W, H, 10, 0, F), synth.training_pairs(W, H, 2, 1, F)
    models = [oracle.welford(tr0), oracle.welford(tr1)]
    tss = [len(tr0), len(tr1)]
    _triggers_where_built(oracle, slab, models, tss, specs)
    d_slab, d_mu, d_s6 = _device(slab, models)
    env = {"ABUB_PIPE_BLOCK0": "60", "ABUB_PIPE_BLOCK": "4"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    for k in env:
        monkeypatch.delenv(k)
    st_ = torch.cuda.current_stream().cuda_stream
    res, st = _both_settings(pipe, lambda: pipe.run(d_slab, d_mu, d_s6, st_), E * C_)
    _against_oracle(oracle, res, slab, models, tss, "seam")
    assert st["need_frames"] > 0, st
    pipe.close()


@pytest.mark.parametrize("over", [0, 1])
def test_pipeline_trigger_at_and_above_the_frame_limit(oracle, over):
    """a stack of exactly abub_trigger_search_limits() frames is searched on the device (its last tile is partial), one
    frame more keeps the host search; a bubble in the last tile, both against the oracle"""
    F0, _ = hip.trigger_search_limits()
    W, H, F, E, C_ = 320, 64, F0 + over, 1, 2
    specs = [synth.EventSpec(F, 450, [(160, 32, 40)]), synth.EventSpec(F, 450, [(100, 30, 40)])]
    slab = np.stack([synth.render_event(W, H, sp, 300, c) for c, sp in enumerate(specs)]).reshape(E, C_, F, H, W)
    tr0, tr1 = synth.training_pairs(W, H, 10, 0, F), synth.training_pairs(W, H, 2, 1, F)
    models = [oracle.welford(tr0), oracle.welford(tr1)]
    tss = [len(tr0), len(tr1)]
    _triggers_where_built(oracle, slab, models, tss, specs)
    d_slab, d_mu, d_s6 = _device(slab, models)
    pipe = host.Pipeline(0, W, H, F, E, C_, tss, nthreads=4)
    st_ = torch.cuda.current_stream().cuda_stream
    res = []
    for v in (0, 1):
        pipe.set_option("trigger", v)
        pipe.run(d_slab, d_mu, d_s6, st_)
        res.append([pipe.result(s) for s in range(E * C_)])
    st = pipe.trigger_stats()
    assert (st["device"], st["host_route"]) == ((0, 2) if over else (2, 0)), st
    assert repr(res[0]) == repr(res[1])
    _against_oracle(oracle, res[1], slab, models, tss, "limit + %d" % over)
    pipe.close()
