"""Scene, stack-length and value edges on the GPU, against the CPU oracle (and numpy for single kernels).

1. A table of hand-built stacks (edgescenes.edge_scenes: bubbles on every border and corner, a disc crossing the edge, a
   component taller than the frame, one above K4b's LDS limit, whole-frame +-60 ADU steps, saturated and dead pixels in
   the frames and in mu, sigma = 0, 6 sigma clipped at 255, a constant camera) through four routes: Pipeline.run with
   the "blobs" knob 0 and 1, Pipeline.run_host and the drop-in Run.analyze, at a fast-path and a generic width.
2. Stack lengths around every F-dependent branch of the batched pipeline, with the trigger at the first evaluable frame,
   on and around the lazy frame-block boundaries and at the end of the stack, with lazy blocks off, on and one frame
   long.
3. K3 on saturated inputs under every K3 knob, the device Otsu on degenerate histograms, K4 / K4b on a mask that is all
   foreground and on a one-pixel ring around the border."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import edgescenes  # noqa: E402
from autobub3hs_amd import _lib, hip, host, synth  # noqa: E402
from test_gpu_events import compare, oracle_event  # noqa: E402
from test_gpu_knobs import K3_MATRIX, _defaults  # noqa: E402,F401  (autouse: default K2 / K3 options after every test)

DEV = "cuda:0"
SENT = 0x5A5A5A5A  # canary word


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _st():
    return torch.cuda.current_stream().cuda_stream


def assert_same(res, ref, key):
    """test_gpu_events.compare (staged, state, boxes exact; area, radius, moments, centroids within 1e-4; dz, dzdt, drdt).
    Pipeline.result() does not report the per-frame dz of a bubble: for its results dz is left out on both sides."""
    if res[2] and "dz" not in res[2][0]:
        res = (res[0], res[1], [dict(b, dz=[]) for b in res[2]], res[3])
        ref = (ref[0], ref[1], [dict(r, dz=[]) for r in ref[2]])
    try:
        compare(res, ref)
    except AssertionError as e:
        raise AssertionError(f"{key}: {e}") from e


# ---- 1. scene edges, end to end --------------------------------------------------------------------------------------

_TABLES = {}


def edge_table(oracle, W, H):
    """-> (names, scenes, oracle results), built once per shape"""
    if (W, H) not in _TABLES:
        sc = edgescenes.edge_scenes(W, H, welford=oracle.welford)
        names = list(sc)
        refs = [oracle_event(oracle, *sc[n]) for n in names]
        _TABLES[(W, H)] = (names, sc, refs)
    return _TABLES[(W, H)]


def _device_model(sc, names):
    mu = torch.from_numpy(np.stack([sc[n][1] for n in names])).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(np.stack([sc[n][2] for n in names])).to(DEV))
    return mu, s6


def _pipeline(monkeypatch, W, H, F, C, tss, groups=None):
    """a pipeline whose candidate lists start at 64 K entries (ABUB_PIPE_PAIRCAP)"""
    monkeypatch.setenv("ABUB_PIPE_PAIRCAP", str(1 << 16))
    if groups:
        monkeypatch.setenv("ABUB_PIPE_GROUPS", str(groups))
    pipe = host.Pipeline(0, W, H, F, 1, C, tss, nthreads=4)
    monkeypatch.delenv("ABUB_PIPE_PAIRCAP")
    monkeypatch.delenv("ABUB_PIPE_GROUPS", raising=False)
    return pipe


@pytest.mark.parametrize("route", ["blobs0", "blobs1", "run_host", "dropin"])
@pytest.mark.parametrize("W,H", [(1280, 96), (322, 120)])  # fused lists / stored images and K4 (generic width)
def test_scene_edges_equal_oracle(oracle, monkeypatch, W, H, route):
    """Every scene is one camera of a one-event run (each camera with its own model).  The three pipeline routes start
    with candidate lists of 64 K entries: the step scenes make nearly every pixel of every tracking image a candidate, so
    the lists must grow and the batch be redone."""
    names, sc, refs = edge_table(oracle, W, H)
    C = len(names)
    F = sc[names[0]][0].shape[0]
    tss = [sc[n][3] for n in names]
    # the table must reach the localiser and the tracker, not only the trigger search
    assert sum(r[0] == 0 and len(r[2]) > 0 for r in refs) >= 12
    assert refs[names.index("constant_camera")][0] == -3
    if route == "dropin":
        run = host.Run()
        for c, n in enumerate(names):
            run.add_event(1, c, sc[n][0])
            run.set_model(c, sc[n][1], sc[n][2], sc[n][3])
        for c, n in enumerate(names):
            assert_same(run.analyze(1, c), refs[c], (W, H, route, n))
        run.close()
        return
    slab = np.ascontiguousarray(np.stack([sc[n][0] for n in names])[None])  # [E=1][C][F][H][W]
    d_mu, d_s6 = _device_model(sc, names)
    pipe = _pipeline(monkeypatch, W, H, F, C, tss, groups=3 if route == "run_host" else None)  # streamed: three groups
    if route == "run_host":
        pipe.run_host(torch.from_numpy(slab).pin_memory(), d_mu, d_s6)
    else:
        pipe.set_option("blobs", 1 if route == "blobs1" else 0)
        pipe.run(torch.from_numpy(slab).to(DEV), d_mu, d_s6, _st())
    for c, n in enumerate(names):
        assert_same(pipe.result(c), refs[c], (W, H, route, n))
    assert pipe.timing()["dropin_stacks"] == 0
    if route == "blobs1":
        st = pipe.blob_stats()
        assert st["candidates"] > 1 << 16, st  # more than the lists' first capacity: they grew
        assert 0 < st["kept"] <= st["foreground"] <= st["candidates"], st
    pipe.close()
    if route == "blobs1":
        # the large disc alone: more than 2048 foreground pixels per image, K4b's dense-plane path
        k = names.index("large_component")
        one = _pipeline(monkeypatch, W, H, F, 1, [tss[k]])
        one.set_option("blobs", 1)
        one.run(torch.from_numpy(np.ascontiguousarray(slab[:, k:k + 1])).to(DEV), d_mu[k:k + 1].contiguous(),
                d_s6[k:k + 1].contiguous(), _st())
        assert_same(one.result(0), refs[k], (W, H, route, "large_component alone"))
        assert one.blob_stats()["large_slots"] > 0, one.blob_stats()
        one.close()


# ---- 2. stack-length edges of the batched pipeline -------------------------------------------------------------------

LAZY_CONFIGS = [("0", None, None), ("1", None, None), ("1", "1", "1")]  # one block / F/2 + 4 then F/5 / one frame each


@pytest.mark.parametrize("F", edgescenes.STACK_LENGTHS)
def test_stack_length_edges_equal_oracle(oracle, monkeypatch, F):
    W, H = 512, 48  # fast-path width: chained trigger search with deferred pieces
    for tss in (4, 16):
        mu, sg = oracle.welford(synth.training_pairs(W, H, tss // 2, 0, 30))
        frames, onsets = edgescenes.trigger_stacks(W, H, F, seed=7 * F + tss)
        E = len(onsets)
        refs = [oracle_event(oracle, frames[e], mu, sg, tss) for e in range(E)]
        if F >= 6:
            assert any(r[0] == 0 and len(r[2]) > 0 for r in refs), (F, tss)
        d_slab = torch.from_numpy(np.ascontiguousarray(frames[:, None])).to(DEV)
        d_mu = torch.from_numpy(mu[None]).to(DEV)
        d_s6 = hip.sigma6(torch.from_numpy(sg[None]).to(DEV))
        for lazy, block0, block in LAZY_CONFIGS:
            monkeypatch.setenv("ABUB_PIPE_LAZY", lazy)
            for k, v in (("ABUB_PIPE_BLOCK0", block0), ("ABUB_PIPE_BLOCK", block)):
                if v:
                    monkeypatch.setenv(k, v)
                else:
                    monkeypatch.delenv(k, raising=False)
            pipe = host.Pipeline(0, W, H, F, E, 1, [tss], nthreads=4)
            pipe.run(d_slab, d_mu, d_s6, _st())
            for e in range(E):
                assert_same(pipe.result(e), refs[e], (F, tss, lazy, block0, onsets[e]))
            jobs = pipe.timing()["trigger_jobs"]
            assert jobs <= E * (F - 1), (F, tss, lazy, block0, jobs)
            pipe.close()
    for k in ("ABUB_PIPE_LAZY", "ABUB_PIPE_BLOCK0", "ABUB_PIPE_BLOCK"):
        monkeypatch.delenv(k, raising=False)


# ---- 3. kernel extremes against numpy ----------------------------------------------------------------------------------

def np_posttrig(f, mu, sg):
    """|f - mu| - 6 sigma, saturated (int64: 6 sigma may exceed 255), 3x3 box with reflect-101 borders, (S + 4) / 9"""
    o = np.clip(np.abs(f.astype(np.int64) - mu.astype(np.int64)) - 6 * sg.astype(np.int64), 0, 255)
    p = np.pad(o, 1, mode="reflect")
    H, W = o.shape
    S = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return ((S + 4) // 9).astype(np.uint8)


K3_SHAPES = [(1280, 48), (1680, 37), (322, 37)]  # fast path: 5 jobs per scanning wave / 4 per wave; generic kernel


@pytest.mark.parametrize("W,H", K3_SHAPES)
def test_k3_saturated_inputs(oracle, W, H):
    """K3 (store mode and histograms only) under every K3 knob, on frames of 0 / 255 / mid-range values against models
    whose mu + 6 sigma saturates: mu of 255 with 6 sigma from 6 to 90 (the scan's HI = min(mu + 6 sigma, 255)), mu of
    255 / 0, sigma of 0, 42 (6 sigma = 252) and 43, 60, 255 (6 sigma clipped at 255).  One launch per model, so that
    every scanning wave of the fast path serves jobs of one model and the zero scan, its suspect lists and the exact tails
    run; one more launch with the models interleaved (mixed waves: their chunks go to the row machine whole)."""
    rs = np.random.RandomState(W + H)
    nf, nm = 6, 5
    fr = np.zeros((nf, H, W), np.uint8)
    fr[1] = 255
    fr[2] = rs.choice(np.array([0, 255], np.uint8), (H, W))
    fr[3] = np.where((np.arange(W)[None] // 7 + np.arange(H)[:, None] // 5) % 2, 255, 0)
    fr[3, H // 2, :] = rs.randint(0, 256, W)
    fr[4] = rs.randint(128, 191, (H, W))  # mid-range: above mu + 6 sigma - 256 and below 255 - 6 sigma for model 3
    fr[5] = rs.randint(0, 256, (H, W))
    mu = np.zeros((nm, H, W), np.uint8)
    sg = np.zeros((nm, H, W), np.uint8)
    mu[0] = 255
    sg[1, :, : W // 2] = 43
    mu[2] = rs.choice(np.array([0, 255], np.uint8), (H, W))
    sg[2] = rs.choice(np.array([0, 42, 43, 60, 255], np.uint8), (H, W))
    mu[3] = 255
    sg[3] = np.array([1, 5, 10, 15], np.uint8)[(np.arange(W) * 4) // W][None]  # bands of 6 sigma = 6, 30, 60, 90:
    # mu + 6 sigma saturates; a wrapped sum (6 sigma - 1) below a mid-range frame value would hide |f - mu| - 6 sigma
    mu[4] = rs.choice(np.array([200, 254, 255], np.uint8), (H, W))
    sg[4] = rs.choice(np.array([1, 7, 13, 21, 43], np.uint8), (H, W))
    O = {(f, m): oracle.posttrig_frame(fr[f], mu[m], sg[m]) for f in range(nf) for m in range(nm)}
    for (f, m), o in O.items():
        assert np.array_equal(o, np_posttrig(fr[f], mu[m], sg[m])), (f, m)  # the oracle itself, at these values
    assert O[(4, 3)].any() and not O[(1, 0)].any() and (O[(0, 0)] == 255).all()
    f_d, mu_d = torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    assert np.array_equal(s6.cpu().numpy(), np.minimum(6 * sg.astype(np.int64), 255))
    launches = [[(f, 0, m, f) for f in range(nf)] for m in range(nm)]            # model-major: one model per launch
    launches.append([(f, 0, m, nm * f + m) for f in range(nf) for m in range(nm)])  # interleaved models
    j_ds = [hip.make_jobs(jobs, DEV) for jobs in launches]
    for (scan, lst, budget, chunks) in K3_MATRIX:
        key = (W, H, scan, lst, budget, chunks)
        for k, v in (("scan", scan), ("list", lst), ("budget", budget), ("chunks", chunks)):
            hip.k3_set_option(k, v)
        for jobs, j_d in zip(launches, j_ds):
            want = [O[(f, m)] for (f, _, m, _) in sorted(jobs, key=lambda j: j[3])]
            href = np.stack([np.bincount(o.ravel(), minlength=256) for o in want])
            hist, img = hip.posttrig(f_d, mu_d, s6, j_d, W, H)
            hist2, _ = hip.posttrig(f_d, mu_d, s6, j_d, W, H, store=False)
            torch.cuda.synchronize()
            assert np.array_equal(hist.cpu().numpy(), href), (key, jobs[0])
            assert np.array_equal(hist2.cpu().numpy(), href), (key, jobs[0])
            got = img.cpu().numpy()
            for j, o in enumerate(want):
                assert np.array_equal(got[j], o), (key, jobs[0], j)


def _degenerate_hists(P):
    """all pixels in one bin, only the values 0 and 255, only bin 255 -- as histograms of P pixels"""
    out = []
    for b in (0, 1, 3, 4, 128, 254, 255):
        h = np.zeros(256, np.int64)
        h[b] = P
        out.append(h)
    for n255 in (P // 2, 1, P - 1):
        h = np.zeros(256, np.int64)
        h[255], h[0] = n255, P - n255
        out.append(h)
    return out


@pytest.mark.parametrize("W,H", [(40, 24), (1280, 1024)])
def test_device_otsu_degenerate_histograms(oracle, W, H):
    from test_oracle_primitives import np_otsu

    P = W * H
    hists, tz = [], []
    for h in _degenerate_hists(P):
        for t in (0, 3, 128, 254, 255):
            hists.append(h)
            tz.append(t)
    hists = np.array(hists, np.uint32)
    tz = np.array(tz, np.int32)
    got = hip.binarize_thr(torch.from_numpy(hists.view(np.int32)).to(DEV), torch.from_numpy(tz).to(DEV), W, H).cpu().numpy()
    for k, (h, t) in enumerate(zip(hists, tz)):
        folded = np.where(np.arange(256) <= t, 0, h).astype(np.int64)
        folded[0] += int(h[: t + 1].sum())
        want = max(int(t), np_otsu(folded))  # mask = tozero(v) > T  <=>  v > max(tozero, T)
        assert want == max(int(t), oracle.otsu(folded.astype(np.uint32), P)), k
        assert got[k] == want == host.binarize_threshold(h, P, int(t)), (k, int(t), int(got[k]), want)


def _ring(H, W, v=200):
    img = np.zeros((H, W), np.uint8)
    img[0, :] = img[-1, :] = v
    img[:, 0] = img[:, -1] = v
    return img


@pytest.mark.parametrize("W,H", [(1280, 48), (322, 37), (40, 24)])
def test_k4_full_and_ring_masks(W, H):
    """abub_fg_compact_dev on an image that is all foreground (255, and 1 with threshold 0) and on a one-pixel ring round
    the border: exactly those raster indices, nothing past cap"""
    P = W * H
    imgs = np.stack([np.full((H, W), 255, np.uint8), np.full((H, W), 1, np.uint8), _ring(H, W), _ring(H, W, 4)])
    thr = np.array([-1, 0, 3, 3], np.int32)
    exp = [np.flatnonzero(im.ravel() > max(t, -1)) for im, t in zip(imgs, thr)]
    assert len(exp[0]) == len(exp[1]) == P and len(exp[2]) == len(exp[3]) == 2 * W + 2 * H - 4
    i_d, t_d = torch.from_numpy(imgs).to(DEV), torch.from_numpy(thr).to(DEV)
    idx = torch.full((len(imgs) * P + 64,), SENT, dtype=torch.int32, device=DEV)
    cnt = torch.zeros((len(imgs),), dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_fg_compact_dev(i_d.data_ptr(), len(imgs), W, H, t_d.data_ptr(), idx.data_ptr(), P,
                                              cnt.data_ptr(), _st()), "abub_fg_compact_dev")
    torch.cuda.synchronize()
    ix, ct = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    assert (ix[len(imgs) * P:] == SENT).all()
    for k, e in enumerate(exp):
        assert ct[k] == len(e), k
        assert np.array_equal(np.sort(ix[k * P: k * P + ct[k]]), e), k
        assert (ix[k * P + ct[k]:(k + 1) * P] == SENT).all(), k


@pytest.mark.parametrize("W,H", [(1280, 48), (322, 37), (40, 24)])
def test_k4b_full_and_ring_masks(W, H):
    """K4b on the same masks: one 8-connected component with the frame as its box (first pixel 0), kept unless the
    minimum box area is the frame's own; slots with more than 2048 foreground pixels take the dense-plane path"""
    P = W * H
    rs = np.random.RandomState(P)
    full = rs.randint(1, 256, (H, W)).astype(np.uint8)
    ring = _ring(H, W)
    imgs = [full, ring, full, ring]
    mb = np.array([-1, 10, P, P - 1], np.int32)  # box area P: kept only if P > min box area
    offs, idx, val = [0], [], []
    for v in imgs:
        i = np.flatnonzero(v.ravel())
        rs.shuffle(i)
        idx.append(i)
        val.append(v.ravel()[i])
        offs.append(offs[-1] + len(i))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)  # noqa: E731
    out = hip.label_blobs(t(offs, np.int32), t(np.concatenate(idx), np.int32), t(np.concatenate(val), np.uint8),
                          t(np.zeros(4), np.int32), t(mb, np.int32), W, H)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    ko, co = out["kept_off"].astype(np.int64), out["comp_off"].astype(np.int64)
    for s, v in enumerate(imgs):
        fg = np.flatnonzero(v.ravel())
        keep = mb[s] < 0 or P > mb[s]
        assert out["ncomp"][s] == 1 and out["nkept_comp"][s] == int(keep), s
        assert np.array_equal(out["kept_idx"][ko[s]:ko[s + 1]], fg if keep else fg[:0]), s
        want = [(0, 0, 0, W - 1, H - 1, len(fg))] if keep else []
        assert [tuple(int(x) for x in r) for r in out["comp"][co[s]:co[s + 1]]] == want, s
    nfg = [int((v > 0).sum()) for v in imgs]
    assert list(out["stats"]) == [sum(n > 2048 for n in nfg), sum(nfg), 4, int(sum(mb[s] < 0 or P > mb[s] for s in range(4)))]
