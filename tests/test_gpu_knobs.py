"""Paths that only a tuning knob reaches, and the candidate-list kernels of the batched pipeline.

INTEGRATION.md promises that no K2 / K3 knob changes a result.  Every knob-selected path here (K2 row machine with the
two-row prefetch ring, K2 / K3 chunking, K3 without its zero scan, K3's in-wave suspect tails, mid-chunk hand-over) is
checked against the CPU oracle, and so is the pipeline under those knobs.  The list kernels (K4 compaction, grouping by
slot, sat-subtract histogram, pair histogram) are checked against numpy at the shapes and edges where they can go
wrong: partial 16-byte words, grid-stride loops, overflow of the caller's capacity, runs of one slot across wave and
block boundaries, the multi-element scan of more than 1024 slots."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib, hip, host, synth  # noqa: E402

DEV = "cuda:0"
SENT = 0x5A5A5A5A  # canary word


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(autouse=True)
def _defaults():
    """Every test starts from (and leaves behind) the default K2 and K3 launcher options."""
    yield
    for k, v in (("bound", 1), ("chain", -1), ("budget", 1024), ("split", 1), ("list", 0), ("wg", -1), ("sync", -1),
                 ("scanpf", -1), ("pf", 1), ("chunks", 0)):
        hip.k2_set_option(k, v)
    for k, v in (("scan", 1), ("list", 1), ("budget", 512), ("chunks", 0)):
        hip.k3_set_option(k, v)


def _st():
    return torch.cuda.current_stream().cuda_stream


def u32(t):
    return t.cpu().numpy().astype(np.uint32)


def rnd_frames(rs, n, H, W, amp=12):
    base = rs.randint(30, 200, (H, W))
    return np.clip(base[None] + rs.randint(-amp, amp + 1, (n, H, W)), 0, 255).astype(np.uint8)


def check_list(pairs, count, imgs, thr, slot_base):
    """The fused list holds exactly the pixels of imgs[k] with value > thr[k] (a negative thr lists like 0), tagged
    slot_base + k, with their values."""
    n = int(count.item())
    pr = u32(pairs[:n])
    total = 0
    for k, img in enumerate(imgs):
        sel = pr[(pr[:, 0] & 0xFFFFFF) == slot_base + k]
        exp = np.flatnonzero(img.ravel() > max(int(thr[k]), 0))
        order = np.argsort(sel[:, 1], kind="stable")
        assert np.array_equal(sel[order, 1], exp), k
        assert np.array_equal((sel[order, 0] >> 24).astype(np.uint8), img.ravel()[exp]), k
        total += len(exp)
    assert total == n


def k2_compact(f_d, s6, j_d, n, W, H, cthr, slot_base, cap=1 << 21):
    pairs = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    hist = torch.empty((n, 256), dtype=torch.int32, device=DEV)
    c_d = torch.tensor(cthr, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_diff_hist_compact_dev(f_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H, hist.data_ptr(),
                                                     None, c_d.data_ptr(), pairs.data_ptr(), cap, count.data_ptr(),
                                                     slot_base, _st()), "abub_diff_hist_compact_dev")
    torch.cuda.synchronize()
    return hist, pairs, count


def k3_compact(f_d, mu_d, s6, j_d, n, W, H, cthr, slot_base, cap=1 << 21, pairs=None, count=None):
    if pairs is None:
        pairs = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
        count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    hist = torch.empty((n, 256), dtype=torch.int32, device=DEV)
    c_d = torch.tensor(cthr, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_posttrig_compact_dev(f_d.data_ptr(), mu_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H,
                                                    hist.data_ptr(), None, c_d.data_ptr(), pairs.data_ptr(), pairs.shape[0],
                                                    count.data_ptr(), slot_base, _st()), "abub_posttrig_compact_dev")
    torch.cuda.synchronize()
    return hist, pairs, count


# ---- 1. K2 row machine with the two-row prefetch ring (option "pf" = 2) --------------------------------------------

PF2_SHAPES = [
    (64, 1280, 0), (50, 1680, 0), (37, 256, 8), (40, 512, 16), (33, 768, 0), (16, 1024, 8), (9, 1536, 0), (21, 2048, 8),
    (64, 100, 16),                                      # every fast-path NDW (5, 7, 1, 2, 3, 4, 6, 8, 1 with 25 lanes)
    (17, 1280, 16), (33, 1680, 16), (17, 256, 16), (2, 1024, 16), (1, 512, 0),  # last chunk shorter than the ring
] + [(37, W, R) for W in (264, 276, 560, 1100, 792, 1400, 1088) for R in (0, 16)]  # partial waves of NDW = 2 .. 8


@pytest.mark.parametrize("H,W,R", PF2_SHAPES)
def test_k2_prefetch_ring_pf2(oracle, H, W, R):
    rs = np.random.RandomState(H * 7919 + W)
    n = 6
    frames = rnd_frames(rs, n, H, W, amp=14)
    frames[3, H // 2:, : W // 3] = np.clip(frames[3, H // 2:, : W // 3].astype(int) + 40, 0, 255)  # a dense block
    sigma = rs.randint(0, 3, (2, H, W)).astype(np.uint8)
    jobs = [(i, max(i - 2, 0), i % 2, k) for k, i in enumerate(range(1, n))]
    Dref = np.stack([oracle.process_frame(frames[c], frames[r], sigma[m]) for (c, r, m, _) in jobs])
    href = np.stack([oracle.hist256(D) for D in Dref])
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    j_d = hip.make_jobs(jobs, DEV)
    cthr = [2, 0, 5, 3, 1]
    hip.k2_set_option("pf", 2)
    for bound, budget in ((0, 1024), (1, 8)):
        hip.k2_set_option("bound", bound)
        hip.k2_set_option("budget", budget)
        for store in (True, False):
            hist, D = hip.diff_hist(f_d, s6, j_d, W, H, store=store, rows_per_chunk=R)
            torch.cuda.synchronize()
            assert np.array_equal(u32(hist), href), (bound, budget, store)
            if store:
                assert np.array_equal(D.cpu().numpy(), Dref), (bound, budget)
        hist, pairs, count = k2_compact(f_d, s6, j_d, len(jobs), W, H, cthr, 11)
        assert np.array_equal(u32(hist), href), (bound, budget)
        check_list(pairs, count, Dref, cthr, 11)


# ---- 2. K2 chunk height chosen by the "chunks" option ---------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1280, 1024), (1680, 1050)])
def test_k2_chunks_option(oracle, W, H):
    """Chunk edges decide where the halo rows are re-read and where the scan's suspect lists restart; 1050 rows leave
    a short last chunk for 64 chunks (17 rows each).  A bubble, a frame that differs everywhere and scattered small
    excursions across every chunk edge; D and histograms == oracle for every chunking and pass."""
    rs = np.random.RandomState(W + H)
    F = 6
    spec = synth.EventSpec(F, t0=2, bubbles=[(W // 3, H // 2, 40), (2 * W // 3, H // 4, -40)])
    fr = synth.render_event(W, H, spec, 31, 0).astype(np.int32)
    fr[4] += 25                                                       # dense everywhere: hand-over of whole chunks
    for f in range(F):
        k = 3000
        fr[f, rs.randint(0, H, k), rs.randint(0, W, k)] += rs.randint(3, 9, k)
    frames = np.clip(fr, 0, 255).astype(np.uint8)
    sigma = np.ones((1, H, W), np.uint8)
    jl = [(i, max(i - 2, 0), 0, i - 1) for i in range(1, F)]
    Dref = np.stack([oracle.process_frame(frames[c], frames[r], sigma[0]) for (c, r, _, _) in jl])
    href = np.stack([oracle.hist256(D) for D in Dref])
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    j_d = hip.make_jobs(jl, DEV)
    for chunks in (8, 16, 64):
        hip.k2_set_option("chunks", chunks)
        for bound in (1, 0):
            hip.k2_set_option("bound", bound)
            hist, D = hip.diff_hist(f_d, s6, j_d, W, H, store=True)
            assert np.array_equal(u32(hist), href), (chunks, bound)
            assert np.array_equal(D.cpu().numpy(), Dref), (chunks, bound)
            hist, _ = hip.diff_hist(f_d, s6, j_d, W, H, store=False)
            assert np.array_equal(u32(hist), href), (chunks, bound)
            hist, _ = hip.diff_hist(f_d, s6, j_d, W, H, store=False, chain=(F - 1, 2))
            assert np.array_equal(u32(hist), href), (chunks, bound)
        hip.k2_set_option("bound", 1)
        hist, D = hip.diff_hist(f_d, s6, j_d, W, H, store=True, chain=(F - 1, 2))  # chained store
        assert np.array_equal(u32(hist), href) and np.array_equal(D.cpu().numpy(), Dref), chunks
        # deferred rows: the pieces call recomputes the deferred launch's chunking from the same options
        hist, state = hip.diff_hist_deferred(f_d, s6, j_d, W, H, chain=(F - 1, 2))
        torch.cuda.synchronize()
        assert state[2].cpu().numpy().any(), chunks
        hip.diff_hist_pieces(f_d, s6, j_d, W, H, hist, state, state[2].clone())
        torch.cuda.synchronize()
        assert np.array_equal(u32(hist), href), chunks
        cthr = [3, 0, 7, 2, 4]
        hist, pairs, count = k2_compact(f_d, s6, j_d, F - 1, W, H, cthr, 0, cap=1 << 23)
        assert np.array_equal(u32(hist), href), chunks
        check_list(pairs, count, Dref, cthr, 0)


# ---- 3. K3 knob matrix ----------------------------------------------------------------------------------------------

K3_MATRIX = [(scan, lst, budget, chunks) for scan in (0, 1) for lst in (0, 1) for budget in (512, 1, 8) for chunks in (0, 8, 64)]


def k3_check_matrix(oracle, fr, mu, sg, jobs, W, H, cthr, combos):
    O = [oracle.posttrig_frame(fr[c], mu[m], sg[m]) for (c, _, m, _) in jobs]
    href = np.stack([oracle.hist256(o) for o in O])
    f_d, mu_d = torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    j_d = hip.make_jobs(jobs, DEV)
    for (scan, lst, budget, chunks) in combos:
        key = (W, H, scan, lst, budget, chunks)
        hip.k3_set_option("scan", scan)
        hip.k3_set_option("list", lst)
        hip.k3_set_option("budget", budget)
        hip.k3_set_option("chunks", chunks)
        hist, img = hip.posttrig(f_d, mu_d, s6, j_d, W, H)
        torch.cuda.synchronize()
        assert np.array_equal(u32(hist), href), key
        assert np.array_equal(img.cpu().numpy(), np.stack(O)), key
        if _lib.lib().abub_fast_path(W):
            hist, pairs, count = k3_compact(f_d, mu_d, s6, j_d, len(jobs), W, H, cthr, 7)
            assert int(count.item()) <= pairs.shape[0]
            assert np.array_equal(u32(hist), href), key
            check_list(pairs, count, O, cthr, 7)
    return O


@pytest.mark.parametrize("H,W", [(40, 56), (3, 3), (17, 5), (64, 1280), (1, 7), (50, 1680), (9, 2048), (33, 768), (2, 512),
                                 (1, 256)])
def test_k3_knob_matrix(oracle, H, W):
    rs = np.random.RandomState(H * 3 + W)
    fr = rnd_frames(rs, 3, H, W, amp=25)
    mu = rs.randint(0, 256, (2, H, W)).astype(np.uint8)
    mu[0] = np.clip(fr[0].astype(int) + rs.randint(-2, 3, (H, W)), 0, 255)
    sg = rs.randint(0, 3, (2, H, W)).astype(np.uint8)
    jobs = [(0, 0, 0, 0), (1, 0, 1, 1), (2, 0, 0, 2)]
    k3_check_matrix(oracle, fr, mu, sg, jobs, W, H, [3, -1, 0], K3_MATRIX)


@pytest.mark.parametrize("W,H", [(1280, 1024), (1680, 1050)])
def test_k3_knob_matrix_full_size(oracle, W, H):
    """The stripe scene of test_k3_suspect_list_paths (about 30 suspect groups in every row: mid-scan flushes of the
    LDS lists, the global list overflows its 64 K minimum with three such jobs), a tracked bubble and a quiet frame,
    under every K3 knob combination."""
    rs = np.random.RandomState(5)
    mu = rs.randint(40, 180, (1, H, W)).astype(np.uint8)
    sg = np.ones((1, H, W), np.uint8)
    sg[0, ::97, ::89] = 0
    fr = np.repeat(mu, 5, axis=0).astype(np.int32) + rs.randint(-1, 2, (5, H, W))
    for k in range(3):
        for x in range(40 + 13 * k, W - 20, 250):
            fr[k, :, x:x + 9] += 30 + k
    yy, xx = np.ogrid[:H, :W]
    fr[3][(yy - 500) ** 2 + (xx - 700) ** 2 <= 45 ** 2] += 50
    fr = np.clip(fr, 0, 255).astype(np.uint8)
    jobs = [(k, 0, 0, k) for k in range(5)]
    O = k3_check_matrix(oracle, fr, mu, sg, jobs, W, H, [3, 0, 5, -1, 3], K3_MATRIX)
    assert int((O[0] > 0).sum()) > 5 * 7 * H and int((O[4] > 0).sum()) < 100


# ---- 4. the batched pipeline under knobs ----------------------------------------------------------------------------

def scene_batched(oracle, W, H):
    """The scene of test_batched_pipeline_equals_oracle."""
    F, E, C = 41, 7, 2
    slab = np.zeros((E, C, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C):
            spec = synth.random_spec(W, H, F, 500 + e, c, p_second=0.4, p_none=0.2, p_flicker=0.3, margin=25)
            slab[e, c] = synth.render_event(W, H, spec, 500 + e, c)
    quiet = synth.render_event(W, H, synth.EventSpec(F), 900, 0)
    quiet[12:] = np.clip(quiet[12:].astype(int) + 1, 0, 255)
    slab[E - 1, 0] = quiet
    tr0 = synth.training_pairs(W, H, 10, 0, F)
    tr1 = synth.training_pairs(W, H, 2, 1, F)
    return slab, [oracle.welford(tr0), oracle.welford(tr1)], [len(tr0), len(tr1)]


def scene_noisy(oracle, W=1280, H=96):
    """The "noisy" regime of the lazy trigger-search test: hot pixels everywhere, every reached frame is dense."""
    F, E, C = 41, 6, 2
    slab = np.zeros((E, C, F, H, W), np.uint8)
    for e in range(E):
        for c in range(C):
            spec = synth.random_spec(W, H, F, 700 + e, c, p_second=0.3, p_none=0.15, p_flicker=0.3, margin=25, regime="noisy")
            slab[e, c] = synth.render_event(W, H, spec, 700 + e, c)
    models, tss = [], []
    for c in range(C):
        tr = np.concatenate([slab[e, c, :2] for e in range(E)])
        models.append(oracle.welford(tr))
        tss.append(len(tr))
    return slab, models, tss


def pipe_check(pipe, d, refs, key):
    pipe.run(*d, torch.cuda.current_stream().cuda_stream)
    for s, ref in enumerate(refs):
        staged, state, bubbles, err = pipe.result(s)
        assert (staged, state) == (ref[0], ref[1]), (key, s, staged, state, ref[0], ref[1], err)
        assert [[tuple(q[k] for k in "xywh") for q in b["desc"]] for b in bubbles] == \
               [[tuple(q[k] for k in "xywh") for q in r["desc"]] for r in ref[2]], (key, s)
        for b, r in zip(bubbles, ref[2]):
            for q, p in zip(b["desc"], r["desc"]):
                assert abs(q["cx"] - p["cx"]) <= 1e-4 and abs(q["cy"] - p["cy"]) <= 1e-4, (key, s)


@pytest.mark.parametrize("scene", ["batched-1280x128", "batched-322x120", "noisy-1280x96"])
def test_pipeline_under_knobs(oracle, scene):
    if scene.startswith("noisy"):
        slab, models, tss = scene_noisy(oracle)
    else:
        W, H = (1280, 128) if "1280" in scene else (322, 120)
        slab, models, tss = scene_batched(oracle, W, H)
    E, C, F, H, W = slab.shape
    refs = []
    for e in range(E):
        for c in range(C):
            a = oracle.Analyzer(slab[e, c], models[c][0], models[c][1], tss[c])
            refs.append(a.any_cam_analysis())
            a.close()
    d = (torch.from_numpy(slab).to(DEV), torch.from_numpy(np.stack([m[0] for m in models])).to(DEV),
         hip.sigma6(torch.from_numpy(np.stack([m[1] for m in models])).to(DEV)))
    for knob, name, value in (("k2", "bound", 0), ("k2", "pf", 2), ("k3", "scan", 0), ("k3", "list", 0)):
        (hip.k2_set_option if knob == "k2" else hip.k3_set_option)(name, value)
        pipe = host.Pipeline(0, W, H, F, E, C, tss, nthreads=4)
        pipe_check(pipe, d, refs, (scene, knob, name, value))
        pipe.close()
        (hip.k2_set_option if knob == "k2" else hip.k3_set_option)(name, {"bound": 1, "pf": 1, "scan": 1, "list": 1}[name])
    # "bound" switched off after the pipeline was made (and ran once with deferred pieces)
    pipe = host.Pipeline(0, W, H, F, E, C, tss, nthreads=4)
    pipe_check(pipe, d, refs, (scene, "bound on"))
    hip.k2_set_option("bound", 0)
    pipe_check(pipe, d, refs, (scene, "bound off after construction"))
    hip.k2_set_option("bound", 1)
    pipe_check(pipe, d, refs, (scene, "bound back on"))
    pipe.close()


# ---- 5. list kernels against numpy ----------------------------------------------------------------------------------

def list_images(rs, n, H, W):
    img = rs.choice(np.array([0, 0, 0, 0, 1, 3, 128, 254, 255, 255], np.uint8), (n, H, W))
    if n > 1:
        img[0] = 0                       # an empty image
        img[-1] = 255                    # a saturated one
    return img


@pytest.mark.parametrize("W,H,n", [(16, 4, 1), (16, 4, 300), (13, 7, 1), (13, 7, 300), (1, 1, 1), (1, 1, 37), (40, 30, 57),
                                   (1680, 1050, 3), (1679, 1050, 2)])
def test_k4_compaction_against_numpy(W, H, n):
    """abub_fg_compact_dev / abub_fg_compact_pairs_dev: the 16-byte path (P % 16 == 0), the scalar path, grid-stride
    loops at full size (the grids are capped at 512 / 64 blocks); thresholds -1 (value 0 admitted), 0, 254, 255 (nothing).
    Per image the listed (index, value) multiset == numpy's; on overflow the true count is reported and nothing is
    written past cap."""
    rs = np.random.RandomState(W * 131 + H * 7 + n)
    img = list_images(rs, n, H, W)
    P = W * H
    thr = np.array([(-1, 0, 254, 255)[k % 4] for k in range(n)], np.int32)
    if n == 1:
        thr[0] = -1
    exp = [np.flatnonzero(img[k].ravel() > thr[k]) for k in range(n)]
    i_d, t_d = torch.from_numpy(img).to(DEV), torch.from_numpy(thr).to(DEV)
    L = _lib.lib()
    # per-image lists: idx [n][cap] and a canary row behind
    for cap in (P, max(P // 3, 1)):
        idx = torch.full((n * cap + 64,), SENT, dtype=torch.int32, device=DEV)
        cnt = torch.zeros((n,), dtype=torch.int32, device=DEV)
        _lib.check(L.abub_fg_compact_dev(i_d.data_ptr(), n, W, H, t_d.data_ptr(), idx.data_ptr(), cap, cnt.data_ptr(), _st()),
                   "abub_fg_compact_dev")
        torch.cuda.synchronize()
        ix, ct = u32(idx), cnt.cpu().numpy()
        assert (ix[n * cap:] == SENT).all()
        for k in range(n):
            assert ct[k] == len(exp[k]), (k, thr[k], cap)
            got = np.sort(ix[k * cap: k * cap + min(ct[k], cap)])
            if ct[k] <= cap:
                assert np.array_equal(got, exp[k]), (k, thr[k])
                assert (ix[k * cap + ct[k]:(k + 1) * cap] == SENT).all(), k
            else:
                assert len(np.unique(got)) == cap and np.isin(got, exp[k]).all(), (k, thr[k])
    # one shared (image | value << 24, index) list
    total = sum(len(e) for e in exp)
    for cap in (total + 1, max(total // 2, 1)):
        pairs = torch.full((cap + 32, 2), SENT, dtype=torch.int32, device=DEV)
        count = torch.full((1,), 12345, dtype=torch.int32, device=DEV)  # the launcher zeroes it
        _lib.check(L.abub_fg_compact_pairs_dev(i_d.data_ptr(), n, W, H, t_d.data_ptr(), pairs.data_ptr(), cap,
                                               count.data_ptr(), _st()), "abub_fg_compact_pairs_dev")
        torch.cuda.synchronize()
        assert int(count.item()) == total, cap
        pr = u32(pairs)
        assert (pr[cap:] == SENT).all()
        got = pr[:min(total, cap)]
        slot, val, ix = got[:, 0] & 0xFFFFFF, got[:, 0] >> 24, got[:, 1]
        assert (slot < n).all() and (ix < P).all()
        assert np.array_equal(val, img.reshape(n, P)[slot, ix])
        keys = slot.astype(np.int64) * P + ix
        assert len(np.unique(keys)) == len(keys)
        want = np.concatenate([k * P + e for k, e in enumerate(exp)]) if total else np.zeros(0, np.int64)
        if total <= cap:
            assert np.array_equal(np.sort(keys), np.sort(want))
        else:
            assert np.isin(keys, want).all()


def group_ref(w0, w1, nslots):
    """numpy counting sort: per slot the multiset of (index, value); entries with slot >= nslots dropped."""
    s = w0 & 0xFFFFFF
    keep = s < nslots
    cnt = np.bincount(s[keep], minlength=nslots)[:nslots]
    return s, keep, cnt


def run_group(L, pairs_np, count, cap, nslots, hist=None, cthr=None):
    pairs = torch.from_numpy(pairs_np.view(np.int32)).to(DEV) if len(pairs_np) else torch.zeros((1, 2), dtype=torch.int32,
                                                                                                   device=DEV)
    c_d = torch.tensor([count], dtype=torch.int64, device=DEV).to(torch.int32)
    scratch = torch.zeros((2 * nslots,), dtype=torch.int32, device=DEV)
    offsets = torch.full((nslots + 1,), SENT, dtype=torch.int32, device=DEV)
    idx = torch.full((cap + 64,), SENT, dtype=torch.int32, device=DEV)
    val = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    if hist is None:
        _lib.check(L.abub_pairs_group_dev(pairs.data_ptr(), c_d.data_ptr(), cap, nslots, scratch.data_ptr(),
                                          offsets.data_ptr(), idx.data_ptr(), val.data_ptr(), _st()), "abub_pairs_group_dev")
    else:
        h_d = torch.from_numpy(hist.astype(np.int32)).to(DEV)
        t_d = torch.from_numpy(np.asarray(cthr, np.int32)).to(DEV)
        _lib.check(L.abub_pairs_group_hist_dev(pairs.data_ptr(), c_d.data_ptr(), cap, nslots, scratch.data_ptr(),
                                               offsets.data_ptr(), idx.data_ptr(), val.data_ptr(), h_d.data_ptr(),
                                               t_d.data_ptr(), _st()), "abub_pairs_group_hist_dev")
    torch.cuda.synchronize()
    return u32(offsets).astype(np.int64), u32(idx), val.cpu().numpy()


def synth_list(rs, nslots, kind):
    """(w0, w1) u32 arrays: 'shuffled' -- random slots (some empty); 'runs' -- runs of one slot of lengths 1 .. 300 in
    list order, so that runs cross 64-entry (wave) and 256-entry (block) boundaries; values 1 .. 255."""
    used = np.sort(rs.choice(nslots, max(1, (nslots * 2) // 3), replace=False))  # a third of the slots stay empty
    if kind == "shuffled":
        n = int(rs.randint(3000, 9000))
        s = rs.choice(used, n)
    else:
        parts = []
        lens = [1, 63, 64, 65, 127, 200, 255, 256, 257, 300, 2, 3, 129]
        for r in range(60):
            parts.append(np.full(lens[r % len(lens)], used[rs.randint(len(used))]))
        s = np.concatenate(parts)
    n = len(s)
    v = rs.randint(1, 256, n).astype(np.uint32)
    w0 = s.astype(np.uint32) | (v << 24)
    w1 = rs.randint(0, 1 << 22, n).astype(np.uint32)
    return w0, w1


def assert_grouped(off, idx, val, w0, w1, nslots, ncount):
    s, keep, cnt = group_ref(w0[:ncount], w1[:ncount], nslots)
    assert np.array_equal(np.diff(off), cnt) and off[0] == 0 and off[nslots] == cnt.sum()
    for sl in np.flatnonzero(cnt):
        a, b = off[sl], off[sl + 1]
        m = keep & (s == sl)
        got = sorted(zip(idx[a:b].tolist(), val[a:b].tolist()))
        want = sorted(zip(w1[:ncount][m].tolist(), (w0[:ncount][m] >> 24).tolist()))
        assert got == want, sl


@pytest.mark.parametrize("nslots", [1, 63, 1024, 1025, 5000])
@pytest.mark.parametrize("kind", ["shuffled", "runs"])
def test_pairs_group_against_numpy(nslots, kind):
    rs = np.random.RandomState(nslots * 3 + len(kind))
    L = _lib.lib()
    w0, w1 = synth_list(rs, nslots, kind)
    n = len(w0)
    pairs = np.stack([w0, w1], 1)
    # counting form: plain, with out-of-range slots mixed in (dropped), truncated at cap (first cap entries)
    off, idx, val = run_group(L, pairs, n, n, nslots)
    assert_grouped(off, idx, val, w0, w1, nslots, n)
    assert (idx[n:] == SENT).all()
    bad = w0.copy()
    pos = rs.choice(n, n // 10, replace=False)
    bad[pos] = (bad[pos] & 0xFF000000) | rs.randint(nslots, nslots + 1000, len(pos)).astype(np.uint32)
    off, idx, val = run_group(L, np.stack([bad, w1], 1), n, n, nslots)
    assert_grouped(off, idx, val, bad, w1, nslots, n)
    cap = n // 3 + 1
    off, idx, val = run_group(L, pairs, n, cap, nslots)
    assert_grouped(off, idx, val, w0, w1, nslots, cap)
    assert (idx[cap:] == SENT).all() and (val[cap:] == 0x5A).all()
    off, idx, val = run_group(L, pairs, 0, n, nslots)  # empty list
    assert (off == 0).all() and (idx == SENT).all()
    # histogram form: counts = bins above max(cthr, 0) of per-slot histograms that also count pixels the list omits
    s = w0 & 0xFFFFFF
    v = (w0 >> 24).astype(np.int64)
    cthr = rs.choice([-1, 0, 0, 0], nslots).astype(np.int32)
    hist = np.zeros((nslots, 256), np.int64)
    np.add.at(hist, (s.astype(np.int64), v), 1)
    hist[:, 0] += rs.randint(0, 1000, nslots)   # value-0 pixels: never listed (also not with cthr = -1)
    off, idx, val = run_group(L, pairs, n, n, nslots, hist, cthr)
    assert_grouped(off, idx, val, w0, w1, nslots, n)
    # overflow of the histogram form: offsets from the full counts, nothing written at or past cap
    off, idx, val = run_group(L, pairs, n, cap, nslots, hist, cthr)
    cnt = np.bincount(s, minlength=nslots)
    assert np.array_equal(np.diff(off), cnt) and off[nslots] == n
    assert (idx[cap:] == SENT).all() and (val[cap:] == 0x5A).all()
    for sl in np.flatnonzero(cnt):                 # slots whose first-cap entries fit below cap are exact
        m = s[:cap] == sl
        a = off[sl]
        if a + m.sum() <= cap:
            got = sorted(zip(idx[a:a + m.sum()].tolist(), val[a:a + m.sum()].tolist()))
            assert got == sorted(zip(w1[:cap][m].tolist(), (w0[:cap][m] >> 24).tolist())), sl


@pytest.mark.parametrize("W,H", [(1280, 96), (1680, 1050)])
def test_producer_chain_grouped_runs(oracle, W, H):
    """What the pipeline relies on: K2 compaction, then K3 compaction into the same list with slot_base, then
    abub_pairs_group_hist_dev with the producers' histograms -- every slot's run == the oracle image's pixels with value
    > cthr (a negative cthr lists like 0)."""
    rs = np.random.RandomState(W + 3 * H)
    fr = rnd_frames(rs, 5, H, W, amp=14)
    fr[3, H // 3: H // 3 + 40, W // 2: W // 2 + 60] = np.clip(fr[3, H // 3: H // 3 + 40, W // 2: W // 2 + 60].astype(int) + 70, 0, 255)
    mu = fr[0:1].copy()
    sg = rs.randint(0, 2, (1, H, W)).astype(np.uint8)
    f_d, mu_d = torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    jobs2, jobs3 = [(3, 1, 0, 0), (4, 2, 0, 1), (2, 1, 0, 2)], [(3, 0, 0, 0), (4, 0, 0, 1)]
    c2, c3 = [2, 3, -1], [3, 0]
    imgs = [oracle.process_frame(fr[c], fr[r], sg[0]) for (c, r, _, _) in jobs2] + \
           [oracle.posttrig_frame(fr[c], mu[0], sg[0]) for (c, _, _, _) in jobs3]
    cthr = c2 + c3
    cap = 1 << 23
    h2, pairs, count = k2_compact(f_d, s6, hip.make_jobs(jobs2, DEV), 3, W, H, c2, 0, cap=cap)
    h3, pairs, count = k3_compact(f_d, mu_d, s6, hip.make_jobs(jobs3, DEV), 2, W, H, c3, 3, pairs=pairs, count=count)
    n = int(count.item())
    assert 100 < n < cap
    nslots = 5
    hist = torch.cat([h2, h3]).contiguous()
    assert np.array_equal(u32(hist), np.stack([oracle.hist256(i) for i in imgs]))
    off, idx, val = run_group(_lib.lib(), u32(pairs[:n]), n, n, nslots, hist.cpu().numpy(), cthr)
    assert off[nslots] == n
    for sl in range(nslots):
        exp = np.flatnonzero(imgs[sl].ravel() > max(cthr[sl], 0))
        a, b = off[sl], off[sl + 1]
        order = np.argsort(idx[a:b], kind="stable")
        assert np.array_equal(idx[a:b][order], exp), sl
        assert np.array_equal(val[a:b][order], imgs[sl].ravel()[exp]), sl


@pytest.mark.parametrize("W,H", [(1, 1), (13, 7), (4097, 3), (1680, 1050)])
def test_subsat_hist_against_numpy(W, H):
    rs = np.random.RandomState(W + H)
    img = rs.choice(np.array([0, 1, 2, 7, 128, 200, 254, 255], np.uint8), (H, W))
    sub = rs.choice(np.array([0, 0, 1, 3, 100, 255], np.uint8), (H, W))
    exp = np.clip(img.astype(int) - sub.astype(int), 0, 255).astype(np.uint8)
    i_d, s_d = torch.from_numpy(img).to(DEV), torch.from_numpy(sub).to(DEV)
    hist = torch.full((256,), SENT, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_subsat_hist_dev(i_d.data_ptr(), s_d.data_ptr(), W, H, hist.data_ptr(), _st()),
               "abub_subsat_hist_dev")
    torch.cuda.synchronize()
    h = u32(hist).astype(np.int64)
    assert np.array_equal(i_d.cpu().numpy(), exp)
    assert np.array_equal(h, np.bincount(exp.ravel(), minlength=256))
    assert h[0] == W * H - h[1:].sum()


@pytest.mark.parametrize("W,H", [(1280, 1024), (1680, 1050), (13, 7), (333, 77), (1, 1)])
def test_pair_hist_against_oracle(oracle, W, H):
    """abub_pair_hist_dev over 300 pairs that share frames, including cur == ref, == oracle.hist256(sat(f1 - f0))."""
    rs = np.random.RandomState(W * 17 + H)
    nf = 6
    fr = rnd_frames(rs, nf, H, W, amp=60)
    fr[5] = 255
    fr[4] = 0
    pairs = [(int(rs.randint(nf)), int(rs.randint(nf)), 0, k) for k in range(300)]
    pairs[0] = (2, 2, 0, 0)
    pairs[1] = (5, 4, 0, 1)
    pairs[2] = (4, 5, 0, 2)
    h = hip.pair_hist(torch.from_numpy(fr).to(DEV), hip.make_jobs(pairs, DEV), W, H).cpu().numpy().astype(np.uint32)
    ref = {}
    for (a, b, _, o) in pairs:
        if (a, b) not in ref:
            ref[(a, b)] = oracle.hist256(np.clip(fr[a].astype(int) - fr[b].astype(int), 0, 255).astype(np.uint8))
        assert np.array_equal(h[o], ref[(a, b)]), (a, b, o)
