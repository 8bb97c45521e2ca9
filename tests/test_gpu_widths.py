"""The K3 zero scan (k3_bound_scan) and the K2 chained scan (k2_sad_chain) at every width class of the fast path.

Both kernels are instantiated per dwords-per-lane (1 .. 8).  Each class is run here with a full wave (64 lanes) and with
a partial one (the last lane reflects the border, idle lanes shadow lane 0), at heights that give a short last chunk
(40 = 16 + 16 + 8 rows) and at 1, 2, 3 and 17 rows, on scenes that the scan itself has to decide -- the K3 launches keep
one model per wave, since a wave whose jobs differ in model hands its whole chunk to the row machine and scans nothing.
Reference: the CPU oracle; every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scanscenes as sc  # noqa: E402
from autobub3hs_amd import _lib, hip, host  # noqa: E402
from scanscenes import DEV, WIDTHS, check_list, u32  # noqa: E402

HEIGHTS = [40, 1, 2, 3, 17]
K3_KNOBS = [(scan, lst, budget) for scan in (0, 1) for lst in (0, 1) for budget in (512, 8)]
SLOT_BASE = 7


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


def k3_compact(f_d, mu_d, s6, j_d, n, W, H, cthr, slot_base, cap):
    pairs = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    hist = torch.empty((n, 256), dtype=torch.int32, device=DEV)
    c_d = torch.tensor(cthr, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_posttrig_compact_dev(f_d.data_ptr(), mu_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H,
                                                    hist.data_ptr(), None, c_d.data_ptr(), pairs.data_ptr(), cap,
                                                    count.data_ptr(), slot_base, _st()), "abub_posttrig_compact_dev")
    torch.cuda.synchronize()
    return hist, pairs, count


def test_width_table():
    """Every width of the table is a fast-path width of the stated class."""
    for ndw, W in WIDTHS:
        assert _lib.lib().abub_fast_path(W) == 1, W
        assert W % (4 * ndw) == 0 and W // (4 * ndw) <= 64, W
        assert all((W // 4) % d or (W // 4) // d > 64 for d in range(1, ndw)), W


# ---- A1. K3 zero scan with shared-model waves -----------------------------------------------------------------------

def k3_launches(rs, mu, sg, ndw):
    """(name, frames, jobs): eleven jobs of one model (groups of 5+5+1, 4+4+3, 3+3+3+2 jobs per wave), one job alone, and a
    model-major launch of 7 + 4 jobs (a model change inside a wave: that wave hands over, the others scan)."""
    one = sc.k3_scan_frames(rs, mu, sg, [0] * 11, ndw)
    models = [0] * 7 + [1] * 4
    two = sc.k3_scan_frames(rs, mu, sg, models, ndw)
    return [("one model", one, [(k, 0, 0, k) for k in range(11)]),
            ("one job", one, [(0, 0, 0, 0)]),
            ("two models", two, [(k, 0, m, k) for k, m in enumerate(models)])]


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("ndw,W", WIDTHS)
def test_k3_scan_width_matrix(oracle, ndw, W, H):
    rs = np.random.RandomState(W * 41 + H)
    mu, sg = sc.k3_models(rs, H, W)
    mu_d = torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    cthr_all = [3, 0, -1, 5, 2, 0, 7, -1, 1, 4, 0]
    for name, fr, jobs in k3_launches(rs, mu, sg, ndw):
        n = len(jobs)
        O = [oracle.posttrig_frame(fr[c], mu[m], sg[m]) for (c, _, m, _) in jobs]
        href = np.stack([oracle.hist256(o) for o in O])
        if n > 3:
            assert not O[3].any(), name                       # the frame that equals mu
            assert int((O[1] > 0).sum()) >= H * (W // 80), name   # the stripes survive the blur in every row
        assert O[0][H // 2].any(), name                       # the blob
        f_d = torch.from_numpy(fr).to(DEV)
        j_d = hip.make_jobs(jobs, DEV)
        cthr = cthr_all[:n]
        cap = max(int(sum((o > 0).sum() for o in O)), 1) + 64
        for scan, lst, budget in K3_KNOBS:
            key = (name, scan, lst, budget)
            hip.k3_set_option("scan", scan)
            hip.k3_set_option("list", lst)
            hip.k3_set_option("budget", budget)
            hist, img = hip.posttrig(f_d, mu_d, s6, j_d, W, H)
            torch.cuda.synchronize()
            assert np.array_equal(u32(hist), href), key
            assert np.array_equal(img.cpu().numpy(), np.stack(O)), key
            hist, _ = hip.posttrig(f_d, mu_d, s6, j_d, W, H, store=False)
            torch.cuda.synchronize()
            assert np.array_equal(u32(hist), href), key
            hist, pairs, count = k3_compact(f_d, mu_d, s6, j_d, n, W, H, cthr, SLOT_BASE, cap)
            assert np.array_equal(u32(hist), href), key
            check_list(pairs, count, O, cthr, [SLOT_BASE + o for (_, _, _, o) in jobs])


@pytest.mark.parametrize("H", [40, 3])
@pytest.mark.parametrize("ndw,W", WIDTHS)
def test_k3_scan_is_not_skipped(oracle, ndw, W, H):
    """The scan really runs on shared-model waves: frames equal to their model give O == 0 and not one row piece for the
    row machine; the model-major list of two models has a wave that sees both (the change is at job 7, and neither 3, 4
    nor 5 jobs per wave put a wave boundary there), which hands its chunks over."""
    rs = np.random.RandomState(W + H)
    mu, sg = sc.k3_models(rs, H, W)
    mu_d = torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    models = [0] * 7 + [1] * 4
    fr = np.stack([mu[0]] * 7 + [mu[1]] * 4)
    f_d = torch.from_numpy(fr).to(DEV)
    for m in (0, 1):
        assert not oracle.posttrig_frame(mu[m], mu[m], sg[m]).any()
    for lst, budget in ((1, 512), (0, 8)):
        hip.k3_set_option("list", lst)
        hip.k3_set_option("budget", budget)
        for jobs, handed in (([(k, 0, 0, k) for k in range(7)], False), ([(7, 0, 1, 0)], False),
                             ([(k, 0, m, k) for k, m in enumerate(models)], True)):
            hist, img = hip.posttrig(f_d, mu_d, s6, hip.make_jobs(jobs, DEV), W, H)
            pieces, _ = hip.bound_counts()
            assert (pieces > 0) == handed, (jobs, lst, budget, pieces)
            assert not img.any() and (hist[:, 0] == W * H).all(), (jobs, lst, budget)


# ---- A2. K2 chained scan -------------------------------------------------------------------------------------------

def k2_chain_scene(W, H):
    """Two stacks of seven decision-boundary frames, one frame per stack differing everywhere by + 30 (the scan hands its
    rows over); stack 0 uses model 0 (sigma 0), stack 1 model 1."""
    rs = np.random.RandomState(W * 3 + H)
    F = 7
    frames, sigma = sc.decision_boundary_stack(rs, 2 * F, H, W)
    for f in (4, F + 5):
        frames[f] = np.clip(frames[f].astype(np.int64) + 30, 0, 255).astype(np.uint8)
    return F, frames, sigma


@pytest.mark.parametrize("H", [40, 17])
@pytest.mark.parametrize("ndw,W", WIDTHS)
def test_k2_chained_width_matrix(oracle, ndw, W, H):
    F, frames, sigma = k2_chain_scene(W, H)
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    for off in (1, 2):
        jobs = hip.stack_jobs(2, F, 1, F - 1, off, 2, DEV)
        jl = [tuple(int(v) for v in r) for r in jobs.cpu().numpy()]
        assert jl[F - 1] == (F + 1, F, 1, F - 1)
        Dref = np.stack([oracle.process_frame(frames[c], frames[r], sigma[m]) for (c, r, m, _) in jl])
        href = np.stack([oracle.hist256(D) for D in Dref])
        n = len(jl)
        for knobs in sc.CHAIN_KNOBS:
            key = (off, knobs)
            sc.set_chain_knobs(knobs)
            hist, _ = hip.diff_hist(f_d, s6, jobs, W, H, chain=(F - 1, off))
            assert np.array_equal(u32(hist), href), key
            hist, D = hip.diff_hist(f_d, s6, jobs, W, H, store=True, chain=(F - 1, off))
            assert np.array_equal(u32(hist), href), key
            assert np.array_equal(D.cpu().numpy(), Dref), key
            # deferred rows, completed in two instalments.  A row counts as dense from 33 suspect groups on, so at 25
            # groups per row only a full suspect list hands rows over: a small budget there
            if W // 4 <= 32:
                hip.k2_set_option("budget", 8)
            hist, state = hip.diff_hist_deferred(f_d, s6, jobs, W, H, chain=(F - 1, off))
            torch.cuda.synchronize()
            inc = state[2].cpu().numpy().astype(bool)
            assert inc.any(), key
            if H == 40 and W >= 512:  # (fewer than 33 suspect groups per row and 512 per chunk in the quiet frames)
                assert not inc.all(), key
            h = u32(hist)
            assert np.array_equal(h[~inc], href[~inc]), key          # complete jobs are final before the pieces call
            idx = np.flatnonzero(inc)
            first, rest = idx[: len(idx) // 2], idx[len(idx) // 2:]
            for part, later in ((first, rest), (rest, idx[:0])):
                before = h.copy()
                want = torch.zeros((n,), dtype=torch.uint8, device=DEV)
                want[torch.from_numpy(part).to(DEV)] = 1
                hip.diff_hist_pieces(f_d, s6, jobs, W, H, hist, state, want)
                torch.cuda.synchronize()
                h = u32(hist)
                assert np.array_equal(h[part], href[part]), key
                assert np.array_equal(h[later], before[later]), key  # not asked for yet: untouched
            assert np.array_equal(h, href), key
            hip.k2_set_option("budget", 1024)


def k2_exact_scene(ndw, W, H):
    """Two stacks of seven frames that equal their stack's base image except for a few marks, so that the chained scan
    itself decides every row (nothing is dense enough to be handed over).  A mark is a pixel e0 above base + 6 sigma with
    one e1 above right below it.  The scan bounds an output row by the vertical 1-4-6-4-1 of the group masses:
    (3, 1) gives 6 * 3 + 4 * 1 = 22, the first value it may not call zero, and D == 1 there (36 * 3 + 24 * 1 = 132 >= 128);
    (1, 3) the same one row lower; (3, 0) gives 18 and D == 0.  The marks sit on the first and on the last pixel of a
    lane, across the chunk edge (rows 15 | 16) and in the last rows; stack 0 has sigma 0, stack 1 sigma 1."""
    rs = np.random.RandomState(W * 7 + H)
    F = 7
    L = 4 * ndw
    base = rs.randint(40, 200, (2, H, W)).astype(np.int64)
    frames = np.repeat(base, F, axis=0)                       # [2 * F]: stack 0, then stack 1
    sigma = np.zeros((2, H, W), np.uint8)
    sigma[1] = 1
    half = (W // 2) // L * L
    xs = [half, half + 24 - 1, half + 48]
    marks = [(1, 5, xs[0], 3, 1), (2, 15, xs[1], 3, 1), (3, 9, xs[2], 1, 3), (5, 12, xs[0], 3, 0), (6, H - 2, xs[1], 3, 1)]
    used = []
    for s in range(2):
        for (f, y, x, e0, e1) in marks:
            if x >= W - 1 or y + 1 >= H or y < 0:
                continue
            frames[s * F + f, y, x] += 6 * s + e0
            frames[s * F + f, y + 1, x] += 6 * s + e1
            used.append((s, f, y, x, e0, e1))
        for f in range(F):                                    # a few lone excursions on both sides of the decision, far left
            k = 6
            frames[s * F + f, rs.randint(0, H, k), rs.randint(0, max(W // 4, 1), k)] += 6 * s + rs.randint(1, 7, k)
    return F, np.clip(frames, 0, 255).astype(np.uint8), sigma, used


@pytest.mark.parametrize("H", [40, 17])
@pytest.mark.parametrize("ndw,W", WIDTHS)
def test_k2_chained_scan_decides_exact_bound(oracle, ndw, W, H):
    """The decision-boundary stacks above are dense enough at these heights that the scan hands many of their chunks to
    the row machine.  Here it keeps every row: no piece is handed over, so each D == 1 pixel of the oracle was found by
    the scan's own bound, at the smallest mass it must not skip."""
    F, frames, sigma, marks = k2_exact_scene(ndw, W, H)
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    for off in (1, 2):
        jobs = hip.stack_jobs(2, F, 1, F - 1, off, 2, DEV)
        jl = [tuple(int(v) for v in r) for r in jobs.cpu().numpy()]
        Dref = np.stack([oracle.process_frame(frames[c], frames[r], sigma[m]) for (c, r, m, _) in jl])
        href = np.stack([oracle.hist256(D) for D in Dref])
        hits = 0
        for (s, f, y, x, e0, e1) in marks:
            D = Dref[s * (F - 1) + f - 1]
            if (e0, e1) == (3, 1) and y + 2 < H:
                assert D[y, x] == 1 and D[y + 1, x] == 0, (s, f, y, x)
                hits += 1
            elif (e0, e1) == (3, 0):
                assert not D[max(y - 2, 0):y + 3, x - 2:x + 3].any(), (s, f, y, x)
        assert hits >= 2
        for knobs in sc.CHAIN_KNOBS:
            key = (off, knobs)
            sc.set_chain_knobs(knobs)
            hist, _ = hip.diff_hist(f_d, s6, jobs, W, H, chain=(F - 1, off))
            torch.cuda.synchronize()
            assert hip.bound_counts()[0] == 0, key
            assert np.array_equal(u32(hist), href), key
            hist, D = hip.diff_hist(f_d, s6, jobs, W, H, store=True, chain=(F - 1, off))
            torch.cuda.synchronize()
            assert hip.bound_counts()[0] == 0, key
            assert np.array_equal(u32(hist), href), key
            assert np.array_equal(D.cpu().numpy(), Dref), key
