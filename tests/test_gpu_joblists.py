"""Job lists the pipeline never builds but the ABI allows: output slots that are a permutation of the job order, pairs
with cur == ref or ref > cur, one pair sent to two slots, chain hints that break in the middle of a block, chains of
several hundred jobs, and abub_fill_stack_jobs_dev against its documented formula.

abub_job.out is the output slot: hist, diff / img, cthr and the list slot are indexed by it, while `incomplete` and `want`
of the deferred pieces are indexed by job.  References are laid out by `out`; every comparison with the CPU oracle is
exact, and a canary row sits behind every output."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scanscenes as sc  # noqa: E402
from autobub3hs_amd import _lib, hip, host  # noqa: E402
from scanscenes import DEV, SENT, check_list, u32  # noqa: E402

SHAPES = [(1280, 48), (792, 40), (100, 40), (53, 37)]  # the last one: the generic kernel


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


def fast(W):
    return _lib.lib().abub_fast_path(W) == 1


def outputs(n, H, W, store=True):
    """hist [n + 1][256] and diff [n + 1][H][W] filled with canary bytes; the launchers get the first n slots."""
    hist = torch.full((n + 1, 256), SENT, dtype=torch.int32, device=DEV)
    diff = torch.full((n + 1, H, W), 0x5A, dtype=torch.uint8, device=DEV) if store else None
    return hist, diff


def check_out(hist, diff, href, Dref, key):
    n = len(href)
    h = u32(hist)
    assert np.array_equal(h[:n], href), key
    assert (h[n] == SENT).all(), key
    if diff is not None:
        d = diff.cpu().numpy()
        assert np.array_equal(d[:n], Dref), key
        assert (d[n] == 0x5A).all(), key


def by_out(jl, per_job):
    """Per-job references -> laid out by output slot."""
    res = np.empty_like(per_job)
    for j, (_, _, _, o) in enumerate(jl):
        res[o] = per_job[j]
    return res


def permutations(n):
    rev = list(range(n - 1, -1, -1))
    rs = np.random.RandomState(12)
    while True:
        der = [int(v) for v in rs.permutation(n)]
        if all(der[j] != j for j in range(n)):
            break
    assert all(rev[j] != j for j in range(n))
    return {"reversed": rev, "derangement": der}


def k2_refs(oracle, frames, sigma, jl):
    D = np.stack([oracle.process_frame(frames[c], frames[r], sigma[m]) for (c, r, m, _) in jl])
    return D, np.stack([oracle.hist256(d) for d in D])


# ---- B1. permuted output slots ---------------------------------------------------------------------------------------

N_PERM = 12


def perm_scene(W, H):
    """Thirteen frames for a stride-2 chain of twelve jobs: quiet ones with scattered excursions and a growing blob, one
    frame that differs everywhere (its two jobs are dense: the deferred scan hands their rows over) and one with a dense
    band inside a chunk."""
    rs = np.random.RandomState(W * 5 + H)
    frames = sc.quiet_stack(rs, N_PERM + 1, H, W, dense=(5,), band=(9, H // 2, H // 2 + 12), blob_from=6)
    sigma = np.ones((1, H, W), np.uint8)
    sigma[0, ::13, ::17] = 0
    return frames, sigma


@pytest.mark.parametrize("perm", ["reversed", "derangement"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_k2_permuted_out(oracle, W, H, perm):
    out = permutations(N_PERM)[perm]
    frames, sigma = perm_scene(W, H)
    jl = [(i, max(i - 2, 0), 0, out[i - 1]) for i in range(1, N_PERM + 1)]
    Dj, hj = k2_refs(oracle, frames, sigma, jl)
    Dref, href = by_out(jl, Dj), by_out(jl, hj)
    n = N_PERM
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    j_d = hip.make_jobs(jl, DEV)
    for bound in (0, 1):
        for lst in (0, 1):
            hip.k2_set_option("bound", bound)
            hip.k2_set_option("list", lst)
            for store in (True, False):
                hist, diff = outputs(n, H, W, store)
                hip.diff_hist(f_d, s6, j_d, W, H, store=store, hist=hist, diff=diff)
                check_out(hist, diff, href, Dref, ("plain", bound, lst, store))
    hip.k2_set_option("bound", 1)
    for lst in (0, 1):
        hip.k2_set_option("list", lst)
        for store in (True, False):
            hist, diff = outputs(n, H, W, store)
            hip.diff_hist(f_d, s6, j_d, W, H, store=store, hist=hist, diff=diff, chain=(n, 2))
            check_out(hist, diff, href, Dref, ("chained", lst, store))
    hip.k2_set_option("list", 0)
    if not fast(W):
        return
    # fused list: cthr indexed by out, list slots slot_base + out
    cthr = [3, 0, -1, 5, 2, 0, 7, -1, 1, 4, 0, 6]
    cap = int((Dref > 0).sum()) + 64
    pairs = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    hist, _ = outputs(n, H, W, False)
    c_d = torch.tensor(cthr, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_diff_hist_compact_dev(f_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H, hist.data_ptr(),
                                                     None, c_d.data_ptr(), pairs.data_ptr(), cap, count.data_ptr(), 5, _st()),
               "abub_diff_hist_compact_dev")
    torch.cuda.synchronize()
    check_out(hist, None, href, Dref, "compact")
    check_list(pairs, count, list(Dref), cthr, [5 + o for o in range(n)])


@pytest.mark.parametrize("perm", ["reversed", "derangement"])
@pytest.mark.parametrize("W,H", SHAPES[:3])
def test_k2_deferred_pieces_permuted_out(oracle, W, H, perm):
    """Deferred rows with out != job: incomplete[] and want[] speak of jobs, the histograms of slots.  The first instalment
    asks for ONE incomplete job j, so want[out[j]] == 0: its slot must still be finalised (bin 0 included), and the slot
    want[] happens to name must stay as it was."""
    out = permutations(N_PERM)[perm]
    frames, sigma = perm_scene(W, H)
    jl = [(i, max(i - 2, 0), 0, out[i - 1]) for i in range(1, N_PERM + 1)]
    _, hj = k2_refs(oracle, frames, sigma, jl)
    href = by_out(jl, hj)
    n = N_PERM
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    j_d = hip.make_jobs(jl, DEV)
    if W // 4 <= 32:  # fewer groups per row than a dense row needs: only a full suspect list hands rows over
        hip.k2_set_option("budget", 128)
    hist, state = hip.diff_hist_deferred(f_d, s6, j_d, W, H, chain=(n, 2))
    torch.cuda.synchronize()
    inc = state[2].cpu().numpy().astype(bool)          # by job
    assert inc.any() and not inc.all()
    slots = np.array(out)
    h = u32(hist)
    done = slots[~inc]
    assert np.array_equal(h[done], href[done])         # complete jobs: final, in their slots
    idx = np.flatnonzero(inc)
    for k, part in enumerate((idx[:1], idx[1:])):
        if not len(part):
            continue
        want = np.zeros(n, np.uint8)
        want[part] = 1
        if k == 0:
            assert not want[slots[part]].any()          # the slot index of the requested job is not a requested job
        before = h.copy()
        hip.diff_hist_pieces(f_d, s6, j_d, W, H, hist, state, torch.from_numpy(want).to(DEV))
        torch.cuda.synchronize()
        h = u32(hist)
        for j in part:
            o = slots[j]
            assert h[o].sum() == W * H, (j, o, int(h[o].sum()), W * H, int(h[o, 0]), int(href[o, 0]))
            assert np.array_equal(h[o], href[o]), (j, o)
        others = np.setdiff1d(np.arange(n), slots[part])
        assert np.array_equal(h[others], before[others])
    assert np.array_equal(h, href)


@pytest.mark.parametrize("perm", ["reversed", "derangement"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_k3_and_pair_hist_permuted_out(oracle, W, H, perm):
    out = permutations(N_PERM)[perm]
    n = N_PERM
    rs = np.random.RandomState(W * 9 + H)
    mu, sg = sc.k3_models(rs, H, W)
    ndw = next((d for d in range(1, 9) if (W // 4) % d == 0 and (W // 4) // d <= 64), 1) if W % 4 == 0 else 1
    fr = sc.k3_scan_frames(rs, mu, sg, [0] * n, ndw)
    jl = [(k, 0, 0, out[k]) for k in range(n)]
    Oj = np.stack([oracle.posttrig_frame(fr[c], mu[0], sg[0]) for (c, _, _, _) in jl])
    Oref = by_out(jl, Oj)
    href = np.stack([oracle.hist256(o) for o in Oref])
    f_d, mu_d = torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sg).to(DEV))
    j_d = hip.make_jobs(jl, DEV)
    L = _lib.lib()
    cthr = [3, 0, -1, 5, 2, 0, 7, -1, 1, 4, 0, 6]
    c_d = torch.tensor(cthr, dtype=torch.int32, device=DEV)
    cap = int((Oref > 0).sum()) + 64
    for scan in (0, 1):
        for lst in (0, 1):
            hip.k3_set_option("scan", scan)
            hip.k3_set_option("list", lst)
            hist, img = outputs(n, H, W)
            _lib.check(L.abub_posttrig_dev(f_d.data_ptr(), mu_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H,
                                           hist.data_ptr(), img.data_ptr(), _st()), "abub_posttrig_dev")
            check_out(hist, img, href, Oref, ("k3", scan, lst))
            if not fast(W):
                continue
            pairs = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
            count = torch.zeros((1,), dtype=torch.int32, device=DEV)
            hist, _ = outputs(n, H, W, False)
            _lib.check(L.abub_posttrig_compact_dev(f_d.data_ptr(), mu_d.data_ptr(), s6.data_ptr(), j_d.data_ptr(), n, W, H,
                                                   hist.data_ptr(), None, c_d.data_ptr(), pairs.data_ptr(), cap,
                                                   count.data_ptr(), 7, _st()), "abub_posttrig_compact_dev")
            torch.cuda.synchronize()
            check_out(hist, None, href, Oref, ("k3 compact", scan, lst))
            check_list(pairs, count, list(Oref), cthr, [7 + o for o in range(n)])
    # pair histograms: sat(f1 - f0)
    pl = [(int(rs.randint(n)), int(rs.randint(n)), 0, out[k]) for k in range(n)]
    hist, _ = outputs(n, H, W, False)
    _lib.check(L.abub_pair_hist_dev(f_d.data_ptr(), hip.make_jobs(pl, DEV).data_ptr(), n, W, H, hist.data_ptr(), _st()),
               "abub_pair_hist_dev")
    pj = np.stack([oracle.hist256(np.clip(fr[a].astype(int) - fr[b].astype(int), 0, 255).astype(np.uint8)) for (a, b, _, _) in pl])
    check_out(hist, None, by_out(pl, pj), None, "pair_hist")


# ---- B2. pair shapes and chains that break in the middle ------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_k2_pair_shapes_and_broken_chains(oracle, W, H):
    F = 9
    rs = np.random.RandomState(W + 11 * H)
    frames = sc.quiet_stack(rs, 2 * F, H, W, dense=(F + 3,), blob_from=4)
    sigma = np.ones((2, H, W), np.uint8)
    sigma[1, ::3, ::2] = 2
    jl = [tuple(int(v) for v in r) for r in hip.stack_jobs(2, F, 1, F - 1, 2, 2, DEV).cpu().numpy()]
    assert jl[0] == (1, 0, 0, 0) and jl[8] == (F + 1, F, 1, 8) and len(jl) == 16
    jl[2] = (3, 3, 0, 2)                 # cur == ref
    jl[4] = (5, 7, 0, 4)                 # ref > cur
    jl[6] = (jl[5][0], jl[5][1], 0, 6)   # the pair of job 5 once more
    jl[10] = (F + 3, 2, 1, 10)           # ref points elsewhere in the middle of a chain
    jl[12] = (F + 5, F + 3, 0, 12)       # another model in the middle of a chain
    jl[14] = (2 * F - 1, 2 * F - 1, 1, 14)   # short-stack tail: cur == ref == last frame
    jl[15] = (2 * F - 1, 2 * F - 1, 1, 15)
    Dref, href = k2_refs(oracle, frames, sigma, jl)
    for j in (2, 14, 15):
        assert not Dref[j].any()
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    j_d = hip.make_jobs(jl, DEV)
    n = len(jl)
    for knobs in sc.CHAIN_KNOBS:
        sc.set_chain_knobs(knobs)
        for store in (False, True):
            hist, diff = outputs(n, H, W, store)
            hip.diff_hist(f_d, s6, j_d, W, H, store=store, hist=hist, diff=diff, chain=(F - 1, 2))
            check_out(hist, diff, href, Dref, (knobs, store))
            for j in (2, 14, 15):
                assert int(hist[j, 0]) == W * H, (knobs, store, j)
                if store:
                    assert not diff[j].any(), (knobs, j)


# ---- B3. long chains -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nst", [1, 2])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_k2_long_chains(oracle, stride, nst):
    """Chains of 257 jobs (more than any workgroup of the chained scan covers, and more than 256): every residue chain is
    cut into many segments of 2 or 4 jobs, over workgroups of 1, 3 and 8 waves."""
    W, H, F = 256, 24, 258
    L = F - 1
    rs = np.random.RandomState(stride * 7 + nst)
    frames = np.concatenate([sc.quiet_stack(rs, F, H, W, dense=(200 + s,), blob_from=F // 2) for s in range(nst)])
    sigma = np.ones((1, H, W), np.uint8)
    jobs = hip.stack_jobs(nst, F, 1, L, stride, 1, DEV)
    jl = [tuple(int(v) for v in r) for r in jobs.cpu().numpy()]
    Dref, href = k2_refs(oracle, frames, sigma, jl)
    assert int(href[200 - 1, 1:].sum()) > W * H // 2   # the dense frame
    f_d = torch.from_numpy(frames).to(DEV)
    s6 = hip.sigma6(torch.from_numpy(sigma).to(DEV))
    n = len(jl)
    for chain, wg in ((4, 8), (2, 3), (-1, -1)):
        hip.k2_set_option("chain", chain)
        hip.k2_set_option("wg", wg)
        for hint in sorted({(L, stride), (n, stride)}):
            for store in (False, True):
                hist, diff = outputs(n, H, W, store)
                hip.diff_hist(f_d, s6, jobs, W, H, store=store, hist=hist, diff=diff, chain=hint)
                check_out(hist, diff, href, Dref, (chain, wg, hint, store))


# ---- B4. abub_fill_stack_jobs_dev ------------------------------------------------------------------------------------

@pytest.mark.parametrize("past", [0, 1, "F + 3"])
def test_fill_stack_jobs_formula(past):
    """cur = s*F + i, ref = s*F + max(i - ref_offset, 0), model = s % nmodels, out = s*count + (i - first) for stack s and
    i in [first, first + count); first = 0, a ref_offset beyond the stack (F + 3), three models over five stacks, more jobs
    than one block fills."""
    F, nst, nmodels = 11, 5, 3
    ref_offset = F + 3 if past == "F + 3" else past
    for first, count in ((0, F), (0, 7), (3, 8)):
        got = hip.stack_jobs(nst, F, first, count, ref_offset, nmodels, DEV).cpu().numpy()
        exp = [(s * F + i, s * F + max(i - ref_offset, 0), s % nmodels, s * count + (i - first))
               for s in range(nst) for i in range(first, first + count)]
        assert np.array_equal(got, np.array(exp)), (first, count)
    F, nst = 70, 5                                    # 350 jobs: two blocks of 256 threads
    ref_offset = F + 3 if past == "F + 3" else past
    got = hip.stack_jobs(nst, F, 0, F, ref_offset, nmodels, DEV).cpu().numpy()
    exp = [(s * F + i, s * F + max(i - ref_offset, 0), s % nmodels, s * F + i) for s in range(nst) for i in range(F)]
    assert len(exp) > 256 and np.array_equal(got, np.array(exp))


def test_fill_stack_jobs_empty():
    """nstacks = 0 or count = 0: OK, and nothing is written."""
    buf = torch.full((8, 4), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    for nst, count in ((0, 5), (3, 0), (0, 0)):
        assert L.abub_fill_stack_jobs_dev(buf.data_ptr(), nst, 9, 0, count, 2, 1, _st()) == 0
    torch.cuda.synchronize()
    assert (buf == 0x5A5A5A5A).all()
