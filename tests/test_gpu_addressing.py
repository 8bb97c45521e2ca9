"""Frames and output slots beyond 4 GiB.

W x H = 2048 x 1024 makes a frame 2^21 bytes, so frame 2048 starts at byte 2^32 and, under a 32-bit wrap of the byte
offset, frame (or slot) 2048 + k aliases k.  Frames 0 .. 3 and 2048 .. 2051 of one slab hold different content: a wrapped
read or write stays inside the same allocation and shows up as a wrong value.  Reference: the CPU oracle, exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib, hip, host  # noqa: E402
from scanscenes import DEV, u32  # noqa: E402

W, H = 2048, 1024
P = W * H
HI = 2048            # first frame / slot past 4 GiB
NF = HI + 4
NEED = 12 << 30      # slab 4 GiB + stored images 4 GiB + room for the rest


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


@pytest.fixture(scope="module")
def scene():
    """slab [2052][H][W] on the device with frames 0 .. 3 and 2048 .. 2051 filled; host copies of those eight frames
    (index k and 4 + k), a model whose mu is frame 0, and a one-slot-per-job output image shared by the tests."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("needs 12 GiB of free device memory")
    assert P == 1 << 21 and HI * P == 1 << 32
    rs = np.random.RandomState(2048)
    base = rs.randint(50, 180, (H, W)).astype(np.int64)
    yy, xx = np.ogrid[:H, :W]
    host_fr = np.empty((8, H, W), np.uint8)
    for k in range(8):
        f = base + rs.randint(-2, 3, (H, W))
        cx, cy, r = 150 + 230 * k, 90 + 110 * k, 12 + 3 * k   # a blob of its own in every frame
        f[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] += 45 + k
        n = 400
        f[rs.randint(0, H, n), rs.randint(0, W, n)] += rs.randint(5, 14, n)
        host_fr[k] = np.clip(f, 0, 255)
    slab = torch.empty((NF, H, W), dtype=torch.uint8, device=DEV)
    slab[0:4] = torch.from_numpy(host_fr[0:4]).to(DEV)
    slab[HI:HI + 4] = torch.from_numpy(host_fr[4:8]).to(DEV)
    mu = host_fr[0:1].copy()
    sigma = np.ones((1, H, W), np.uint8)
    sigma[0, ::37, ::29] = 0
    out = torch.empty((NF, H, W), dtype=torch.uint8, device=DEV)
    d = {"slab": slab, "fr": host_fr, "mu": mu, "sigma": sigma, "out": out,
         "mu_d": torch.from_numpy(mu).to(DEV), "s6": hip.sigma6(torch.from_numpy(sigma).to(DEV))}
    yield d
    d.clear()
    del slab, out
    torch.cuda.empty_cache()


def hostf(scene, i):
    """Host copy of slab frame i (0 .. 3 or 2048 .. 2051)."""
    return scene["fr"][i if i < 4 else 4 + i - HI]


PAIRS = [(HI + 2, HI), (HI + 3, HI + 1), (HI + 1, 1)]


@pytest.fixture(scope="module")
def k2_ref(oracle, scene):
    D = np.stack([oracle.process_frame(hostf(scene, c), hostf(scene, r), scene["sigma"][0]) for (c, r) in PAIRS])
    h = np.stack([oracle.hist256(d) for d in D])
    assert all(d.any() for d in D)
    # what a wrapped frame index would give differs
    assert not np.array_equal(D[0], oracle.process_frame(hostf(scene, 2), hostf(scene, 0), scene["sigma"][0]))
    return D, h


@pytest.fixture(scope="module")
def k3_ref(oracle, scene):
    O = np.stack([oracle.posttrig_frame(hostf(scene, HI + k), scene["mu"][0], scene["sigma"][0]) for k in range(4)])
    assert all(o.any() for o in O)
    return O, np.stack([oracle.hist256(o) for o in O])


def test_k2_reads_frames_past_4gib(scene, k2_ref):
    Dref, href = k2_ref
    jobs = hip.make_jobs([(c, r, 0, k) for k, (c, r) in enumerate(PAIRS)], DEV)
    for bound in (0, 1):
        hip.k2_set_option("bound", bound)
        hist, D = hip.diff_hist(scene["slab"], scene["s6"], jobs, W, H, store=True)
        assert np.array_equal(u32(hist), href), bound
        assert np.array_equal(D.cpu().numpy(), Dref), bound
        hist, _ = hip.diff_hist(scene["slab"], scene["s6"], jobs, W, H, store=False)
        assert np.array_equal(u32(hist), href), bound
    for store in (False, True):
        hist, D = hip.diff_hist(scene["slab"], scene["s6"], jobs, W, H, store=store, chain=(3, 1))
        assert np.array_equal(u32(hist), href), store
        if store:
            assert np.array_equal(D.cpu().numpy(), Dref)


def test_k2_chain_past_4gib(oracle, scene):
    """A chain that really has the hinted structure up there: job q refs the cur frame of job q - 1."""
    cl = [(HI + 1 + q, HI + q, 0, q) for q in range(3)]
    Dref = np.stack([oracle.process_frame(hostf(scene, c), hostf(scene, r), scene["sigma"][0]) for (c, r, _, _) in cl])
    href = np.stack([oracle.hist256(d) for d in Dref])
    jobs = hip.make_jobs(cl, DEV)
    for store in (False, True):
        hist, D = hip.diff_hist(scene["slab"], scene["s6"], jobs, W, H, store=store, chain=(3, 1))
        assert np.array_equal(u32(hist), href), store
        if store:
            assert np.array_equal(D.cpu().numpy(), Dref)


def test_k3_reads_frames_past_4gib(scene, k3_ref):
    Oref, href = k3_ref
    jobs = hip.make_jobs([(HI + k, 0, 0, k) for k in range(4)], DEV)
    for scan in (1, 0):
        hip.k3_set_option("scan", scan)
        hist, img = hip.posttrig(scene["slab"], scene["mu_d"], scene["s6"], jobs, W, H)
        assert np.array_equal(u32(hist), href), scan
        assert np.array_equal(img.cpu().numpy(), Oref), scan
        hist, _ = hip.posttrig(scene["slab"], scene["mu_d"], scene["s6"], jobs, W, H, store=False)
        assert np.array_equal(u32(hist), href), scan


def test_train_and_pair_hist_past_4gib(oracle, scene):
    idx = torch.arange(HI, HI + 4, dtype=torch.int32, device=DEV)
    mu, sg = hip.train(scene["slab"], W, H, idx=idx)
    mu_r, sg_r = oracle.welford(scene["fr"][4:8])
    assert np.array_equal(mu.cpu().numpy(), mu_r) and np.array_equal(sg.cpu().numpy(), sg_r)
    mu_w, _ = oracle.welford(scene["fr"][0:4])
    assert not np.array_equal(mu_r, mu_w)
    pl = [(c, r, 0, k) for k, (c, r) in enumerate(PAIRS + [(1, HI + 1)])]
    h = u32(hip.pair_hist(scene["slab"], hip.make_jobs(pl, DEV), W, H))
    for (c, r, _, o) in pl:
        d = np.clip(hostf(scene, c).astype(int) - hostf(scene, r).astype(int), 0, 255).astype(np.uint8)
        assert np.array_equal(h[o], oracle.hist256(d)), (c, r)


def out_jobs(real):
    """2048 jobs (0, 0, 0, j) whose image is zero, then the real ones in slots 2048 .. 2051."""
    jl = [(0, 0, 0, j) for j in range(HI)] + [(c, r, 0, HI + k) for k, (c, r) in enumerate(real)]
    return hip.make_jobs(jl, DEV)


def check_low_slots(hist, img):
    assert not bool(img[:HI].any())
    assert bool((hist[:HI, 0] == P).all()) and not bool(hist[:HI, 1:].any())


def test_k2_writes_slots_past_4gib(oracle, scene, k2_ref):
    D3, h3 = k2_ref
    real = PAIRS + [(HI + 3, HI + 2)]
    D4 = oracle.process_frame(hostf(scene, HI + 3), hostf(scene, HI + 2), scene["sigma"][0])
    Dref = np.concatenate([D3, D4[None]])
    href = np.concatenate([h3, oracle.hist256(D4)[None]])
    jobs = out_jobs(real)
    for bound in (0, 1):
        hip.k2_set_option("bound", bound)
        scene["out"][:4].fill_(0x5A)     # where a wrapped slot would land
        scene["out"][HI:].fill_(0x5A)
        hist, img = hip.diff_hist(scene["slab"], scene["s6"], jobs, W, H, store=True, diff=scene["out"])
        torch.cuda.synchronize()
        assert np.array_equal(u32(hist[HI:]), href), bound
        assert np.array_equal(img[HI:].cpu().numpy(), Dref), bound
        check_low_slots(hist, img)


def test_k3_writes_slots_past_4gib(scene, k3_ref):
    Oref, href = k3_ref
    # mu is frame 0, so the 2048 jobs on frame 0 give O == 0
    jl = [(0, 0, 0, j) for j in range(HI)] + [(HI + k, 0, 0, HI + k) for k in range(4)]
    jobs = hip.make_jobs(jl, DEV)
    scene["out"][:4].fill_(0x5A)
    scene["out"][HI:].fill_(0x5A)
    hist = torch.empty((NF, 256), dtype=torch.int32, device=DEV)
    img = scene["out"]
    _lib.check(_lib.lib().abub_posttrig_dev(scene["slab"].data_ptr(), scene["mu_d"].data_ptr(), scene["s6"].data_ptr(),
                                            jobs.data_ptr(), NF, W, H, hist.data_ptr(), img.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "abub_posttrig_dev")
    torch.cuda.synchronize()
    assert np.array_equal(u32(hist[HI:]), href)
    assert np.array_equal(img[HI:].cpu().numpy(), Oref)
    check_low_slots(hist, img)
