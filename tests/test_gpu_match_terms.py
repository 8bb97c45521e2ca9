"""Both term kernels of the bellows matcher (abub_match_ccorr_batch_dev: k_match_num + k_match_wsum2, and the per-event
abub_match_ccorr_dev) against the numpy definition (tests/matchref.py), bit for bit in u64, at the seams of k_match_num's
paths -- the template-row split and its atomics, the u32 -> u64 flush, the LDS template chunks -- at ragged plane ends, at
every segment width of k_match_wsum2, and at the limits the entries enforce."""
import ctypes as C

import numpy as np
import pytest

import matchref
from matchref import match_chunks, match_geometry

from autobub3hs_amd import _lib

INVALID = -1  # ABUB_E_INVALID
MR = 8        # output rows per wave of k_match_num: a template chunk shorter than this never takes the full-row path

# (W, H, tw, th, njobs) -> the path it must take: nsplit, rsplit, and whichever of nc, rc, ybl, rw, rh the case is about
NAMED = [
    ((96, 100, 9, 64, 1), dict(nsplit=2, rsplit=32, chunks=1)),             # the split alone
    ((40, 150, 5, 129, 1), dict(nsplit=4, rsplit=33, last=30)),             # an uneven last split
    ((64, 200, 8, 130, 2), dict(nsplit=4, rsplit=33, ybl=3)),               # two jobs: the per-job memset region, atomics
    ((333, 100, 300, 64, 1), dict(nsplit=2, nc=76, rc=13, chunks=3)),       # full-row and partial-row path per split
    ((600, 80, 520, 33, 1), dict(nsplit=1, nc=131, rc=7, chunks=5, ybl=2)),  # every chunk shorter than MR
    ((4096, 70, 4000, 64, 1), dict(nsplit=2, rsplit=32, flush=16, rc=1)),   # split with flush; sums past 2^32
    ((4096, 24, 4093, 20, 1), dict(nsplit=1, nc=1024, rc=1)),               # nc == MTPL: the widest template admitted
    ((300, 40, 40, 9, 3), dict(nsplit=1, rw=261, rh=32)),                   # two x blocks, rw % 4 == 1, rh == 32
    ((523, 75, 7, 3, 2), dict(nsplit=1, rw=517, rh=73, ybl=3)),             # odd W: unaligned words throughout
    ((4, 66051, 1, 66051, 1), dict(rw=4, rh=1)),                            # the tallest template the u32 column sums hold
]


def geometry(W, H, tw, th, njobs):
    nsplit, rsplit, flush = match_geometry(W, H, tw, th, njobs)
    nc, rc = match_chunks(tw)
    rw, rh = W - tw + 1, H - th + 1
    return dict(nsplit=nsplit, rsplit=rsplit, flush=flush, nc=nc, rc=rc, rw=rw, rh=rh, ybl=(rh + 31) // 32,
                chunks=(min(rsplit, th) + rc - 1) // rc, last=th - (nsplit - 1) * rsplit)


def test_named_shapes_take_the_paths_they_name():
    for shape, want in NAMED:
        g = geometry(*shape)
        assert {k: g[k] for k in want} == want, (shape, g)
    g = geometry(4096, 70, 4000, 64, 1)
    assert g["nsplit"] > 1 and g["rsplit"] > g["flush"]            # the split combined with the flush
    assert 65025 * 4000 * 64 > 1 << 32                              # past u32 in num and in the wsum2 prefix
    g = geometry(333, 100, 300, 64, 1)
    assert g["rc"] > MR and g["rsplit"] % g["rc"] < MR              # a long chunk (both paths) and a short last one
    assert geometry(600, 80, 520, 33, 1)["rc"] < MR
    assert matchref.TH_MAX * 65025 < 1 << 32 <= (matchref.TH_MAX + 1) * 65025


def runs_frame(rng, H, W):
    """A random frame with runs of 0 and of 255 of random lengths along the raster"""
    f = rng.randint(0, 256, H * W).astype(np.uint8)
    p = 0
    while p < f.size:
        n = int(rng.randint(1, 40))
        kind = rng.randint(0, 4)
        if kind < 2:
            f[p:p + n] = 0 if kind == 0 else 255
        p += n
    return f.reshape(H, W)


def slab_of(rng, H, W):
    """[random, saturated, runs, random]"""
    return np.stack([rng.randint(0, 256, (H, W)).astype(np.uint8), np.full((H, W), 255, np.uint8), runs_frame(rng, H, W),
                     rng.randint(0, 256, (H, W)).astype(np.uint8)])


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class Checker:
    """One slab on the device; every job of every call compared with the reference of its frame (computed once)."""

    def __init__(self, slab, odd_offset=False):
        import torch

        self.slab = slab
        self.dev = "cuda:0"
        if odd_offset:  # the slab at an odd byte offset of a larger tensor
            big = torch.zeros(slab.size + 64, dtype=torch.uint8, device=self.dev)
            big[13:13 + slab.size] = torch.from_numpy(slab.reshape(-1)).to(self.dev)
            self.d_slab = big[13:13 + slab.size].view(slab.shape)
            assert self.d_slab.data_ptr() % 2 == 1 and self.d_slab.is_contiguous()
        else:
            self.d_slab = torch.from_numpy(slab).to(self.dev)
        self.ref = {}

    def reference(self, f, tmpl, key):
        if (f, key) not in self.ref:
            self.ref[(f, key)] = matchref.terms(self.slab[f], tmpl)
        return self.ref[(f, key)]

    def batch(self, idx, tmpl, key):
        import torch

        from autobub3hs_amd import hip

        assert max(idx) < len(self.slab) and min(idx) >= 0  # every index stays inside the slab
        H, W = self.slab.shape[1:]
        th, tw = tmpl.shape
        out = [torch.full((len(idx), H - th + 1, W - tw + 1), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=self.dev)
               for _ in range(2)]  # garbage where the sums go: the split path adds into num
        num, w2 = hip.match_terms(self.d_slab, torch.tensor(idx, dtype=torch.int32, device=self.dev),
                                  torch.from_numpy(tmpl).to(self.dev), out=out)
        num, w2 = _u64(num), _u64(w2)
        for k, f in enumerate(idx):
            en, ew = self.reference(f, tmpl, key)
            assert np.array_equal(num[k], en), ("num", self.slab.shape, tmpl.shape, idx, k)
            assert np.array_equal(w2[k], ew), ("wsum2", self.slab.shape, tmpl.shape, idx, k)
        return num, w2

    def per_event(self, f, tmpl, key):
        import torch

        H, W = self.slab.shape[1:]
        th, tw = tmpl.shape
        num = torch.full((H - th + 1, W - tw + 1), -1, dtype=torch.int64, device=self.dev)
        w2 = torch.full_like(num, -1)
        t_d = torch.from_numpy(tmpl).to(self.dev)
        _lib.check(_lib.lib().abub_match_ccorr_dev(self.d_slab[f].data_ptr(), W, H, t_d.data_ptr(), tw, th, num.data_ptr(),
                                                   w2.data_ptr(), torch.cuda.current_stream().cuda_stream))
        en, ew = self.reference(f, tmpl, key)
        assert np.array_equal(_u64(num), en), ("per-event num", self.slab.shape, tmpl.shape, f)
        assert np.array_equal(_u64(w2), ew), ("per-event wsum2", self.slab.shape, tmpl.shape, f)


# frame_idx per call: repeats frames, is not sorted, does not start at 0 (a single job takes each frame in turn)
CALLS = {1: ([[3], [2]], [[1]]), 2: ([[3, 2], [2, 2]], [[1, 1]]), 3: ([[2, 0, 2], [3, 1, 3]], [[1, 3, 1]])}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s, _ in NAMED], ids=["%dx%d_t%dx%d_j%d" % s for s, _ in NAMED])
def test_named_shape_exact(shape):
    W, H, tw, th, njobs = shape
    want = dict(NAMED)[shape]
    g = geometry(*shape)
    assert {k: g[k] for k in want} == want, g  # a change to match_geom fails here, not by testing something else
    rng = np.random.RandomState(W * 31 + th)
    ck = Checker(slab_of(rng, H, W))
    tmpl = rng.randint(0, 256, (th, tw)).astype(np.uint8)
    sat = np.full((th, tw), 255, np.uint8)
    plain, saturated = CALLS[njobs]
    for idx in plain:
        ck.batch(idx, tmpl, "rnd")
    for idx in saturated:
        num, w2 = ck.batch(idx, sat, "sat")
        for k, f in enumerate(idx):
            if f == 1:  # the closed form in every placement
                assert (num[k] == 65025 * tw * th).all() and (w2[k] == 65025 * tw * th).all(), (shape, k)
    if njobs == 1:  # the per-event kernel on the same frames
        for f in (3, 2):
            ck.per_event(f, tmpl, "rnd")
        ck.per_event(1, sat, "sat")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(523, 75, 7, 3, 2), (64, 200, 8, 130, 2), (300, 40, 40, 9, 3)],
                         ids=lambda s: "%dx%d_t%dx%d_j%d" % s)
def test_slab_at_an_odd_byte_offset(shape):
    W, H, tw, th, njobs = shape
    rng = np.random.RandomState(W + 7)
    ck = Checker(slab_of(rng, H, W), odd_offset=True)
    tmpl = rng.randint(0, 256, (th, tw)).astype(np.uint8)
    ck.batch([3, 0, 2][:njobs] if njobs == 3 else [3, 2], tmpl, "rnd")
    ck.batch([3] * njobs, tmpl, "rnd")  # the slab's last frame: ld4's byte tail at the slab's last bytes


def sweep(shapes, idx=(2, 0, 1, 2)):
    for W, H, tw, th in shapes:
        rng = np.random.RandomState(W * 7 + H * 3 + tw)
        ck = Checker(slab_of(rng, H, W)[:3])
        tmpl = rng.randint(0, 256, (th, tw)).astype(np.uint8)
        tmpl[rng.randint(0, th), rng.randint(0, tw)] = 255
        ck.batch(list(idx), tmpl, "rnd")
        ck.per_event(2, tmpl, "rnd")


@pytest.mark.gpu
def test_sweep_template_width_residues():
    """tw % 4 in all four residues (nc = (tw + 2) / 4 + 1), tw == W, th == H, both (a 1 x 1 plane), and th == 1"""
    assert [match_chunks(tw)[0] for tw in range(1, 10)] == [1, 2, 2, 2, 2, 3, 3, 3, 3]
    sweep([(37, 20, tw, 5) for tw in range(1, 10)])
    sweep([(37, 20, 37, 5), (37, 20, 6, 20), (37, 20, 37, 20), (37, 20, 5, 1), (37, 20, 1, 1), (1, 1, 1, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [255, 256, 257, 511, 513, 4095, 4096])
def test_sweep_wsum2_segment_widths(W):
    """seg = ceil(W / 256) changes at these widths; rh in 1, 7, 8, 9, 17: one row, a ragged block, one block exactly, one
    row into the second block (the sliding column update carried over), three blocks"""
    assert (W + 255) // 256 == {255: 1, 256: 1, 257: 2, 511: 2, 513: 3, 4095: 16, 4096: 16}[W]
    sweep([(W, rh + 3, 3, 4) for rh in (1, 7, 8, 9, 17)])


@pytest.mark.gpu
def test_sweep_plane_heights_around_a_block():
    """rh in 31, 32, 33 at W = 21: the last wave full, and one row into a second workgroup whose other waves have y0 >= rh"""
    sweep([(21, rh + 4, 4, 5) for rh in (31, 32, 33)])


# ---- refusals ------------------------------------------------------------------------------------------------------------

REFUSED = [
    (4, 66052, 1, 66052, 1),    # th = 66052: the u32 column sums of k_match_wsum2 overflow on a saturated frame
    (4096, 24, 4094, 20, 1),    # nc = 1025 > MTPL
    (4097, 8, 3, 3, 1),         # W > 4096
    (8, 8, 8, 8, 0),            # njobs = 0
    (8, 8, 8, 8, 65536),        # njobs = 65536
    (16, 8, 17, 3, 1),          # tw > W
    (16, 8, 3, 9, 1),           # th > H
]
ADMITTED = [(4, 66051, 1, 66051, 1), (4096, 24, 4093, 20, 1), (4096, 8, 3, 3, 1), (8, 8, 8, 8, 65535), (16, 8, 16, 8, 1)]


def test_scratch_bytes_is_zero_where_the_entries_refuse():
    L = _lib.lib()
    for case in REFUSED:
        assert L.abub_match_best_scratch_bytes(*case) == 0, case
    for case in ADMITTED:
        assert L.abub_match_best_scratch_bytes(*case) > 0, case
    # placement indices are u32 with 0xffffffff for "none": rw * rh >= 2^32 - 1 is refused
    assert L.abub_match_best_scratch_bytes(4096, 1 << 20, 1, 1, 1) == 0
    assert L.abub_match_best_scratch_bytes(4096, (1 << 20) - 1, 1, 1, 1) > 0


def test_too_many_placements_refused_before_the_device():
    L = _lib.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: refused up front
    assert L.abub_match_ccorr_batch_dev(fake, 4096, 1 << 20, fake, 1, fake, 1, 1, fake, fake, None) == INVALID
    assert L.abub_match_best_batch_dev(fake, 4096, 1 << 20, fake, 1, fake, 1, 1, fake, fake, 1 << 40, None) == INVALID
    assert b"bad arguments" in L.abub_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%dx%d_t%dx%d_j%d" % c)
def test_refused_before_any_launch(case):
    """ABUB_E_INVALID, and not a byte of the outputs written.  Every buffer has the size a launch would need."""
    import torch

    W, H, tw, th, njobs = case
    dev = "cuda:0"
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n = max(njobs, 1) * max(W - tw + 1, 1) * max(H - th + 1, 1)
    frames = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    tmpl = torch.full((th, tw), 255, dtype=torch.uint8, device=dev)
    fidx = torch.zeros(max(njobs, 1), dtype=torch.int32, device=dev)
    num = torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    w2 = num.clone()
    rc = L.abub_match_ccorr_batch_dev(frames.data_ptr(), W, H, fidx.data_ptr(), njobs, tmpl.data_ptr(), tw, th, num.data_ptr(),
                                      w2.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == INVALID, (case, rc)
    assert b"bad arguments" in L.abub_last_error()
    assert bool((num == 0x5A5A5A5A5A5A5A5A).all()) and bool((w2 == 0x5A5A5A5A5A5A5A5A).all())
    assert L.abub_match_best_scratch_bytes(*case) == 0
    scratch = torch.full((28 * n + 4096,), 0x5A, dtype=torch.uint8, device=dev)  # what the admitted layout would take
    xy = torch.full((2 * max(njobs, 1),), 7.5, dtype=torch.float32, device=dev)
    assert scratch.data_ptr() % 256 == 0
    rc = L.abub_match_best_batch_dev(frames.data_ptr(), W, H, fidx.data_ptr(), njobs, tmpl.data_ptr(), tw, th, xy.data_ptr(),
                                     scratch.data_ptr(), scratch.numel(), st)
    torch.cuda.synchronize()
    assert rc == INVALID, (case, rc)
    assert bool((scratch == 0x5A).all()) and bool((xy == 7.5).all())


@pytest.mark.gpu
def test_tallest_template_admitted_and_exact_when_saturated():
    """th = 66051 on a saturated frame: wsum2 == 66051 * 65025 = 4 294 966 275, the largest column sum a u32 holds"""
    import torch

    from autobub3hs_amd import hip

    dev = "cuda:0"
    W, H, tw, th = 4, matchref.TH_MAX, 1, matchref.TH_MAX
    frames = torch.full((1, H, W), 255, dtype=torch.uint8, device=dev)
    num, w2 = hip.match_terms(frames, torch.zeros(1, dtype=torch.int32, device=dev),
                              torch.full((th, tw), 255, dtype=torch.uint8, device=dev))
    assert _u64(w2).tolist() == [[[66051 * 65025] * 4]] and _u64(num).tolist() == [[[66051 * 65025] * 4]]
    assert 66051 * 65025 == 4294966275 < 1 << 32
