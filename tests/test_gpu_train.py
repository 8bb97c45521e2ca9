"""K1 (abub_train_dev: k1_welford, k1_welford4) against the CPU oracle, byte for byte, where float parity can slip.

The inputs are the designed pixels of tests/trainref.py: tests/test_train_ref.py shows, with a numpy restatement alone,
that hundreds of them change a byte when the m2 update is contracted to a fused multiply-add or the divide becomes a
multiplication by a reciprocal, and thousands when a divide or sqrt lands one float low.  So a pass here says that this
build rounds as the reference does; a pass on random frames would not.  Around that: every form of `idx`, the plane
sizes round the block and dword boundaries with canaries round the outputs, any byte address for frames, mu and sigma
(the dword kernel is taken only for aligned ones, include/abub_hip.h), degenerate N, and the same through
abub_ctx_train on both sides of max_frames."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib  # noqa: E402

import trainref  # noqa: E402
from ctxapi import OK, Ctx  # noqa: E402

DEV = "cuda:0"
CAN = 0xC3  # canary byte
PAD = 64    # canary bytes behind every buffer


@pytest.fixture(scope="module")
def groups():
    return trainref.designed()


def dev_at(a, off):
    """`a` at byte offset `off` of a canary-filled device buffer -> (buffer, view of the copy)."""
    buf = torch.full((off + a.size + PAD,), CAN, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return buf, view


def canaries_intact(buf, off, n):
    b = buf.cpu().numpy()
    return (b[:off] == CAN).all() and (b[off + n:] == CAN).all()


def train(st, idx=None, N=None, off=(0, 4, 4)):
    """abub_train_dev on st [F, H, W]; frames, mu and sigma at byte offsets `off` of 16-byte aligned canary buffers.
    idx: None or an int32 device tensor (any view).  Every byte round mu and sigma must keep its value."""
    F, H, W = st.shape
    P = H * W
    fbuf, f_d = dev_at(st, off[0])
    mbuf = torch.full((off[1] + P + PAD,), CAN, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((off[2] + P + PAD,), CAN, dtype=torch.uint8, device=DEV)
    assert mbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    if N is None:
        N = F if idx is None else idx.numel()
    _lib.check(_lib.lib().abub_train_dev(f_d.data_ptr(), None if idx is None else idx.data_ptr(), N, W, H,
                                         mbuf.data_ptr() + off[1], sbuf.data_ptr() + off[2],
                                         torch.cuda.current_stream().cuda_stream), "abub_train_dev")
    torch.cuda.synchronize()
    assert canaries_intact(mbuf, off[1], P) and canaries_intact(sbuf, off[2], P), (P, off)
    assert canaries_intact(fbuf, off[0], st.size) and np.array_equal(f_d.cpu().numpy(), st.ravel())
    mu = mbuf[off[1]:off[1] + P].cpu().numpy().reshape(H, W)
    sg = sbuf[off[2]:off[2] + P].cpu().numpy().reshape(H, W)
    return mu, sg


def check(oracle, st, **kw):
    mu_r, sg_r = oracle.welford(st)
    mu, sg = train(st, **kw)
    bad = np.flatnonzero((mu != mu_r).ravel() | (sg != sg_r).ravel())
    assert bad.size == 0, (st.shape, kw, bad.size, bad[:8], mu.ravel()[bad[:8]], mu_r.ravel()[bad[:8]],
                           sg.ravel()[bad[:8]], sg_r.ravel()[bad[:8]])
    return mu_r, sg_r


# ------------------------------------------------------------------------------------------------------------------
# the designed set through both kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["dword", "byte"])
def test_designed_set(oracle, groups, kernel):
    """One call per N.  'dword': every pixel of the group as an 8-row plane (P % 4 == 0, k1_welford4).  'byte': the
    last pixel dropped, so that P is odd (k1_welford)."""
    for N, g in groups.items():
        n = g.shape[1]
        st = trainref.as_plane(g, 8, n // 8) if kernel == "dword" else trainref.as_plane(g, 1, n - 1)
        assert (st.shape[1] * st.shape[2]) % 4 == (0 if kernel == "dword" else 3)
        check(oracle, st)


# ------------------------------------------------------------------------------------------------------------------
# idx
# ------------------------------------------------------------------------------------------------------------------
def slab40(groups, H, W):
    """40 frames: the designed group of N = 36 (order matters there) and four frames of noise."""
    rs = np.random.RandomState(40)
    return np.concatenate([trainref.as_plane(groups[36], H, W), rs.randint(0, 256, (4, H, W)).astype(np.uint8)])


@pytest.mark.parametrize("H,W", [(13, 20), (13, 21)], ids=["dword", "byte"])
def test_idx_forms(oracle, groups, H, W):
    st = slab40(groups, H, W)
    f_all = oracle.welford(st)
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(DEV)  # noqa: E731

    def through_idx(ix, idx_d=None):
        ix = np.asarray(ix)
        mu_r, sg_r = oracle.welford(st[ix])
        mu, sg = train(st, idx=dev(ix) if idx_d is None else idx_d)
        assert np.array_equal(mu, mu_r) and np.array_equal(sg, sg_r), ix
        return mu_r, sg_r

    # NULL is 0 .. N-1
    for got in (train(st), train(st, idx=dev(np.arange(40)))):
        assert np.array_equal(got[0], f_all[0]) and np.array_equal(got[1], f_all[1])
    # NULL with N below the slab's frame count: the first N frames
    first = oracle.welford(st[:36])
    got = train(st, N=36)
    assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    # a permutation: the frames in idx's order, not in the slab's
    through_idx(np.random.RandomState(7).permutation(40))
    # descending over the designed frames: the same set as st[:36] in another order, and another result
    down = through_idx(np.arange(35, -1, -1))
    assert not (np.array_equal(down[0], first[0]) and np.array_equal(down[1], first[1]))
    # repeated indices
    rep = through_idx([5, 5, 5, 39, 7, 7, 0, 39, 5])
    assert rep[1].any()
    through_idx([17] * 6)
    # a view that starts at an odd element of a larger tensor (4-byte aligned, not 8)
    perm = np.random.RandomState(8).permutation(40)[:25]
    big = dev(np.concatenate([[39, 38, 37], perm, [0, 1, 2]]))
    view = big[3:3 + 25]
    assert view.data_ptr() % 8 == 4
    through_idx(perm, idx_d=view)


# ------------------------------------------------------------------------------------------------------------------
# plane sizes, canaries, addresses
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028])
def test_plane_sizes(oracle, groups, P):
    """Round one block of the byte kernel (256 pixels) and one block of the dword kernel (1024 pixels: 1028 is the
    first P that takes k1_welford4 with two blocks).  mu and sigma are views at a 4-byte offset inside canary-filled
    tensors (train() asserts that the bytes round them stay)."""
    for N in (9, 16):
        check(oracle, trainref.as_plane(groups[N], 1, P))


def test_any_byte_address(oracle, groups):
    """frames, mu and sigma at byte offsets 1 to 3, one at a time and all at once, on a plane with P % 4 == 0: the
    same bytes as the aligned call (which the oracle pins)."""
    st = trainref.as_plane(groups[16], 8, groups[16].shape[1] // 8)
    assert st[0].size % 4 == 0
    mu_r, sg_r = check(oracle, st, off=(0, 0, 0))
    for o in (1, 2, 3):
        for off in ((o, 0, 0), (0, o, 0), (0, 0, o), (o, o, o), (o, 4 - o, (o + 1) % 4)):
            mu, sg = train(st, off=off)
            assert np.array_equal(mu, mu_r) and np.array_equal(sg, sg_r), off
    # and with P % 4 != 0 nothing is assumed of the addresses either
    st = trainref.as_plane(groups[9], 1, 1027)
    mu_r, sg_r = check(oracle, st, off=(0, 0, 0))
    for off in ((1, 2, 3), (3, 1, 2)):
        mu, sg = train(st, off=off)
        assert np.array_equal(mu, mu_r) and np.array_equal(sg, sg_r), off


# ------------------------------------------------------------------------------------------------------------------
# degenerate N and planes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 5), (3, 7)], ids=["dword", "byte"])
def test_short_and_constant_stacks(oracle, H, W):
    rs = np.random.RandomState(5)
    one = rs.randint(0, 256, (1, H, W)).astype(np.uint8)
    mu, sg = check(oracle, one)  # N = 1: 0 / 0, sigma is defined as 0
    assert np.array_equal(mu, one[0]) and not sg.any()
    two = np.empty((2, H, W), np.uint8)
    two[0], two[1] = 0, 255
    mu, sg = check(oracle, two)
    assert (mu == 127).all() and (sg == 180).all()
    two[0] = 255
    mu, sg = check(oracle, two)
    assert (mu == 255).all() and not sg.any()
    for v in (0, 255):
        mu, sg = check(oracle, np.full((7, H, W), v, np.uint8))
        assert (mu == v).all() and not sg.any()


def test_long_run(oracle):
    st = trainref.noisy_frames(np.random.RandomState(300), 300, 16, 16, amp=3)
    check(oracle, st)
    check(oracle, np.ascontiguousarray(st[:, :15, :15]))  # P = 225: the byte kernel


# ------------------------------------------------------------------------------------------------------------------
# through the context
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames", [16, 4])
def test_ctx_train_designed_group(oracle, groups, max_frames):
    """N = 16 with max_frames 16 (the set fits the context's slab) and 4 (it does not); the model left resident is
    the oracle's too."""
    g = groups[16]
    H, W = 8, g.shape[1] // 8
    tr = trainref.as_plane(g, H, W)
    mu_r, sg_r = oracle.welford(tr)
    assert ((sg_r > 0) & (sg_r < 43)).sum() > 100  # pixels where 6 sigma neither vanishes nor saturates
    rs = np.random.RandomState(16)
    fr = rs.randint(0, 256, (4, H, W)).astype(np.uint8)
    fr[0], fr[3] = 0, 255
    with Ctx(W, H, max_frames) as ctx:
        rc, mu, sg = ctx.train(list(tr))
        assert rc == OK
        assert np.array_equal(mu, mu_r) and np.array_equal(sg, sg_r)
        assert ctx.upload(list(fr)) == OK
        D = oracle.process_frame(fr[3], fr[0], sg_r)
        assert D.any()
        rc, Dg, hg = ctx.diff_frame(3, 0)
        assert rc == OK and np.array_equal(Dg, D) and np.array_equal(hg, oracle.hist256(D))
        for i in (0, 2, 3):
            Oi = oracle.posttrig_frame(fr[i], mu_r, sg_r)
            assert Oi.any()
            rc, Og, hg = ctx.posttrig(i)
            assert rc == OK and np.array_equal(Og, Oi) and np.array_equal(hg, oracle.hist256(Oi)), i
