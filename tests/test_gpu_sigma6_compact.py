"""abub_sigma6_dev against its definition, and K4 (abub_fg_compact_dev, abub_fg_compact_pairs_dev) against numpy at the
seams of both kernels: the 16-byte path and the byte path, the all-zero-dword shortcut under every sign of the
threshold, the second step of both capped grids, capacities at and just under the true count, and any byte address
for the images (the 16-byte path is taken only for aligned ones, include/abub_hip.h).

The lists are unordered (one atomic per entry), so a list is compared as a sorted set; on overflow the entries that
were stored are distinct members of the expected set."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib  # noqa: E402

DEV = "cuda:0"
CAN = 0xC3          # canary byte
SENT = 0x5A5A5A5A   # canary word
PAD = 64
THRS = (-1, 0, 1, 254, 255)


def _st():
    return torch.cuda.current_stream().cuda_stream


def u32(t):
    return t.cpu().numpy().astype(np.uint32)


def dev_at(a, off):
    """`a` at byte offset `off` of a canary-filled device buffer -> (buffer, view of the copy)."""
    buf = torch.full((off + a.size + PAD,), CAN, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size]
    if a.size:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return buf, view


def untouched(buf, off, a):
    """The buffer made by dev_at(a, off) still holds the canaries and `a`."""
    b = buf.cpu().numpy()
    return (b[:off] == CAN).all() and (b[off + a.size:] == CAN).all() and np.array_equal(b[off:off + a.size], a.ravel())


# ------------------------------------------------------------------------------------------------------------------
# sigma6
# ------------------------------------------------------------------------------------------------------------------
def sigma6(s, off_in=0, off_out=0, n=None):
    n = s.size if n is None else n
    ibuf, i_d = dev_at(s, off_in)
    obuf = torch.full((off_out + s.size + PAD,), CAN, dtype=torch.uint8, device=DEV)
    assert obuf.data_ptr() % 16 == 0
    _lib.check(_lib.lib().abub_sigma6_dev(ibuf.data_ptr() + off_in, obuf.data_ptr() + off_out, n, _st()), "abub_sigma6_dev")
    torch.cuda.synchronize()
    assert untouched(ibuf, off_in, s)
    return obuf.cpu().numpy()


def test_sigma6_every_value():
    s = np.arange(256, dtype=np.uint8)
    exp = np.minimum(6 * s.astype(np.int32), 255).astype(np.uint8)
    assert exp[42] == 252 and exp[43] == 255 and exp[255] == 255
    out = sigma6(s)
    assert np.array_equal(out[:256], exp) and (out[256:] == CAN).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 257])
def test_sigma6_sizes_and_addresses(n):
    """One block and its boundary; the grid is capped at 4096 blocks of 256, so at n = 4096 * 256 + 257 the loop runs
    a second step, in 257 threads.  Input and output at byte offsets 0 to 3."""
    rs = np.random.RandomState(n % 9973)
    s = rs.randint(0, 256, n).astype(np.uint8)
    s[-1], s[0] = 43, 42
    if n > 4096 * 256:
        s[4096 * 256 - 1: 4096 * 256 + 2] = (41, 42, 44)
    exp = np.minimum(6 * s.astype(np.int32), 255).astype(np.uint8)
    for off_in, off_out in ((0, 0), (1, 2), (2, 3), (3, 1), (0, 3), (2, 0)):
        out = sigma6(s, off_in, off_out)
        assert (out[:off_out] == CAN).all() and (out[off_out + n:] == CAN).all(), (off_in, off_out)
        assert np.array_equal(out[off_out:off_out + n], exp), (off_in, off_out)


def test_sigma6_of_nothing():
    out = sigma6(np.arange(256, dtype=np.uint8), 1, 1, n=0)
    assert (out == CAN).all()


# ------------------------------------------------------------------------------------------------------------------
# K4
# ------------------------------------------------------------------------------------------------------------------
VALUES = np.array([1, 2, 3, 128, 254, 255], np.uint8)


def sparse(rs, H, W, nfg):
    img = np.zeros(H * W, np.uint8)
    at = rs.choice(H * W, min(nfg, H * W), replace=False)
    img[at] = VALUES[rs.randint(0, len(VALUES), at.size)]
    return img.reshape(H, W)


def images(H, W):
    """name -> image: the hard planes of the issue at this size."""
    P = H * W
    rs = np.random.RandomState(H * 4099 + W)
    out = {"zero": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    ends = np.zeros(P, np.uint8)
    ends[0], ends[P - 1] = 255, 1
    out["ends"] = ends.reshape(H, W)
    # dwords with exactly one non-zero byte, in each of the four positions in turn (and every other dword zero)
    one = np.zeros(P, np.uint8)
    j = np.arange(0, P // 4, 2)
    one[4 * j + (j // 2) % 4] = VALUES[(j // 2) % len(VALUES)]
    out["onebyte"] = one.reshape(H, W)
    out["sparse"] = sparse(rs, H, W, max(P // 50, 3))
    return out


def fg_compact(img, thr, cap, off=0):
    """abub_fg_compact_dev on img [n, H, W] at byte offset `off` -> (count [n], idx [n * cap + PAD] with canaries)."""
    n, H, W = img.shape
    ibuf, i_d = dev_at(img, off)
    t_d = torch.tensor(list(thr), dtype=torch.int32, device=DEV)
    idx = torch.full((n * cap + PAD,), SENT, dtype=torch.int32, device=DEV)
    cnt = torch.full((n,), 12345, dtype=torch.int32, device=DEV)  # the launcher zeroes it
    _lib.check(_lib.lib().abub_fg_compact_dev(i_d.data_ptr(), n, W, H, t_d.data_ptr(), idx.data_ptr(), cap, cnt.data_ptr(),
                                              _st()), "abub_fg_compact_dev")
    torch.cuda.synchronize()
    assert untouched(ibuf, off, img)
    return u32(cnt), u32(idx)


def fg_pairs(img, thr, cap, off=0):
    """abub_fg_compact_pairs_dev -> (count, pairs [cap + PAD, 2] with canaries)."""
    n, H, W = img.shape
    ibuf, i_d = dev_at(img, off)
    t_d = torch.tensor(list(thr), dtype=torch.int32, device=DEV)
    pairs = torch.full((cap + PAD, 2), SENT, dtype=torch.int32, device=DEV)
    count = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().abub_fg_compact_pairs_dev(i_d.data_ptr(), n, W, H, t_d.data_ptr(), pairs.data_ptr(), cap,
                                                    count.data_ptr(), _st()), "abub_fg_compact_pairs_dev")
    torch.cuda.synchronize()
    assert untouched(ibuf, off, img)
    return int(u32(count)[0]), u32(pairs)


def expected(img, thr):
    return [np.flatnonzero(im.ravel() > t) for im, t in zip(img, thr)]


def check_lists(img, thr, cap, off=0):
    """Per-image lists: the true count whatever cap is; min(count, cap) distinct members of the expected set, all of it
    when it fits; nothing at or behind idx[k][cap) -- the next image's row holds that image's entries only -- and
    nothing behind the last row."""
    n = len(img)
    exp = expected(img, thr)
    ct, ix = fg_compact(img, thr, cap, off)
    assert (ix[n * cap:] == SENT).all(), (thr, cap, off)
    for k in range(n):
        assert ct[k] == len(exp[k]), (k, thr[k], cap, off, ct[k], len(exp[k]))
        row = ix[k * cap:(k + 1) * cap]
        m = min(len(exp[k]), cap)
        assert (row[m:] == SENT).all(), (k, thr[k], cap, off)
        got = np.sort(row[:m])
        if len(exp[k]) <= cap:
            assert np.array_equal(got, exp[k]), (k, thr[k], cap, off)
        else:
            assert len(np.unique(got)) == cap and np.isin(got, exp[k]).all(), (k, thr[k], cap, off)


def check_pairs(img, thr, cap, off=0):
    """The shared list: the true total; min(total, cap) distinct (image, index) entries of the expected set, each with
    its image's tag in the low 24 bits and the pixel's value in the high byte; nothing behind pairs[cap)."""
    n, P = len(img), img[0].size
    exp = expected(img, thr)
    total = sum(len(e) for e in exp)
    count, pr = fg_pairs(img, thr, cap, off)
    assert count == total, (thr, cap, off, count, total)
    assert (pr[cap:] == SENT).all(), (thr, cap, off)
    m = min(total, cap)
    assert (pr[m:cap] == SENT).all(), (thr, cap, off)
    slot, val, ix = pr[:m, 0] & 0xFFFFFF, pr[:m, 0] >> 24, pr[:m, 1]
    assert (slot < n).all() and (ix < P).all(), (thr, cap, off)
    assert np.array_equal(val, img.reshape(n, P)[slot, ix]), (thr, cap, off)
    keys = slot.astype(np.int64) * P + ix
    want = np.concatenate([k * P + e for k, e in enumerate(exp)]) if total else np.zeros(0, np.int64)
    if total <= cap:
        assert np.array_equal(np.sort(keys), want), (thr, cap, off)
    else:
        assert len(np.unique(keys)) == cap and np.isin(keys, want).all(), (thr, cap, off)


SMALL = [(3, 5), (16, 1), (64, 80), (333, 77)]  # H x W; 15 and 25641 pixels are no multiple of 16


@pytest.mark.parametrize("H,W", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_k4_every_image_under_every_threshold(H, W):
    P = H * W
    for name, im in images(H, W).items():
        for t in THRS:
            n_exp = int((im.astype(int) > t).sum())
            assert n_exp == {"zero": P if t < 0 else 0, "full": P if t < 255 else 0}.get(name, n_exp)
            check_lists(im[None], [t], P)
            check_pairs(im[None], [t], P)


@pytest.mark.parametrize("H,W", [(512, 513), (2048, 1025)], ids=["512x513", "2048x1025"])
def test_k4_second_loop_step(H, W):
    """P % 16 == 0 at both sizes.  512 x 513 is 513 pixels more than the pairs form's 64 blocks cover in one step,
    2048 x 1025 is 2048 more than the 512 blocks of abub_fg_compact_dev do: the foreground is sparse, with pixels in
    the part that only the second step reads, its first and last among them.  Under thr = -1 every pixel is listed,
    the zero dwords too: the list overflows and reports P."""
    P = H * W
    assert P % 16 == 0
    step = (64 if H == 512 else 512) * 256 * 16
    assert step < P < 2 * step
    rs = np.random.RandomState(W)
    im = sparse(rs, H, W, 3000).ravel()
    im[[0, step - 1, step, P - 1]] = (255, 254, 1, 2)
    im[step + 1 + rs.choice(P - step - 2, 20, replace=False)] = 255
    im = im.reshape(1, H, W)
    cap = 4096
    for t in THRS:
        n_exp = int((im.astype(int) > t).sum())
        assert n_exp == P if t < 0 else n_exp <= 3100
        check_lists(im, [t], cap)
        check_pairs(im, [t], cap)
    # the byte kernels walk the same plane in more steps
    check_lists(im, [0], cap, off=1)
    check_pairs(im, [0], cap, off=8)


@pytest.mark.parametrize("H,W", [(64, 80), (333, 77)], ids=["64x80", "333x77"])
def test_k4_capacity(H, W):
    """cap == count, count - 1 and 1, for one image and for two (where a row that overflows must not reach into the
    next image's).  check_lists / check_pairs assert the true count, the membership of what was stored and the
    canaries behind."""
    rs = np.random.RandomState(H + W)
    a, b = sparse(rs, H, W, 300), sparse(rs, H, W, 200)
    ca, cb = int((a > 0).sum()), int((b > 0).sum())
    assert ca == 300 and cb == 200
    for cap in (ca, ca - 1, 1):
        check_lists(a[None], [0], cap)
        check_pairs(a[None], [0], cap)
        check_lists(np.stack([a, b]), [0, 0], cap)
    for cap in (ca + cb, ca + cb - 1, ca, 1):
        check_pairs(np.stack([a, b]), [0, 0], cap)
    # full images: every thread of the grid wants a place
    full = np.full((1, H, W), 255, np.uint8)
    for cap in (H * W, H * W - 1, 1):
        check_lists(full, [254], cap)
        check_pairs(full, [254], cap)


@pytest.mark.parametrize("H,W", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_k4_three_images_three_thresholds(H, W):
    ims = images(H, W)
    for names, thr in ((("sparse", "onebyte", "full"), (1, -1, 254)), (("zero", "sparse", "ends"), (-1, 254, 0)),
                       (("full", "zero", "onebyte"), (255, 0, 2))):
        img = np.stack([ims[k] for k in names])
        check_lists(img, thr, H * W)
        check_pairs(img, thr, 3 * H * W)


@pytest.mark.parametrize("H,W", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_k4_any_byte_address(H, W):
    """Images at byte offsets 1 to 3 (and 4 and 8: aligned for a dword, not for 16 bytes): the same lists as at
    offset 0, which check_lists / check_pairs pin against numpy.  With two images and P % 16 != 0 the second image
    is at an odd address even when the first is not."""
    ims = images(H, W)
    img = np.stack([ims["sparse"], ims["onebyte"]])
    for off in (0, 1, 2, 3, 4, 8):
        check_lists(img, (0, -1), H * W, off)
        check_pairs(img, (1, 0), 2 * H * W, off)
